"""MPNet encoders on the HIP path: embedders (``MPNetModel``: sentence-transformers/all-mpnet-base-v2, all-mpnet-base-v1,
multi-qa-mpnet-base-dot-v1, multi-qa-mpnet-base-cos-v1), weights in the layout of ``tt_mpnet_weights`` (include/tt_hip.h), driven by
the one host-side ``encoder.Encoder`` through the ``MPNET_*_PATH`` records.

The reference hands whatever Hugging Face name its config holds to ``HuggingFaceEmbedding`` (``services/model_manager.py:188-272``).
MPNet is the post-LN BERT layer with a learned relative-position bias added to every layer's attention scores: one
``[32 buckets][heads]`` table (``encoder.relative_attention_bias.weight``) for all layers.  The bucket of a key - query distance is
a fact of the distance alone (``bucket_of_distance``; every distance beyond +-128 shares the last bucket of its side), so the
kernels look the bias up in a per-head table over the clamped distance, built here once per weights object (``distance_table``).
Positions start at ``padding_idx + 1 = 2`` as in XLM-R; there are no token types.  Precision: bf16 or fp16; the
reference-precision default of the XLM-R / BERT family has no MPNet implementation (``precision.build_encoder``).
"""
from __future__ import annotations

import ctypes
import math
from ctypes import POINTER, Structure, c_void_p
from typing import Dict, List

import numpy as np
import torch

from .encoder import MPNET_BF16_PATH, MPNET_FP16_PATH, EncoderConfig, _EncW, _FamilyWeights, _LayerW

NUM_BUCKETS = 32       # MPNetEncoder.compute_position_bias / relative_position_bucket: both hard-coded at the call site
MAX_DISTANCE = 128
LOG2E = 1.4426950408889634


class _MpW(Structure):
    """tt_mpnet_weights."""
    _fields_ = [("enc", _EncW), ("rel_bias", c_void_p), ("bias_table", c_void_p)]


def bucket_of_distance(d: int) -> int:
    """The bucket ``MPNetEncoder.relative_position_bucket`` (32 buckets, max_distance 128) gives ``relative_position = d`` =
    key index - query index.  With n = -d: 16 [n < 0] + f(|n|), f(m) = m below 8, else
    min(15, 8 + trunc(log(m / 8) / log(16) * 8)) -- in fp32 as transformers computes it (the steps, at m = 12, 16, 23, 32, 46, 64
    and 91, are those of exact arithmetic)."""
    n = -int(d)
    half, exact = NUM_BUCKETS // 2, NUM_BUCKETS // 4
    ret = half if n < 0 else 0
    m = abs(n)
    if m < exact:
        return ret + m
    ratio = np.log(np.float32(m) / np.float32(exact), dtype=np.float32) / np.float32(math.log(MAX_DISTANCE / exact))
    return ret + min(half - 1, exact + int(ratio * np.float32(half - exact)))


def distance_buckets() -> np.ndarray:
    """int64 [257]: the bucket of every clamped distance d = key - query in [-128, 128].  |d| >= 91 is bucket 15 (or 31) already,
    so clamping a longer distance to +-128 does not change its bucket."""
    return np.asarray([bucket_of_distance(d) for d in range(-MAX_DISTANCE, MAX_DISTANCE + 1)], dtype=np.int64)


def distance_table(rel_bias: torch.Tensor) -> torch.Tensor:
    """``rel_bias`` [32][heads] (the checkpoint's layout) -> fp32 [heads][257]: table[h][d + 128] = rel_bias[bucket(d)][h] *
    log2(e), what ``tt_attention_relbias`` adds to a score in its log2 domain."""
    if rel_bias.dim() != 2 or rel_bias.shape[0] != NUM_BUCKETS:
        raise ValueError(f"relative_attention_bias {tuple(rel_bias.shape)}: expected [{NUM_BUCKETS}][heads]")
    idx = torch.from_numpy(distance_buckets()).to(rel_bias.device)
    return (rel_bias.to(torch.float32)[idx] * LOG2E).t().contiguous()


_LAYER_TENSORS = ([f"attention.attn.{n}.{p}" for n in "qkvo" for p in ("weight", "bias")]
                  + [f"{m}.{p}" for m in ("attention.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm")
                     for p in ("weight", "bias")])
# tensors of the checkpoint that play no part: sentence-transformers never reads the pooler, position_ids is a buffer
_IGNORED = {"pooler.dense.weight", "pooler.dense.bias", "embeddings.position_ids"}


def state_names(cfg: EncoderConfig) -> List[str]:
    """The checkpoint tensors an MPNet of ``cfg`` carries (after an ``mpnet.`` prefix is stripped)."""
    names = ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.LayerNorm.weight",
             "embeddings.LayerNorm.bias", "encoder.relative_attention_bias.weight"]
    for i in range(cfg.layers):
        names += [f"encoder.layer.{i}.{t}" for t in _LAYER_TENSORS]
    return names


def check_config(cfg: EncoderConfig) -> None:
    """The shapes the MPNet kernels take (tt_mpnet_forward refuses the others before a launch; say so here first)."""
    H, nh = cfg.hidden, cfg.heads
    if H % 128 or H > 1024:
        raise NotImplementedError(f"mpnet: hidden_size={H} (a multiple of 128 up to 1024, the scan's limit)")
    if nh <= 0 or H != 64 * nh:
        raise NotImplementedError(f"mpnet: hidden_size={H} with num_attention_heads={nh}: head_dim must be 64")
    if cfg.ffn <= 0 or cfg.ffn % 128:
        raise NotImplementedError(f"mpnet: intermediate_size={cfg.ffn} (a multiple of 128)")
    if cfg.num_labels:
        raise NotImplementedError("mpnet: classification heads are not supported (embedders only)")


def _strip(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in state.items():
        for pre in ("0.auto_model.", "mpnet."):
            if k.startswith(pre):
                k = k[len(pre):]
        out[k] = v
    return out


def check_state(cfg: EncoderConfig, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``state`` without its ``mpnet.`` prefix, after checking that it holds every tensor of ``state_names(cfg)`` and nothing the
    forward would not read: a masked-LM head, a classifier ... mean another export of the architecture and are refused by name,
    not ignored.  ``pooler.dense.*`` and ``embeddings.position_ids`` play no part."""
    sd = _strip(state)
    names = state_names(cfg)
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"checkpoint is not an MPNet of {cfg}: missing {missing[:4]}")
    extra = sorted(set(sd) - set(names) - _IGNORED)
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the MPNet path does not compute: {extra[:4]}")
    return sd


class MpnetWeights(_FamilyWeights):
    """Device-resident MPNet weights for ``tt_mpnet_forward`` (bf16) or ``tt_mpnet_forward_f16`` (fp16): the projections (q, k, v
    rows concatenated to [3H][H]) and the embedding tables in the element type; biases, LayerNorm parameters, the checkpoint's
    bias table and the per-head distance table built from it in fp32."""

    _paths, _path_name = (MPNET_BF16_PATH, MPNET_FP16_PATH), "the MPNet path"

    def __init__(self, cfg: EncoderConfig, state: Dict[str, torch.Tensor], device: torch.device, dtype: torch.dtype = torch.bfloat16):
        self._begin(cfg, device, dtype)
        check_config(cfg)
        sd = check_state(cfg, state)
        mat, vec = self._loaders(sd)
        H, F = cfg.hidden, cfg.ffn
        enc = _EncW(hidden=H, layers=cfg.layers, heads=cfg.heads, ffn=F, vocab=cfg.vocab_size, max_pos=cfg.max_pos, type_vocab=1,
                    ln_eps=cfg.ln_eps, word_emb=mat(["embeddings.word_embeddings.weight"], (cfg.vocab_size, H)),
                    pos_emb=mat(["embeddings.position_embeddings.weight"], (cfg.max_pos, H)),
                    emb_ln_g=vec(["embeddings.LayerNorm.weight"], H), emb_ln_b=vec(["embeddings.LayerNorm.bias"], H))
        self._layers = (_LayerW * max(cfg.layers, 1))()
        for i in range(cfg.layers):
            p, L = f"encoder.layer.{i}.", self._layers[i]
            qkv = [p + f"attention.attn.{n}." for n in "qkv"]
            L.qkv_w, L.qkv_b = mat([m + "weight" for m in qkv], (3 * H, H)), vec([m + "bias" for m in qkv], 3 * H)
            L.o_w, L.o_b = mat([p + "attention.attn.o.weight"], (H, H)), vec([p + "attention.attn.o.bias"], H)
            L.ln1_g, L.ln1_b = vec([p + "attention.LayerNorm.weight"], H), vec([p + "attention.LayerNorm.bias"], H)
            L.ffn1_w, L.ffn1_b = mat([p + "intermediate.dense.weight"], (F, H)), vec([p + "intermediate.dense.bias"], F)
            L.ffn2_w, L.ffn2_b = mat([p + "output.dense.weight"], (H, F)), vec([p + "output.dense.bias"], H)
            L.ln2_g, L.ln2_b = vec([p + "output.LayerNorm.weight"], H), vec([p + "output.LayerNorm.bias"], H)
        enc.layer = ctypes.cast(self._layers, POINTER(_LayerW))
        rel = sd["encoder.relative_attention_bias.weight"]
        if tuple(rel.shape) != (NUM_BUCKETS, cfg.heads):
            raise ValueError(f"encoder.relative_attention_bias.weight {tuple(rel.shape)} does not match {cfg} "
                             f"(expected {(NUM_BUCKETS, cfg.heads)})")
        rel = self._kept(rel.to(device=device, dtype=torch.float32).contiguous())
        self.bias_table = self._kept(distance_table(rel))
        self.struct = _MpW(enc=enc, rel_bias=rel.data_ptr(), bias_table=self.bias_table.data_ptr())


def synthetic_state(cfg: EncoderConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random MPNet weights of ``cfg`` (fp32, CPU) with trained-model-like scales: N(0, 0.02) projections and embeddings,
    LayerNorm weights around 1, and a bias table several units wide, as the published checkpoints' are (benchmarks and tests)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std=0.02):
        return torch.randn(*shape, generator=g) * std

    H, F = cfg.hidden, cfg.ffn
    sd = {"embeddings.word_embeddings.weight": rnd(cfg.vocab_size, H), "embeddings.position_embeddings.weight": rnd(cfg.max_pos, H),
          "embeddings.LayerNorm.weight": 1 + rnd(H, std=0.1), "embeddings.LayerNorm.bias": rnd(H, std=0.05),
          "encoder.relative_attention_bias.weight": rnd(NUM_BUCKETS, cfg.heads, std=2.0)}
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        for n in "qkvo":
            sd[p + f"attention.attn.{n}.weight"], sd[p + f"attention.attn.{n}.bias"] = rnd(H, H), rnd(H)
        sd[p + "attention.LayerNorm.weight"], sd[p + "attention.LayerNorm.bias"] = 1 + rnd(H, std=0.1), rnd(H, std=0.05)
        sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"] = rnd(F, H), rnd(F)
        sd[p + "output.dense.weight"], sd[p + "output.dense.bias"] = rnd(H, F), rnd(H)
        sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"] = 1 + rnd(H, std=0.1), rnd(H, std=0.05)
    return sd


# the published geometry (sentence-transformers/all-mpnet-base-v2 config.json; the four checkpoints share it)
MPNET_BASE = EncoderConfig(arch="mpnet", vocab_size=30527, hidden=768, layers=12, heads=12, ffn=3072, max_pos=514, type_vocab=1,
                           pad_id=1, ln_eps=1e-5)
KNOWN_CONFIGS = {name: MPNET_BASE for name in (
    "sentence-transformers/all-mpnet-base-v2", "sentence-transformers/all-mpnet-base-v1",
    "sentence-transformers/multi-qa-mpnet-base-dot-v1", "sentence-transformers/multi-qa-mpnet-base-cos-v1")}
