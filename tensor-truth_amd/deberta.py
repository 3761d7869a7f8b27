"""DeBERTa-v2 / v3 cross-encoders on the HIP path (``DebertaV2ForSequenceClassification``: mixedbread-ai/mxbai-rerank-xsmall-v1 /
-base-v1 / -large-v1, the deberta-v3 checkpoints under cross-encoder/, fine-tunes of microsoft/deberta-v3-*), weights in the layout
of ``tt_deberta_weights`` (include/tt_hip.h), driven by the one host-side ``encoder.Encoder`` through the ``DEBERTA_*_PATH`` records.

The reference hands whatever cross-encoder name its config holds to ``SentenceTransformerRerank``
(``services/model_manager.py:333-337``).  DeBERTa-v3 is the post-LN BERT layer with disentangled attention: no absolute positions
and no token types in the embeddings (``LayerNorm(word[id])``); every layer's attention adds a content-to-position and a
position-to-content term to the content score,

    i(q, k) = clamp(bucket(q - k) + span, 0, 2 span - 1)                       span = position_buckets
    score   = (Q[q] . K[k] + Q[q] . PK[i(q, k)] + K[k] . PQ[i(q, k)]) / sqrt(3 * 64)
    PK, PQ  = key_proj / query_proj (the layer's own, with bias: share_att_key) of LayerNorm(encoder.rel_embeddings)[0 : 2 span]

``bucket`` (transformers' ``make_log_bucket_position``) is a fact of the distance alone, and PK / PQ of the weights alone: both are
built here once per weights object (``build_dist_index``; ``DebertaWeights``), so no logarithm and no per-forward projection of
the relative embeddings runs on the device.  Precision: bf16 or fp16; the reference-precision default of the XLM-R / BERT family
has no DeBERTa implementation (``precision.build_encoder``).  Cross-encoders only: a ``DebertaV2Model`` without a head is refused.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, Structure, c_int32, c_void_p
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from .encoder import DEBERTA_BF16_PATH, DEBERTA_FP16_PATH, EncoderConfig, _EncW, _FamilyWeights, _LayerW

MAX_POSITIONS = 512      # the index table a workgroup stages (csrc/varlen.h Disentangled::MAX_POS)


@dataclass(frozen=True)
class DebertaConfig(EncoderConfig):
    """The ``EncoderConfig`` fields (``max_pos`` = ``max_position_embeddings``, the longest sequence: the embeddings hold no
    position table; ``type_vocab`` 1: no token types) and what the disentangled attention reads."""

    arch: str = "deberta-v2"
    position_buckets: int = 256
    max_relative_positions: int = 512      # resolved: config.json's -1 means max_position_embeddings


class _DbW(Structure):
    """tt_deberta_weights."""
    _fields_ = [("enc", _EncW), ("pos_key", POINTER(c_void_p)), ("pos_query", POINTER(c_void_p)), ("dist_index", c_void_p),
                ("n_pos", c_int32), ("max_pos", c_int32), ("pooler_dense_wt", c_void_p), ("pooler_dense_b", c_void_p),
                ("cls_w", c_void_p), ("cls_b", c_void_p)]


def log_bucket(relative_pos: torch.Tensor, bucket_size: int, max_position: int) -> torch.Tensor:
    """transformers' ``make_log_bucket_position`` restated, in the same fp32 torch arithmetic (``ceil(log(...))`` sits on rounding
    edges: another precision or library may land one bucket off): the identity up to +-bucket_size / 2, logarithmic beyond."""
    sign = torch.sign(relative_pos)
    mid = bucket_size // 2
    abs_pos = torch.where((relative_pos < mid) & (relative_pos > -mid), torch.tensor(mid - 1).type_as(relative_pos),
                          torch.abs(relative_pos))
    log_pos = torch.ceil(torch.log(abs_pos / mid) / torch.log(torch.tensor((max_position - 1) / mid)) * (mid - 1)) + mid
    return torch.where(abs_pos <= mid, relative_pos.type_as(log_pos), log_pos * sign)


def build_dist_index(position_buckets: int, max_pos: int, max_relative_positions: Optional[int] = None) -> torch.Tensor:
    """int32 [2 max_pos - 1]: ``dist_index[d + max_pos - 1] = clamp(bucket(d) + span, 0, 2 span - 1)`` for every distance d =
    query - key in [-(max_pos - 1), max_pos - 1], span = ``position_buckets`` -- the row of PK and of PQ both position terms of the
    pair read (the bucket is odd in d, so the position-to-content term's ``-bucket(k - q)`` is the same index).  Non-decreasing."""
    if position_buckets <= 0 or max_pos <= 0:
        raise ValueError(f"build_dist_index: position_buckets={position_buckets} max_pos={max_pos}")
    mrp = max_pos if max_relative_positions is None or max_relative_positions < 1 else max_relative_positions
    d = torch.arange(-(max_pos - 1), max_pos, dtype=torch.long)
    b = log_bucket(d, position_buckets, mrp).to(torch.long)
    idx = torch.clamp(b + position_buckets, 0, 2 * position_buckets - 1).to(torch.int32)
    if (idx[1:] < idx[:-1]).any():
        raise ValueError("build_dist_index: the bucket index is not monotone in the distance")
    return idx


_LAYER_TENSORS = ([f"attention.self.{n}_proj.{p}" for n in ("query", "key", "value") for p in ("weight", "bias")]
                  + [f"{m}.{p}" for m in ("attention.output.dense", "attention.output.LayerNorm", "intermediate.dense", "output.dense",
                                          "output.LayerNorm") for p in ("weight", "bias")])
_HEAD_TENSORS = ["pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias"]
# buffers of older exports that play no part
_IGNORED = {"embeddings.position_ids"}


def state_names(cfg: EncoderConfig) -> List[str]:
    """The checkpoint tensors a DeBERTa-v3 cross-encoder of ``cfg`` carries (after the ``deberta.`` prefix is stripped)."""
    names = ["embeddings.word_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias",
             "encoder.rel_embeddings.weight", "encoder.LayerNorm.weight", "encoder.LayerNorm.bias"]
    for i in range(cfg.layers):
        names += [f"encoder.layer.{i}.{t}" for t in _LAYER_TENSORS]
    return names + (_HEAD_TENSORS if cfg.num_labels else [])


def check_config(cfg: EncoderConfig) -> None:
    """The shapes the DeBERTa kernels take (tt_deberta_forward refuses the others before a launch; say so here first)."""
    H, nh = cfg.hidden, cfg.heads
    if H % 128 or H > 1024:
        raise NotImplementedError(f"deberta-v2: hidden_size={H} (a multiple of 128 up to 1024, the scan's limit)")
    if nh <= 0 or H != 64 * nh:
        raise NotImplementedError(f"deberta-v2: hidden_size={H} with num_attention_heads={nh}: head_dim must be 64")
    if cfg.ffn <= 0 or cfg.ffn % 128:
        raise NotImplementedError(f"deberta-v2: intermediate_size={cfg.ffn} (a multiple of 128)")
    if cfg.position_buckets <= 0 or cfg.position_buckets % 2:
        raise NotImplementedError(f"deberta-v2: position_buckets={cfg.position_buckets} (a positive even number)")
    if cfg.max_pos > MAX_POSITIONS:
        raise NotImplementedError(f"deberta-v2: max_position_embeddings={cfg.max_pos} (up to {MAX_POSITIONS}: the distance table a "
                                  "workgroup stages)")
    if cfg.num_labels != 1:
        raise NotImplementedError(
            "deberta-v2: only single-label cross-encoders (DebertaV2ForSequenceClassification) are served; a DebertaV2Model without "
            "a classification head (an embedder) is out of scope" if not cfg.num_labels else
            f"deberta-v2 classification checkpoint with num_labels={cfg.num_labels}: only single-label cross-encoder heads are "
            "supported")


def _strip(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {(k[len("deberta."):] if k.startswith("deberta.") else k): v for k, v in state.items()}


def check_state(cfg: EncoderConfig, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``state`` without its ``deberta.`` prefix, after checking that it holds every tensor of ``state_names(cfg)`` and nothing the
    forward would not read: ``pos_key_proj`` / ``pos_query_proj`` (share_att_key false), position or token-type embeddings, a
    convolution, an ``embed_proj``, a masked-LM head ... mean a variant the kernels do not compute and are refused by name, not
    ignored.  ``embeddings.position_ids`` plays no part."""
    sd = _strip(state)
    own = [k for k in sd if "pos_key_proj" in k or "pos_query_proj" in k]
    if own:
        raise NotImplementedError(f"deberta-v2 checkpoint carries pos_key_proj / pos_query_proj tensors ({own[:2]}): share_att_key "
                                  "false is not computed")
    names = state_names(cfg)
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"checkpoint is not a DeBERTa-v2 cross-encoder of {cfg}: missing {missing[:4]}")
    extra = sorted(set(sd) - set(names) - _IGNORED)
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the DeBERTa path does not compute: {extra[:4]}")
    return sd


class DebertaWeights(_FamilyWeights):
    """Device-resident DeBERTa weights for ``tt_deberta_forward`` (bf16) or ``tt_deberta_forward_f16`` (fp16): the projections
    (query, key, value rows concatenated to [3H][H]) and the word table in the element type; biases, LayerNorm parameters and the
    head in fp32; per layer PK / PQ = key_proj / query_proj of the normalised relative embeddings (fp32 torch on the device,
    rounded once to the element type) and the distance table -- all built here, once."""

    _paths, _path_name = (DEBERTA_BF16_PATH, DEBERTA_FP16_PATH), "the DeBERTa path"

    def __init__(self, cfg: EncoderConfig, state: Dict[str, torch.Tensor], device: torch.device, dtype: torch.dtype = torch.bfloat16):
        self._begin(cfg, device, dtype)
        check_config(cfg)
        sd = check_state(cfg, state)
        mat, vec = self._loaders(sd, flatten=True)       # classifier.weight is a [1][H] row
        H, F, n_pos = cfg.hidden, cfg.ffn, 2 * cfg.position_buckets
        enc = _EncW(hidden=H, layers=cfg.layers, heads=cfg.heads, ffn=F, vocab=cfg.vocab_size, max_pos=cfg.max_pos, type_vocab=1,
                    ln_eps=cfg.ln_eps, word_emb=mat(["embeddings.word_embeddings.weight"], (cfg.vocab_size, H)),
                    emb_ln_g=vec(["embeddings.LayerNorm.weight"], H), emb_ln_b=vec(["embeddings.LayerNorm.bias"], H))
        rel = sd["encoder.rel_embeddings.weight"]
        if rel.dim() != 2 or rel.shape[0] < n_pos or rel.shape[1] != H:
            raise ValueError(f"encoder.rel_embeddings.weight {tuple(rel.shape)} does not match {cfg} (expected [{n_pos}][{H}])")
        f32 = dict(device=device, dtype=torch.float32)
        rel = torch.nn.functional.layer_norm(rel[:n_pos].to(**f32), (H,), sd["encoder.LayerNorm.weight"].to(**f32),
                                             sd["encoder.LayerNorm.bias"].to(**f32), cfg.ln_eps)
        self._layers = (_LayerW * max(cfg.layers, 1))()
        self._pos_key = (c_void_p * max(cfg.layers, 1))()
        self._pos_query = (c_void_p * max(cfg.layers, 1))()
        self.pos_key: List[torch.Tensor] = []
        self.pos_query: List[torch.Tensor] = []
        for i in range(cfg.layers):
            p, L = f"encoder.layer.{i}.", self._layers[i]
            qkv = [p + f"attention.self.{n}_proj." for n in ("query", "key", "value")]
            L.qkv_w, L.qkv_b = mat([m + "weight" for m in qkv], (3 * H, H)), vec([m + "bias" for m in qkv], 3 * H)
            L.o_w, L.o_b = mat([p + "attention.output.dense.weight"], (H, H)), vec([p + "attention.output.dense.bias"], H)
            L.ln1_g, L.ln1_b = vec([p + "attention.output.LayerNorm.weight"], H), vec([p + "attention.output.LayerNorm.bias"], H)
            L.ffn1_w, L.ffn1_b = mat([p + "intermediate.dense.weight"], (F, H)), vec([p + "intermediate.dense.bias"], F)
            L.ffn2_w, L.ffn2_b = mat([p + "output.dense.weight"], (H, F)), vec([p + "output.dense.bias"], H)
            L.ln2_g, L.ln2_b = vec([p + "output.LayerNorm.weight"], H), vec([p + "output.LayerNorm.bias"], H)
            for proj, store, ptrs in (("key", self.pos_key, self._pos_key), ("query", self.pos_query, self._pos_query)):
                t = torch.nn.functional.linear(rel, sd[p + f"attention.self.{proj}_proj.weight"].to(**f32),
                                               sd[p + f"attention.self.{proj}_proj.bias"].to(**f32))
                store.append(self._kept(t.to(dtype).contiguous()))
                ptrs[i] = store[-1].data_ptr()
        enc.layer = ctypes.cast(self._layers, POINTER(_LayerW))
        self.dist_index = self._kept(build_dist_index(cfg.position_buckets, cfg.max_pos, cfg.max_relative_positions).to(device))
        self.struct = _DbW(enc=enc, pos_key=ctypes.cast(self._pos_key, POINTER(c_void_p)),
                           pos_query=ctypes.cast(self._pos_query, POINTER(c_void_p)), dist_index=self.dist_index.data_ptr(),
                           n_pos=n_pos, max_pos=cfg.max_pos)
        if tuple(sd["pooler.dense.weight"].shape) != (H, H) or sd["classifier.weight"].numel() != H:
            raise ValueError(f"pooler.dense.weight {tuple(sd['pooler.dense.weight'].shape)} / classifier.weight "
                             f"{tuple(sd['classifier.weight'].shape)} do not match {cfg}")
        dense_t = self._kept(sd["pooler.dense.weight"].to(**f32).t().contiguous())          # [in][out]
        self.struct.pooler_dense_wt = dense_t.data_ptr()
        self.struct.pooler_dense_b = vec(["pooler.dense.bias"], H)
        self.struct.cls_w, self.struct.cls_b = vec(["classifier.weight"], H), vec(["classifier.bias"], 1)


def synthetic_state(cfg: EncoderConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random DeBERTa-v3 cross-encoder weights of ``cfg`` (fp32, CPU) with trained-model-like scales: N(0, 0.02) projections
    and word embeddings, LayerNorm weights around 1, relative embeddings of unit scale with an offset (the published checkpoints'
    are far from the +-0.02 initialisation, which would leave both position terms below 16-bit noise) (benchmarks and tests)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std=0.02):
        return torch.randn(*shape, generator=g) * std

    H, F = cfg.hidden, cfg.ffn
    sd = {"embeddings.word_embeddings.weight": rnd(cfg.vocab_size, H), "embeddings.LayerNorm.weight": 1 + rnd(H, std=0.1),
          "embeddings.LayerNorm.bias": rnd(H, std=0.05), "encoder.rel_embeddings.weight": 0.3 + rnd(2 * cfg.position_buckets, H, std=1.0),
          "encoder.LayerNorm.weight": 1 + rnd(H, std=0.1), "encoder.LayerNorm.bias": rnd(H, std=0.05)}
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        for n in ("query", "key", "value"):
            sd[p + f"attention.self.{n}_proj.weight"], sd[p + f"attention.self.{n}_proj.bias"] = rnd(H, H), rnd(H)
        sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"] = rnd(H, H), rnd(H)
        sd[p + "attention.output.LayerNorm.weight"], sd[p + "attention.output.LayerNorm.bias"] = 1 + rnd(H, std=0.1), rnd(H, std=0.05)
        sd[p + "intermediate.dense.weight"], sd[p + "intermediate.dense.bias"] = rnd(F, H), rnd(F)
        sd[p + "output.dense.weight"], sd[p + "output.dense.bias"] = rnd(H, F), rnd(H)
        sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"] = 1 + rnd(H, std=0.1), rnd(H, std=0.05)
    if cfg.num_labels:
        sd["pooler.dense.weight"], sd["pooler.dense.bias"] = rnd(H, H), rnd(H)
        sd["classifier.weight"], sd["classifier.bias"] = rnd(cfg.num_labels, H, std=0.2), rnd(cfg.num_labels)
    return sd


# the published geometry (config.json of the three mixedbread-ai/mxbai-rerank-*-v1 sizes: the deberta-v3 xsmall / base / large shapes)
def _known(hidden: int, heads: int, layers: int, ffn: int) -> DebertaConfig:
    return DebertaConfig(vocab_size=128100, hidden=hidden, layers=layers, heads=heads, ffn=ffn, max_pos=512, type_vocab=1, pad_id=0,
                         ln_eps=1e-7, num_labels=1, position_buckets=256, max_relative_positions=512)


MXBAI_RERANK_XSMALL = _known(384, 6, 12, 1536)
MXBAI_RERANK_BASE = _known(768, 12, 12, 3072)
MXBAI_RERANK_LARGE = _known(1024, 16, 24, 4096)
KNOWN_CONFIGS = {"mixedbread-ai/mxbai-rerank-xsmall-v1": MXBAI_RERANK_XSMALL, "mixedbread-ai/mxbai-rerank-base-v1": MXBAI_RERANK_BASE,
                 "mixedbread-ai/mxbai-rerank-large-v1": MXBAI_RERANK_LARGE}
