"""Decoder embedders (``Qwen3Model`` architecture: Qwen3-Embedding) and rerankers (``Qwen3ForSequenceClassification``: the form
the Qwen3-Reranker checkpoints take for cross-encoder use) on the HIP path: weights in the layout of ``tt_decoder_weights``
(include/tt_hip.h), driven by the one host-side ``encoder.Encoder`` through the ``DECODER_*_PATH`` records.

The reference embeds with whatever Hugging Face model its config names (``api/routes/startup.py:108-133``,
``services/model_manager.py:214-252``); for the Qwen3-Embedding checkpoints sentence-transformers runs ``Qwen3Model`` and pools
the LAST token (``1_Pooling/config.json``: ``pooling_mode_lasttoken``), then normalises.  Every size comes from ``config.json``
(``weights._config_from_hf``).  Precision: bf16 (what the published checkpoints declare) or fp16; the reference-precision
default of the encoder family (fp32 semantics on split planes) has no decoder implementation (``precision.build_encoder``).
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, Structure, c_float, c_int32, c_void_p
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

from .encoder import DECODER_BF16_PATH, DECODER_FP16_PATH, EncoderConfig, _FamilyWeights, _strip_prefix


@dataclass(frozen=True)
class DecoderConfig(EncoderConfig):
    """The ``EncoderConfig`` fields (``ln_eps`` = the RMSNorm epsilon) plus grouped-query attention -- ``kv_heads`` KV heads of
    ``head_dim`` each -- and the RoPE base.  ``num_labels == 1``: a ``*ForSequenceClassification`` checkpoint, whose head reads
    the token ``encoder.pooled_rows`` names: with ``pad_token_id`` set the rightmost token that differs from it, else the last
    (``pad_id`` is something else: the filler ``pack_tokens`` writes into rows of no sequence)."""

    arch: str = "qwen3"
    kv_heads: int = 0
    head_dim: int = 0
    rope_theta: float = 0.0
    pad_token_id: Optional[int] = None


class _DecLayerW(Structure):
    """tt_decoder_layer_weights."""
    _fields_ = [(n, c_void_p) for n in ("qkv_w", "q_norm", "k_norm", "o_w", "attn_norm", "ffn_norm", "gate_up_w", "down_w")]


class _DecW(Structure):
    """tt_decoder_weights."""
    _fields_ = ([(n, c_int32) for n in ("hidden", "layers", "heads", "kv_heads", "head_dim", "ffn", "vocab")]
                + [("rms_eps", c_float), ("rope_theta", c_float), ("embed", c_void_p), ("layer", POINTER(_DecLayerW)),
                   ("final_norm", c_void_p)])


def state_names(cfg: DecoderConfig) -> List[str]:
    """The checkpoint tensors a ``Qwen3Model`` of ``cfg`` carries (after the ``model.`` prefix of ``*ForCausalLM`` exports is
    stripped), in the order the weights are built from them."""
    names = ["embed_tokens.weight"]
    for i in range(cfg.layers):
        p = f"layers.{i}."
        names += [p + f"self_attn.{n}_proj.weight" for n in ("q", "k", "v", "o")]
        names += [p + "self_attn.q_norm.weight", p + "self_attn.k_norm.weight", p + "input_layernorm.weight",
                  p + "post_attention_layernorm.weight"]
        names += [p + f"mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
    return names + ["norm.weight"] + (["score.weight"] if cfg.num_labels else [])


def check_config(cfg: DecoderConfig) -> None:
    """The shapes the decoder kernels take (tt_decoder_forward refuses the others before a launch; say so here first)."""
    D, nq, nkv, H = cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.hidden
    if D not in (64, 128):
        raise NotImplementedError(f"decoder embedder: head_dim={D} (supported: 64, 128)")
    if nkv <= 0 or nq % nkv:
        raise ValueError(f"decoder embedder: num_attention_heads={nq} is not a multiple of num_key_value_heads={nkv}")
    if H % 128 or H > 1024:
        raise NotImplementedError(f"decoder embedder: hidden_size={H} (a multiple of 128 up to 1024, the scan's limit)")
    if ((nq + 2 * nkv) * D) % 128 or (nq * D) % 64 or cfg.ffn % 64:
        raise NotImplementedError(f"decoder embedder: heads={nq} kv_heads={nkv} head_dim={D} ffn={cfg.ffn} do not fit the GEMM tiles")


class DecoderWeights(_FamilyWeights):
    """Device-resident ``Qwen3Model`` weights for ``tt_decoder_forward`` (bf16) or ``tt_decoder_forward_f16`` (fp16): the
    projections in the element type -- q/k/v rows concatenated into one matrix, gate/up into another -- and the RMSNorm weights
    in fp32.  A ``*ForSequenceClassification`` checkpoint (``cfg.num_labels``) brings ``score.weight``: ``score_w``, fp32 [H], the
    operand of ``tt_decoder_score`` (transformers' head is ``Linear(H, 1, bias=False)``: a ``score.bias`` is refused like any
    other tensor the forward would not read)."""

    _paths, _path_name = (DECODER_BF16_PATH, DECODER_FP16_PATH), "the decoder embedder"

    def __init__(self, cfg: DecoderConfig, state: Dict[str, torch.Tensor], device: torch.device,
                 dtype: torch.dtype = torch.bfloat16):
        self._begin(cfg, device, dtype)
        check_config(cfg)
        if cfg.num_labels not in (0, 1):
            raise ValueError("only single-label (sigmoid) cross-encoder heads are supported")
        sd = _strip_prefix(state)
        names = state_names(cfg)
        missing = [n for n in names if n not in sd]
        if missing:
            raise ValueError(f"checkpoint is not a Qwen3Model of {cfg}: missing {missing[:4]}")
        # tensors this forward would not read (q/k/v biases, ...) mean another architecture variant: refused, not ignored.  A
        # *ForCausalLM export's lm_head, and a *ForSequenceClassification export's score head under an embedder's config, are the
        # only extras that play no part in the embedding.
        extra = sorted(set(sd) - set(names) - {"lm_head.weight", "score.weight"})
        if extra:
            raise NotImplementedError(f"checkpoint carries tensors the decoder embedder does not compute: {extra[:4]}")
        mat, vec = self._loaders(sd)
        H, D, nq, nkv, F = cfg.hidden, cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.ffn
        emb = mat(["embed_tokens.weight"], (cfg.vocab_size, H))
        self._layers = (_DecLayerW * max(cfg.layers, 1))()
        for i in range(cfg.layers):
            p, L = f"layers.{i}.", self._layers[i]
            L.qkv_w = mat([p + f"self_attn.{n}_proj.weight" for n in ("q", "k", "v")], ((nq + 2 * nkv) * D, H))
            L.o_w = mat([p + "self_attn.o_proj.weight"], (H, nq * D))
            L.gate_up_w = mat([p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"], (2 * F, H))
            L.down_w = mat([p + "mlp.down_proj.weight"], (H, F))
            L.q_norm, L.k_norm = vec([p + "self_attn.q_norm.weight"], D), vec([p + "self_attn.k_norm.weight"], D)
            L.attn_norm, L.ffn_norm = vec([p + "input_layernorm.weight"], H), vec([p + "post_attention_layernorm.weight"], H)
        self.struct = _DecW(hidden=H, layers=cfg.layers, heads=nq, kv_heads=nkv, head_dim=D, ffn=F, vocab=cfg.vocab_size,
                            rms_eps=cfg.ln_eps, rope_theta=cfg.rope_theta, embed=emb,
                            layer=ctypes.cast(self._layers, POINTER(_DecLayerW)), final_norm=vec(["norm.weight"], H))
        self.score_w: Optional[torch.Tensor] = None
        if cfg.num_labels:
            if tuple(sd["score.weight"].shape) != (1, H):
                raise ValueError(f"score.weight {tuple(sd['score.weight'].shape)} does not match {cfg} (expected (1, {H}))")
            self.score_w = self._kept(sd["score.weight"].reshape(H).to(device=device, dtype=torch.float32).contiguous())


def synthetic_state(cfg: DecoderConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random ``Qwen3Model`` weights of ``cfg`` (fp32, CPU) with trained-model-like scales: N(0, 0.02) projections and
    embeddings, RMSNorm weights around 1 (benchmarks and parity tests; no network here)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std=0.02):
        return torch.randn(*shape, generator=g) * std

    H, D, nq, nkv, F = cfg.hidden, cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.ffn
    sd = {"embed_tokens.weight": rnd(cfg.vocab_size, H), "norm.weight": 1 + rnd(H, std=0.1)}
    for i in range(cfg.layers):
        p = f"layers.{i}."
        sd[p + "self_attn.q_proj.weight"] = rnd(nq * D, H)
        sd[p + "self_attn.k_proj.weight"] = rnd(nkv * D, H)
        sd[p + "self_attn.v_proj.weight"] = rnd(nkv * D, H)
        sd[p + "self_attn.o_proj.weight"] = rnd(H, nq * D)
        sd[p + "self_attn.q_norm.weight"] = 1 + rnd(D, std=0.1)
        sd[p + "self_attn.k_norm.weight"] = 1 + rnd(D, std=0.1)
        sd[p + "input_layernorm.weight"] = 1 + rnd(H, std=0.1)
        sd[p + "post_attention_layernorm.weight"] = 1 + rnd(H, std=0.1)
        sd[p + "mlp.gate_proj.weight"] = rnd(F, H)
        sd[p + "mlp.up_proj.weight"] = rnd(F, H)
        sd[p + "mlp.down_proj.weight"] = rnd(H, F)
    if cfg.num_labels:
        sd["score.weight"] = rnd(cfg.num_labels, H, std=0.15)
    return sd


# Qwen3-Embedding-0.6B's geometry (its config.json): what the 0.6B-shaped tests and measurements build with seeded weights
QWEN3_EMBEDDING_0_6B = DecoderConfig(arch="qwen3", vocab_size=151669, hidden=1024, layers=28, heads=16, ffn=3072, max_pos=32768,
                                    type_vocab=1, pad_id=0, ln_eps=1e-6, kv_heads=8, head_dim=128, rope_theta=1e6)
