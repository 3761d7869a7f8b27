"""ModernBERT encoders on the HIP path: embedders (``ModernBertModel``: gte-modernbert, nomic modernbert-embed, the
answerdotai/ModernBERT fine-tunes) and cross-encoders (``ModernBertForSequenceClassification``: gte-reranker-modernbert), weights in
the layout of ``tt_modernbert_weights`` (include/tt_hip.h), driven by the one host-side ``encoder.Encoder`` through the
``MODERNBERT_*_PATH`` records.

The reference hands whatever Hugging Face name its config holds to ``HuggingFaceEmbedding`` and ``SentenceTransformerRerank``
(``services/model_manager.py:214-260, 333-337``).  Every size comes from ``config.json`` (``weights._config_from_hf``): the
per-layer attention type (``layer_types``), the two RoPE bases, the window.  Positions are 0-based within each sequence (RoPE; no
position table).  Precision: bf16 or fp16; the reference-precision default of the XLM-R / BERT family has no ModernBERT
implementation (``precision.build_encoder``).
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, Structure, c_float, c_int32, c_void_p
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

from .encoder import MODERNBERT_BF16_PATH, MODERNBERT_FP16_PATH, EncoderConfig, _FamilyWeights, _strip_prefix


@dataclass(frozen=True)
class ModernBertConfig(EncoderConfig):
    """The ``EncoderConfig`` fields (``ln_eps`` = ``norm_eps``; ``pad_id`` = the filler ``pack_tokens`` writes into rows of no
    sequence) plus what ModernBERT's attention reads: ``layer_types[i]`` is "full_attention" or "sliding_attention", a sliding
    layer keeps key k for query q iff ``|q - k| <= local_attention // 2`` and rotates with ``local_rope_theta``.
    ``num_labels == 1``: a ``ModernBertForSequenceClassification`` checkpoint, whose head pools as ``classifier_pooling`` says."""

    arch: str = "modernbert"
    layer_types: Tuple[str, ...] = ()
    global_rope_theta: float = 160000.0
    local_rope_theta: float = 10000.0
    local_attention: int = 128
    classifier_pooling: str = "cls"


class _MbLayerW(Structure):
    """tt_modernbert_layer_weights."""
    _fields_ = [(n, c_void_p) for n in ("qkv_w", "o_w", "attn_norm", "mlp_norm", "wi_w", "wo_w")] + [("sliding", c_int32)]


class _MbW(Structure):
    """tt_modernbert_weights."""
    _fields_ = ([(n, c_int32) for n in ("hidden", "layers", "heads", "ffn", "vocab", "local_attention")]
                + [(n, c_float) for n in ("norm_eps", "global_rope_theta", "local_rope_theta")]
                + [("embed", c_void_p), ("emb_norm", c_void_p), ("layer", POINTER(_MbLayerW)), ("final_norm", c_void_p)]
                + [(n, c_void_p) for n in ("head_dense_wt", "head_norm", "cls_w", "cls_b")])


_HEAD_NAMES = ["head.dense.weight", "head.norm.weight", "classifier.weight", "classifier.bias"]
# tensors of other exports of the same encoder that play no part here: the masked-LM prediction head and decoder (their
# ``head.*`` is the prediction head, not a classifier's), and a classifier's head under an embedder's config
_IGNORED = {"decoder.weight", "decoder.bias", "lm_head.weight", "lm_head.bias"}


def state_names(cfg: ModernBertConfig) -> List[str]:
    """The checkpoint tensors a ModernBERT of ``cfg`` carries (after the ``model.`` prefix of the ``*For...`` exports is
    stripped), in the order the weights are built from them.  Layer 0 has no ``attn_norm`` (transformers: Identity)."""
    names = ["embeddings.tok_embeddings.weight", "embeddings.norm.weight"]
    for i in range(cfg.layers):
        p = f"layers.{i}."
        names += ([p + "attn_norm.weight"] if i else []) + [p + "attn.Wqkv.weight", p + "attn.Wo.weight", p + "mlp_norm.weight",
                                                            p + "mlp.Wi.weight", p + "mlp.Wo.weight"]
    return names + ["final_norm.weight"] + (_HEAD_NAMES if cfg.num_labels else [])


def check_config(cfg: ModernBertConfig) -> None:
    """The shapes the ModernBERT kernels take (tt_modernbert_forward refuses the others before a launch; say so here first)."""
    H, nh = cfg.hidden, cfg.heads
    if H % 128 or H > 1024:
        raise NotImplementedError(f"modernbert: hidden_size={H} (a multiple of 128 up to 1024, the scan's limit)")
    if nh <= 0 or H != 64 * nh:
        raise NotImplementedError(f"modernbert: hidden_size={H} with num_attention_heads={nh}: head_dim must be 64")
    if cfg.ffn <= 0 or cfg.ffn % 64:
        raise NotImplementedError(f"modernbert: intermediate_size={cfg.ffn} (a multiple of 64)")
    if len(cfg.layer_types) != cfg.layers or set(cfg.layer_types) - {"full_attention", "sliding_attention"}:
        raise ValueError(f"modernbert: layer_types={cfg.layer_types!r} does not name full_attention / sliding_attention for "
                         f"each of the {cfg.layers} layers")
    if cfg.local_attention < 0 or cfg.global_rope_theta <= 0 or cfg.local_rope_theta <= 0:
        raise ValueError(f"modernbert: local_attention={cfg.local_attention} rope bases {cfg.global_rope_theta} / {cfg.local_rope_theta}")
    if cfg.classifier_pooling not in ("cls", "mean"):
        raise NotImplementedError(f"modernbert: classifier_pooling={cfg.classifier_pooling!r} (supported: 'cls', 'mean')")


def check_state(cfg: ModernBertConfig, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``state`` without its ``model.`` prefix, after checking that it holds every tensor of ``state_names(cfg)`` and nothing the
    forward would not read: projection or norm biases, a layer-0 ``attn_norm`` ... mean another variant of the architecture and
    are refused, not ignored.  The masked-LM decoder, and the head tensors under an embedder's config, play no part."""
    sd = _strip_prefix(state)
    names = state_names(cfg)
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"checkpoint is not a ModernBERT of {cfg}: missing {missing[:4]}")
    extra = sorted(set(sd) - set(names) - _IGNORED - (set() if cfg.num_labels else set(_HEAD_NAMES)))
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the ModernBERT path does not compute: {extra[:4]}")
    return sd


class ModernBertWeights(_FamilyWeights):
    """Device-resident ModernBERT weights for ``tt_modernbert_forward`` (bf16) or ``tt_modernbert_forward_f16`` (fp16): the
    projections and the embedding table in the element type, the norm weights in fp32.  A ``*ForSequenceClassification``
    checkpoint (``cfg.num_labels``) brings the head, kept in fp32: ``head.dense`` transposed to [in][out] (the head kernel's lanes
    read it row by row), ``head.norm``, ``classifier.weight`` [H] and ``classifier.bias`` [1]."""

    _paths, _path_name = (MODERNBERT_BF16_PATH, MODERNBERT_FP16_PATH), "the ModernBERT path"

    def __init__(self, cfg: ModernBertConfig, state: Dict[str, torch.Tensor], device: torch.device,
                 dtype: torch.dtype = torch.bfloat16):
        self._begin(cfg, device, dtype)
        check_config(cfg)
        if cfg.num_labels not in (0, 1):
            raise NotImplementedError("modernbert: num_labels > 1: only single-label (sigmoid) cross-encoder heads are supported")
        sd = check_state(cfg, state)
        mat, vec = self._loaders(sd)
        H, F = cfg.hidden, cfg.ffn
        emb = mat(["embeddings.tok_embeddings.weight"], (cfg.vocab_size, H))
        self._layers = (_MbLayerW * max(cfg.layers, 1))()
        for i in range(cfg.layers):
            p, L = f"layers.{i}.", self._layers[i]
            L.qkv_w = mat([p + "attn.Wqkv.weight"], (3 * H, H))
            L.o_w = mat([p + "attn.Wo.weight"], (H, H))
            L.wi_w = mat([p + "mlp.Wi.weight"], (2 * F, H))
            L.wo_w = mat([p + "mlp.Wo.weight"], (H, F))
            L.attn_norm = vec([p + "attn_norm.weight"], H) if i else None
            L.mlp_norm = vec([p + "mlp_norm.weight"], H)
            L.sliding = 1 if cfg.layer_types[i] == "sliding_attention" else 0
        self.struct = _MbW(hidden=H, layers=cfg.layers, heads=cfg.heads, ffn=F, vocab=cfg.vocab_size,
                           local_attention=cfg.local_attention, norm_eps=cfg.ln_eps, global_rope_theta=cfg.global_rope_theta,
                           local_rope_theta=cfg.local_rope_theta, embed=emb, emb_norm=vec(["embeddings.norm.weight"], H),
                           layer=ctypes.cast(self._layers, POINTER(_MbLayerW)), final_norm=vec(["final_norm.weight"], H))
        if cfg.num_labels:
            dense, cls = sd["head.dense.weight"], sd["classifier.weight"]
            if tuple(dense.shape) != (H, H) or tuple(cls.shape) != (1, H) or tuple(sd["classifier.bias"].shape) != (1,):
                raise ValueError(f"head.dense {tuple(dense.shape)} / classifier {tuple(cls.shape)} do not match {cfg} (one label)")
            f32 = dict(device=device, dtype=torch.float32)
            self.struct.head_dense_wt = self._kept(dense.to(**f32).t().contiguous()).data_ptr()
            self.struct.head_norm = vec(["head.norm.weight"], H)
            self.struct.cls_w = self._kept(cls.reshape(H).to(**f32).contiguous()).data_ptr()
            self.struct.cls_b = vec(["classifier.bias"], 1)


def synthetic_state(cfg: ModernBertConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random ModernBERT weights of ``cfg`` (fp32, CPU) with trained-model-like scales: N(0, 0.02) projections and
    embeddings, norm weights around 1 (benchmarks and parity tests)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std=0.02):
        return torch.randn(*shape, generator=g) * std

    H, F = cfg.hidden, cfg.ffn
    sd = {"embeddings.tok_embeddings.weight": rnd(cfg.vocab_size, H), "embeddings.norm.weight": 1 + rnd(H, std=0.1),
          "final_norm.weight": 1 + rnd(H, std=0.1)}
    for i in range(cfg.layers):
        p = f"layers.{i}."
        if i:
            sd[p + "attn_norm.weight"] = 1 + rnd(H, std=0.1)
        sd[p + "attn.Wqkv.weight"] = rnd(3 * H, H)
        sd[p + "attn.Wo.weight"] = rnd(H, H)
        sd[p + "mlp_norm.weight"] = 1 + rnd(H, std=0.1)
        sd[p + "mlp.Wi.weight"] = rnd(2 * F, H)
        sd[p + "mlp.Wo.weight"] = rnd(H, F)
    if cfg.num_labels:
        sd["head.dense.weight"] = rnd(H, H)
        sd["head.norm.weight"] = 1 + rnd(H, std=0.1)
        sd["classifier.weight"] = rnd(cfg.num_labels, H, std=0.15)
        sd["classifier.bias"] = rnd(cfg.num_labels)
    return sd


def default_layer_types(layers: int, every: int) -> Tuple[str, ...]:
    """What transformers derives when config.json names no ``layer_types`` (older exports): global every ``every``-th layer."""
    return tuple("full_attention" if i % every == 0 else "sliding_attention" for i in range(layers))


# the published geometries (answerdotai/ModernBERT-base / -large config.json): what the base- and large-shaped tests and
# measurements build with seeded weights
MODERNBERT_BASE = ModernBertConfig(vocab_size=50368, hidden=768, layers=22, heads=12, ffn=1152, max_pos=8192, type_vocab=1,
                                   pad_id=50283, ln_eps=1e-5, layer_types=default_layer_types(22, 3), local_attention=128)
MODERNBERT_LARGE = ModernBertConfig(vocab_size=50368, hidden=1024, layers=28, heads=16, ffn=2624, max_pos=8192, type_vocab=1,
                                    pad_id=50283, ln_eps=1e-5, layer_types=default_layer_types(28, 3), local_attention=128)
