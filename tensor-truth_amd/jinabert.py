"""JinaBERT embedders on the HIP path: the remote-code architecture (``jinaai/jina-bert-implementation``) behind
``jinaai/jina-embeddings-v2-small-en`` and ``-base-en``, the 8192-token English embedders; weights in the layout of
``tt_jinabert_weights`` (include/tt_hip.h), driven by the one host-side ``encoder.Encoder`` through the ``JINABERT_*_PATH`` records.

The reference loads embedders with ``trust_remote_code: True`` by default (``app_utils/config_schema.py:61,74``), so these
checkpoints load there.  Their ``config.json`` says ``"model_type": "bert"``; what tells them from BERT is
``"position_embedding_type": "alibi"`` (``weights._config_from_hf`` dispatches on it, arch ``"jina_bert"``).  The layer is the
post-LN BERT block with two differences: no position table -- every head h adds the ALiBi bias ``-slope_h |query - key|`` to its
scores after the 1/sqrt(64) scaling, symmetric, over the sequence's own tokens -- and a GEGLU feed-forward
(``wo(GELU_erf(g[:, :F]) * g[:, F:])``, ``g = gated_layers(h)`` without a bias).  Every token of an embedder call is of type 0,
whose ``token_type_embeddings`` row is still added.  Precision: bf16 or fp16; the reference-precision default of the XLM-R / BERT
family has no implementation here (``precision.build_encoder``).

[UPSTREAM-K] The modelling file is not part of the installed transformers, so the tensor names, the config keys and which half of
``gated_layers`` is activated are stated from knowledge of the upstream module, not checked against it.  The arithmetic is pinned
piece by piece to classes that are installed (tests/golden/make_jinabert_golden.py).  The loader is therefore strict: a tensor it
does not know is refused by name, so a wrong assumption about upstream surfaces as a refusal, not as wrong vectors.
"""
from __future__ import annotations

import ctypes
import logging
import math
import re
from ctypes import POINTER, Structure, c_float, c_int32, c_void_p
from dataclasses import dataclass
from typing import Dict, List

import torch

from .encoder import JINABERT_BF16_PATH, JINABERT_FP16_PATH, EncoderConfig, _FamilyWeights

logger = logging.getLogger(__name__)

ARCH = "jina_bert"


@dataclass(frozen=True)
class JinaBertConfig(EncoderConfig):
    """The ``EncoderConfig`` fields (``pad_id`` = the filler ``pack_tokens`` writes into rows of no sequence; ``max_pos`` = the
    longest sequence, there is no position table to run out of)."""

    arch: str = ARCH
    vocab_size: int = 30528
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    ffn: int = 3072
    max_pos: int = 8192
    type_vocab: int = 2
    pad_id: int = 0
    ln_eps: float = 1e-12


def alibi_slopes(heads: int) -> List[float]:
    """The per-head slopes of the original ALiBi rule, in double: for a power of two n the geometric series 2^(-8 i / n),
    i = 1 .. n; otherwise the series of the power of two below, then every other term of the next power of two's series."""
    if heads <= 0:
        raise ValueError(f"alibi_slopes: heads={heads}")

    def pow2(n: int) -> List[float]:
        return [2.0 ** (-8.0 * (i + 1) / n) for i in range(n)]

    below = 1 << (heads.bit_length() - 1)
    if below == heads:
        return pow2(heads)
    return pow2(below) + pow2(2 * below)[0::2][:heads - below]


def config_from_hf(d: dict) -> JinaBertConfig:
    """``config.json`` of a JinaBERT checkpoint (``model_type`` "bert", ``position_embedding_type`` "alibi") -> ``JinaBertConfig``.
    Variants the kernels do not compute are refused by field name."""
    if d.get("model_type") != "bert" or d.get("position_embedding_type") != "alibi":
        raise ValueError(f"model_type={d.get('model_type')!r} position_embedding_type={d.get('position_embedding_type')!r} is not a "
                         "JinaBERT config (model_type 'bert', position_embedding_type 'alibi')")
    archs = " ".join(d.get("architectures") or [])
    if "ForSequenceClassification" in archs or "ForTokenClassification" in archs or "ForQuestionAnswering" in archs:
        raise ValueError(f"architectures={d.get('architectures')!r}: {ARCH} checkpoints are served as embedders only "
                         "(HipHuggingFaceEmbedding); a *ForSequenceClassification head of this type is not supported")
    hidden, heads = int(d["hidden_size"]), int(d["num_attention_heads"])
    head_dim = hidden // heads if heads > 0 and hidden % heads == 0 else 0
    ff = str(d.get("feed_forward_type", "original"))
    act = str(d.get("hidden_act", "gelu"))
    bad = [f"{n}={v!r}" for n, v, ok in (("feed_forward_type", ff, ff == "geglu"), ("hidden_act", act, act == "gelu"),
                                         ("head_dim", head_dim, head_dim == 64),
                                         ("hidden_size", hidden, hidden <= 1024 and hidden % 128 == 0)) if not ok]
    if bad:
        raise NotImplementedError(f"{ARCH} checkpoint with {', '.join(bad)}: the path computes feed_forward_type 'geglu' with "
                                  "hidden_act 'gelu' (exact erf), head_dim 64 (hidden_size / num_attention_heads) and hidden_size a "
                                  "multiple of 128 up to 1024 only")
    vocab = int(d["vocab_size"])
    pad = d.get("pad_token_id", 0)
    return JinaBertConfig(vocab_size=vocab, hidden=hidden, layers=int(d["num_hidden_layers"]), heads=heads,
                          ffn=int(d["intermediate_size"]), max_pos=int(d.get("max_position_embeddings", 8192)),
                          type_vocab=int(d.get("type_vocab_size", 2)),
                          pad_id=int(pad) if pad is not None and 0 <= int(pad) < vocab else 0,
                          ln_eps=float(d.get("layer_norm_eps", 1e-12)), num_labels=0)


class _JbLayerW(Structure):
    """tt_jinabert_layer_weights."""
    _fields_ = [(n, c_void_p) for n in ("qkv_w", "qkv_b", "o_w", "o_b", "ln1_g", "ln1_b", "gate_w", "down_w", "down_b", "ln2_g",
                                        "ln2_b")]


class _JbW(Structure):
    """tt_jinabert_weights."""
    _fields_ = ([(n, c_int32) for n in ("hidden", "layers", "heads", "ffn", "vocab", "type_vocab")] + [("ln_eps", c_float)]
                + [(n, c_void_p) for n in ("word_emb", "type_emb", "emb_ln_g", "emb_ln_b", "alibi_slope_log2")]
                + [("layer", POINTER(_JbLayerW))])


# ---- names [UPSTREAM-K] -----------------------------------------------------------------------------------------------------------
# tensors an embedder does not read: BertModel's pooler (sentence-transformers pools the hidden states itself) and the masked-LM head
_NOT_READ = re.compile(r"^(pooler\.|cls\.)")


def state_names(cfg: JinaBertConfig) -> List[str]:
    """The checkpoint tensors a model of ``cfg`` carries and the forward reads."""
    names = ["embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight",
             "embeddings.LayerNorm.bias"]
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        for m in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                  "attention.output.LayerNorm", "mlp.wo", "mlp.layernorm"):
            names += [p + m + ".weight", p + m + ".bias"]
        names.append(p + "mlp.gated_layers.weight")
    return names


def check_config(cfg: JinaBertConfig) -> None:
    """The shapes the kernels take (tt_jinabert_forward refuses the others before a launch; say so here first)."""
    H, nh = cfg.hidden, cfg.heads
    if cfg.arch != ARCH:
        raise ValueError(f"jinabert: arch={cfg.arch!r} is not {ARCH!r}")
    if H % 128 or H > 1024:
        raise NotImplementedError(f"{ARCH}: hidden_size={H} (a multiple of 128 up to 1024, the scan's limit)")
    if nh <= 0 or H != 64 * nh:
        raise NotImplementedError(f"{ARCH}: hidden_size={H} with num_attention_heads={nh}: head_dim must be 64")
    if cfg.ffn <= 0 or cfg.ffn % 128:
        raise NotImplementedError(f"{ARCH}: intermediate_size={cfg.ffn} (a multiple of 128)")
    if cfg.num_labels:
        raise NotImplementedError(f"{ARCH}: classification heads are not supported (embedders only)")
    if cfg.type_vocab < 1:
        raise ValueError(f"{ARCH}: type_vocab_size={cfg.type_vocab}")


def check_state(cfg: JinaBertConfig, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``state`` with one optional ``bert.`` prefix stripped, after checking that it holds every tensor of ``state_names(cfg)`` and
    nothing else the forward would have to compute: ``attention.self.layer_norm_q`` / ``layer_norm_k`` (the qk-post-norm variant
    behind jina-embeddings-v2-base-de / -es / -zh / -code), a position table, a bias on ``gated_layers`` ... are refused by name,
    not ignored.  ``pooler.*`` and ``cls.*`` play no part in an embedder and are dropped, by name in the log."""
    sd = {(k[len("bert."):] if k.startswith("bert.") else k): v for k, v in state.items()}
    names = state_names(cfg)
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"checkpoint is not a {ARCH} of {cfg}: missing {missing[:4]}")
    rest = sorted(set(sd) - set(names))
    extra = [k for k in rest if not _NOT_READ.search(k)]
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the {ARCH} path does not compute: {extra[:4]}")
    if rest:
        logger.info("%s: tensors not read by an embedder: %s", ARCH, rest)
    return {n: sd[n] for n in names}


class JinaBertWeights(_FamilyWeights):
    """Device-resident weights for ``tt_jinabert_forward`` (bf16) or ``tt_jinabert_forward_f16`` (fp16): the projections (query, key,
    value rows concatenated to [3H][H]; ``gated_layers`` as stored, [2F][H]: the rows GELU is applied to, then the rows that
    multiply them -- the order ``gated_act_kernel`` reads) and the embedding tables in the element type; biases, LayerNorm
    parameters and the ALiBi slopes (times log2(e), from double, one rounding) in fp32."""

    _paths, _path_name = (JINABERT_BF16_PATH, JINABERT_FP16_PATH), "the path"

    def __init__(self, cfg: JinaBertConfig, state: Dict[str, torch.Tensor], device: torch.device, dtype: torch.dtype = torch.bfloat16):
        self._begin(cfg, device, dtype)
        check_config(cfg)
        sd = check_state(cfg, state)
        mat, vec = self._loaders(sd)
        H, F = cfg.hidden, cfg.ffn
        self._layers = (_JbLayerW * max(cfg.layers, 1))()
        for i in range(cfg.layers):
            p, L = f"encoder.layer.{i}.", self._layers[i]
            qkv = [p + f"attention.self.{n}." for n in ("query", "key", "value")]
            L.qkv_w, L.qkv_b = mat([m + "weight" for m in qkv], (3 * H, H)), vec([m + "bias" for m in qkv], 3 * H)
            L.o_w, L.o_b = mat([p + "attention.output.dense.weight"], (H, H)), vec([p + "attention.output.dense.bias"], H)
            L.ln1_g, L.ln1_b = vec([p + "attention.output.LayerNorm.weight"], H), vec([p + "attention.output.LayerNorm.bias"], H)
            L.gate_w = mat([p + "mlp.gated_layers.weight"], (2 * F, H))
            L.down_w, L.down_b = mat([p + "mlp.wo.weight"], (H, F)), vec([p + "mlp.wo.bias"], H)
            L.ln2_g, L.ln2_b = vec([p + "mlp.layernorm.weight"], H), vec([p + "mlp.layernorm.bias"], H)
        log2e = math.log2(math.e)
        slopes = torch.tensor([s * log2e for s in alibi_slopes(cfg.heads)], dtype=torch.float64).to(torch.float32)
        self.struct = _JbW(hidden=H, layers=cfg.layers, heads=cfg.heads, ffn=F, vocab=cfg.vocab_size, type_vocab=cfg.type_vocab,
                           ln_eps=cfg.ln_eps, word_emb=mat(["embeddings.word_embeddings.weight"], (cfg.vocab_size, H)),
                           type_emb=mat(["embeddings.token_type_embeddings.weight"], (cfg.type_vocab, H)),
                           emb_ln_g=vec(["embeddings.LayerNorm.weight"], H), emb_ln_b=vec(["embeddings.LayerNorm.bias"], H),
                           alibi_slope_log2=self._kept(slopes.to(device).contiguous()).data_ptr(),
                           layer=ctypes.cast(self._layers, POINTER(_JbLayerW)))


def synthetic_state(cfg: JinaBertConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random weights of ``cfg`` (fp32, CPU) under the checkpoint names, with trained-model-like scales: N(0, 0.02)
    projections and embeddings, LayerNorm weights around 1 (benchmarks and tests)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std=0.02):
        return torch.randn(*shape, generator=g) * std

    H, F = cfg.hidden, cfg.ffn
    sd = {"embeddings.word_embeddings.weight": rnd(cfg.vocab_size, H), "embeddings.token_type_embeddings.weight": rnd(cfg.type_vocab, H),
          "embeddings.LayerNorm.weight": 1 + rnd(H, std=0.1), "embeddings.LayerNorm.bias": rnd(H, std=0.05)}
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        for m in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
            sd[p + m + ".weight"], sd[p + m + ".bias"] = rnd(H, H), rnd(H)
        sd[p + "mlp.gated_layers.weight"] = rnd(2 * F, H)
        sd[p + "mlp.wo.weight"], sd[p + "mlp.wo.bias"] = rnd(H, F), rnd(H)
        for m in ("attention.output.LayerNorm", "mlp.layernorm"):
            sd[p + m + ".weight"], sd[p + m + ".bias"] = 1 + rnd(H, std=0.1), rnd(H, std=0.05)
    return sd


# the published geometries (jina-embeddings-v2-small-en / -base-en; the bert-base-uncased vocabulary padded to 30528)
JINA_V2_SMALL = JinaBertConfig(hidden=512, layers=4, heads=8, ffn=2048)
JINA_V2_BASE = JinaBertConfig(hidden=768, layers=12, heads=12, ffn=3072)
