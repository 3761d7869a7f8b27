"""Which arithmetic a HIP embedder / reranker runs in, and who decides.

The reference never passes a dtype to its reranker (``SentenceTransformerRerank(model=, top_n=, device=)``,
``src/tensortruth/services/model_manager.py:333-337``) and passes one to its embedder only when the per-model config
holds ``torch_dtype`` (``services/model_manager.py:218-229``; ``app_utils/config_schema.py:66-76``: default None), so the
reference's own precision is fp32 -- and so is this package's DEFAULT: an unchanged reference call (no dtype anywhere)
resolves to mode "reference", whose scores are within north_star's 1e-3 relative of the reference's CPU path.
BASELINE.json's configurations name bf16 (and fp8 for config 5): those are the modes a caller NAMES (``torch_dtype:
"bfloat16"`` in the per-model config, as the reference's own config schema allows; ``TT_PRECISION=bf16``;
``ModelManager.set_precision("bf16")``), and the ones ``bench.py`` names for its headline.

    mode "reference"  fp32 semantics: scores within north_star's 1e-3 relative of the CPU path.  Implementations
                      (``TT_REFERENCE_IMPL``); "f16x3" / "bf16x3" for hidden a multiple of 128 with 64- or 32-wide heads (round 6:
                      bge-small-en-v1.5 and ms-marco-MiniLM-L-6-v2 included), "f16c" for multiples of 256 with 64-wide heads,
                      anything else "fp32":
                        "f16x3"  (default, round 4) every operand as two fp16 planes, three fp16 MFMA products per product
                                 (``encoder_x3`` on fp16 planes): a third of the bf16 matrix rate, 22 significand bits -- holds
                                 1e-3 with a margin even on the stress fixture (tests/stress_weights.py)
                        "f16c"   fp16 main products + block-scaled e4m3 correction terms (``encoder_f16c``): HALF the bf16
                                 rate, 1e-4 on the standard fixture, but 7e-3 relative on the stress fixture's smallest scores
                                 (ranking intact): the fast variant, for callers who accept that
                        "bf16x3" round 3's two bf16 planes (16 bits): 2e-5 / 1.0e-3 (standard / stress)
                        "fp32"   the fp32 MFMA (``encoder_f32``, 1/16 of the bf16 rate)
    mode "bf16"       bf16 weights / activations, fp32 accumulate (BASELINE configs 2-4; the reference's ``torch_dtype: bfloat16``)
    mode "fp16"       IEEE fp16 weights / activations, fp32 accumulate: the bf16 mode's rate (v_mfma_*_f16) with three more
                      mantissa bits at every rounding point -- scores about ten times closer to the reference than bf16;
                      what the reference's ``torch_dtype: "float16"`` asks for, and FlagEmbedding's own default for the BGE
                      models.  Values beyond +-65504 saturate at the GEMM / LayerNorm outputs.
    mode "fp8"        the layer projections in OCP e4m3 (BASELINE config 5's "fp8 MFMA reranker")

Resolution order (first that says something): ``model_kwargs["precision"]``; ``model_kwargs["torch_dtype"]`` (float32 ->
reference; float16 -> fp16; bfloat16 -> bf16) and ``model_kwargs["gemm_dtype"]``; ``ModelManager.precision`` (a config key the
application sets once; ModelManager puts it into the model_kwargs it builds); the process environment ``TT_PRECISION``;
"reference" (round 4; rounds 1-3 defaulted to bf16, which put the unchanged calls 10x outside the tolerance).  The active
mode is logged when a model is loaded.
"""
from __future__ import annotations

import functools
import logging
import os
from typing import Any, Callable, Dict, Optional, Tuple

logger = logging.getLogger(__name__)

MODES = ("bf16", "fp16", "fp8", "reference")
# what a call that names no dtype gets: the reference's own arithmetic (services/model_manager.py:333-337 passes none;
# app_utils/config_schema.py:66-76 defaults torch_dtype to None) -- fp32 semantics
DEFAULT_MODE = "reference"
_ALIASES = {"bf16": "bf16", "bfloat16": "bf16", "fp16": "fp16", "float16": "fp16", "half": "fp16", "fp8": "fp8", "e4m3": "fp8",
            "reference": "reference", "fp32": "reference", "float32": "reference", "float": "reference", "bf16x3": "reference"}


def canonical(value) -> str:
    v = str(value).replace("torch.", "").strip().lower()
    if v not in _ALIASES:
        raise ValueError(f"precision {value!r}: expected one of {MODES}")
    return _ALIASES[v]


def resolve(model_kwargs: Optional[Dict[str, Any]] = None, environ=None) -> str:
    mk = model_kwargs or {}
    if mk.get("precision") is not None:
        return canonical(mk["precision"])
    td = mk.get("torch_dtype")
    if td is not None:
        t = str(td).replace("torch.", "")
        if t in ("float32", "fp32", "float"):
            return "reference"
        if t in ("float16", "fp16", "half") and mk.get("gemm_dtype") is None:
            return "fp16"
        if mk.get("gemm_dtype") is None:
            return "bf16"          # bfloat16, and anything else the HIP path maps to bf16 (logged by the callers)
    if mk.get("gemm_dtype") is not None:
        return canonical(mk["gemm_dtype"])
    env = (os.environ if environ is None else environ).get("TT_PRECISION")
    if env:
        return canonical(env)
    return DEFAULT_MODE


def reference_impl(cfg, environ=None) -> str:
    """"f16x3" (two fp16 planes per operand: three matrix-time units) where the model shape fits, else "fp32" (fp32 MFMA);
    ``TT_REFERENCE_IMPL`` = "f16c" / "bf16x3" / "fp32" selects another implementation."""
    from . import encoder_f16c, encoder_x3

    forced = (os.environ if environ is None else environ).get("TT_REFERENCE_IMPL", "").strip().lower()
    if forced in ("fp32", "float32", "f32"):
        return "fp32"
    if forced in ("bf16x3", "x3", "split-bf16"):
        return "bf16x3" if encoder_x3.supports(cfg) else "fp32"
    if forced in ("f16c", "fast"):
        return "f16c" if encoder_f16c.supports(cfg) else "fp32"
    return "f16x3" if encoder_x3.supports(cfg) else "fp32"


def _implementations() -> Dict[str, Tuple[Callable, str]]:
    """Mode (or, for mode "reference", implementation) -> (weights factory ``f(cfg, state, device)``, description)."""
    import torch

    from .encoder import EncoderWeights
    from .encoder_f16c import EncoderWeightsF16C
    from .encoder_f32 import EncoderWeightsF32
    from .encoder_x3 import EncoderWeightsX3

    return {
        "f16c": (EncoderWeightsF16C, "reference (fp32 semantics as fp16 products + block-scaled e4m3 correction terms on the "
                                     "matrix cores, fp32 residual stream)"),
        "f16x3": (functools.partial(EncoderWeightsX3, dtype=torch.float16),
                  "reference (fp32 semantics as split-fp16 on the fp16 matrix cores, fp32 residual stream)"),
        "bf16x3": (EncoderWeightsX3, "reference (fp32 semantics as split-bf16 on the bf16 matrix cores, fp32 residual stream)"),
        "fp32": (EncoderWeightsF32, "reference (fp32 weights, activations and MFMA)"),
        "fp16": (functools.partial(EncoderWeights, dtype=torch.float16), "fp16 (fp32 accumulate)"),
        "bf16": (EncoderWeights, "bf16 (fp32 accumulate)"),
        "fp8": (EncoderWeights, "fp8 e4m3 layer projections, bf16 elsewhere"),
    }


def build_encoder(cfg, state, device, model_kwargs: Optional[Dict[str, Any]], what: str) -> Tuple[Any, Any, str]:
    """-> (weights, encoder, description) for the resolved precision; logs it."""
    from .encoder import Encoder

    mode = resolve(model_kwargs)
    if getattr(cfg, "arch", "") == "qwen3":
        return _build_decoder(cfg, state, device, mode, what)
    if getattr(cfg, "arch", "") == "modernbert":
        return _build_modernbert(cfg, state, device, mode, what)
    if getattr(cfg, "arch", "") == "gemma3_text":
        return _build_gemma(cfg, state, device, mode, what)
    if getattr(cfg, "arch", "") == "mpnet":
        return _build_mpnet(cfg, state, device, mode, what)
    if getattr(cfg, "arch", "") == "deberta-v2":
        return _build_deberta(cfg, state, device, mode, what)
    if getattr(cfg, "arch", "") in ("nomic_bert", "jina_embeddings_v3"):
        return _build_ropebert(cfg, state, device, mode, what)
    if getattr(cfg, "arch", "") == "jina_bert":
        return _build_jinabert(cfg, state, device, mode, what)
    if getattr(cfg, "arch", "") == "t5":
        return _build_t5(cfg, state, device, mode, what)
    impl = reference_impl(cfg) if mode == "reference" else mode
    make, desc = _implementations()[impl]
    w = make(cfg, state, device)
    if impl == "fp8":
        w.set_gemm_dtype("fp8")
    if impl == "fp32" and os.environ.get("TT_REFERENCE_IMPL", "").strip().lower() not in ("fp32", "float32", "f32"):
        # the rate cliff of the default mode: the split-plane kernels take hidden sizes that are multiples of 128
        # with 64- or 32-wide heads (bge-m3, the bge rerankers; round 6: bge-small 384 and MiniLM's 32-wide heads too); any
        # other shape runs on the fp32 MFMA -- ~1/16 of the bf16 matrix rate instead of 1/3
        logger.warning("%s: hidden=%d heads=%d has no split-plane kernel: the reference precision falls back to the fp32 MFMA "
                       "path (about 1/16 of the bf16 rate; name torch_dtype=bfloat16 / float16 or TT_PRECISION for the "
                       "16-bit modes)", what, getattr(cfg, "hidden", -1), getattr(cfg, "heads", -1))
    logger.info("%s: precision = %s", what, desc)
    return w, Encoder(w), desc


def _build_decoder(cfg, state, device, mode: str, what: str) -> Tuple[Any, Any, str]:
    """Decoder embedders (Qwen3-Embedding): bf16 -- what the published checkpoints declare -- or fp16.  The reference precision
    (fp32 semantics, what no torch_dtype means for the encoder family) has no decoder implementation: refused, never computed in
    another precision behind the caller's back."""
    import torch

    from .decoder import DecoderWeights
    from .encoder import Encoder

    if mode not in ("bf16", "fp16"):
        raise NotImplementedError(
            f"{what}: precision '{mode}' is not available for decoder embedders (Qwen3-Embedding); pass "
            f"model_kwargs={{'torch_dtype': 'bfloat16'}} or {{'torch_dtype': 'float16'}}")
    w = DecoderWeights(cfg, state, device, dtype=torch.float16 if mode == "fp16" else torch.bfloat16)
    desc = "fp16 (fp32 accumulate)" if mode == "fp16" else "bf16 (fp32 accumulate)"
    logger.info("%s: decoder embedder, precision = %s", what, desc)
    return w, Encoder(w), desc


def _build_modernbert(cfg, state, device, mode: str, what: str) -> Tuple[Any, Any, str]:
    """ModernBERT encoders: bf16 or fp16, resolved as for the decoder embedders.  The reference precision (fp32 semantics, what no
    torch_dtype means for the XLM-R / BERT family) has no ModernBERT implementation: refused, never computed in another precision
    behind the caller's back."""
    import torch

    from .encoder import Encoder
    from .modernbert import ModernBertWeights

    if mode not in ("bf16", "fp16"):
        raise NotImplementedError(
            f"{what}: precision '{mode}' is not available for ModernBERT encoders; pass "
            f"model_kwargs={{'torch_dtype': 'bfloat16'}} or {{'torch_dtype': 'float16'}}")
    w = ModernBertWeights(cfg, state, device, dtype=torch.float16 if mode == "fp16" else torch.bfloat16)
    desc = "fp16 (fp32 accumulate)" if mode == "fp16" else "bf16 (fp32 accumulate)"
    logger.info("%s: ModernBERT encoder, precision = %s", what, desc)
    return w, Encoder(w), desc


def _build_gemma(cfg, state, device, mode: str, what: str) -> Tuple[Any, Any, str]:
    """EmbeddingGemma embedders: bf16 only.  The model card rules float16 out (the activations overflow its range), and the
    reference precision (fp32 semantics, what no torch_dtype means for the XLM-R / BERT family) has no implementation here:
    refused, never computed in another precision behind the caller's back."""
    from .encoder import Encoder
    from .gemma import GemmaWeights

    if mode != "bf16":
        why = (" (the model card: float16 is not supported, the activations overflow its range)" if mode == "fp16" else "")
        raise NotImplementedError(
            f"{what}: precision '{mode}' is not available for EmbeddingGemma embedders{why}; pass "
            f"model_kwargs={{'torch_dtype': 'bfloat16'}}")
    w = GemmaWeights(cfg, state, device)
    desc = "bf16 (fp32 accumulate)"
    logger.info("%s: EmbeddingGemma embedder, precision = %s", what, desc)
    return w, Encoder(w), desc


def _build_mpnet(cfg, state, device, mode: str, what: str) -> Tuple[Any, Any, str]:
    """MPNet embedders: bf16 or fp16, resolved as for the ModernBERT encoders.  The reference precision (fp32 semantics, what no
    torch_dtype means for the XLM-R / BERT family) has no MPNet implementation: refused, never computed in another precision
    behind the caller's back."""
    import torch

    from .encoder import Encoder
    from .mpnet import MpnetWeights

    if mode not in ("bf16", "fp16"):
        raise NotImplementedError(
            f"{what}: precision '{mode}' is not available for MPNet encoders; pass "
            f"model_kwargs={{'torch_dtype': 'bfloat16'}} or {{'torch_dtype': 'float16'}}")
    w = MpnetWeights(cfg, state, device, dtype=torch.float16 if mode == "fp16" else torch.bfloat16)
    desc = "fp16 (fp32 accumulate)" if mode == "fp16" else "bf16 (fp32 accumulate)"
    logger.info("%s: MPNet encoder, precision = %s", what, desc)
    return w, Encoder(w), desc


def _build_deberta(cfg, state, device, mode: str, what: str) -> Tuple[Any, Any, str]:
    """DeBERTa-v2 / v3 cross-encoders: bf16 or fp16, resolved as for the MPNet encoders.  The reference precision (fp32 semantics,
    what no torch_dtype means for the XLM-R / BERT family) has no DeBERTa implementation: refused, never computed in another
    precision behind the caller's back."""
    import torch

    from .deberta import DebertaWeights
    from .encoder import Encoder

    if mode not in ("bf16", "fp16"):
        raise NotImplementedError(
            f"{what}: precision '{mode}' is not available for DeBERTa encoders; pass "
            f"model_kwargs={{'torch_dtype': 'bfloat16'}} or {{'torch_dtype': 'float16'}}")
    w = DebertaWeights(cfg, state, device, dtype=torch.float16 if mode == "fp16" else torch.bfloat16)
    desc = "fp16 (fp32 accumulate)" if mode == "fp16" else "bf16 (fp32 accumulate)"
    logger.info("%s: DeBERTa encoder, precision = %s", what, desc)
    return w, Encoder(w), desc


def _build_ropebert(cfg, state, device, mode: str, what: str) -> Tuple[Any, Any, str]:
    """NomicBERT / Jina-v3 embedders: bf16 or fp16, resolved as for the ModernBERT encoders.  The reference precision (fp32
    semantics, what no torch_dtype means for the XLM-R / BERT family) has no implementation for them: refused, never computed in
    another precision behind the caller's back."""
    import torch

    from .encoder import Encoder
    from .ropebert import RopeBertWeights

    if mode not in ("bf16", "fp16"):
        raise NotImplementedError(
            f"{what}: precision '{mode}' is not available for NomicBERT / Jina-v3 encoders; pass "
            f"model_kwargs={{'torch_dtype': 'bfloat16'}} or {{'torch_dtype': 'float16'}}")
    w = RopeBertWeights(cfg, state, device, dtype=torch.float16 if mode == "fp16" else torch.bfloat16)
    desc = "fp16 (fp32 accumulate)" if mode == "fp16" else "bf16 (fp32 accumulate)"
    logger.info("%s: %s encoder, precision = %s", what, cfg.arch, desc)
    return w, Encoder(w), desc


def _build_t5(cfg, state, device, mode: str, what: str) -> Tuple[Any, Any, str]:
    """T5 encoders: bf16 only.  The FFN activations of a T5 leave float16's range -- transformers' own float16 run clamps them,
    which is another model -- the fp8 projections exist for the XLM-R / BERT family only, and the reference precision (fp32
    semantics, what no torch_dtype means for that family) has no implementation here: refused, never computed in another
    precision behind the caller's back."""
    from .encoder import Encoder
    from .t5 import T5Weights

    if mode != "bf16":
        why = {"fp16": " (T5's feed-forward activations leave float16's range; transformers clamps them in float16, which is "
                       "another model)",
               "fp8": " (the fp8 projections exist for the XLM-R / BERT family only)",
               "reference": " (the fp32-semantics paths exist for the XLM-R / BERT family only)"}.get(mode, "")
        raise NotImplementedError(
            f"{what}: precision '{mode}' is not available for T5 encoders{why}; pass "
            f"model_kwargs={{'torch_dtype': 'bfloat16'}}")
    w = T5Weights(cfg, state, device)
    desc = "bf16 (fp32 accumulate)"
    logger.info("%s: T5 encoder, precision = %s", what, desc)
    return w, Encoder(w), desc


def _build_jinabert(cfg, state, device, mode: str, what: str) -> Tuple[Any, Any, str]:
    """JinaBERT embedders (jina-embeddings-v2): bf16 or fp16, resolved as for the ModernBERT encoders.  The reference precision
    (fp32 semantics, what no torch_dtype means for the XLM-R / BERT family) has no implementation for them: refused, never computed
    in another precision behind the caller's back."""
    import torch

    from .encoder import Encoder
    from .jinabert import JinaBertWeights

    if mode not in ("bf16", "fp16"):
        raise NotImplementedError(
            f"{what}: precision '{mode}' is not available for JinaBERT encoders; pass "
            f"model_kwargs={{'torch_dtype': 'bfloat16'}} or {{'torch_dtype': 'float16'}}")
    w = JinaBertWeights(cfg, state, device, dtype=torch.float16 if mode == "fp16" else torch.bfloat16)
    desc = "fp16 (fp32 accumulate)" if mode == "fp16" else "bf16 (fp32 accumulate)"
    logger.info("%s: JinaBERT encoder, precision = %s", what, desc)
    return w, Encoder(w), desc
