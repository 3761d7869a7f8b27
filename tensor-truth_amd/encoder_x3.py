"""Reference precision at matrix-core speed: host side of ``tt_encoder_forward_x3`` (csrc/x3_path.hip, "bf16x3").

The reference builds its embedder and reranker without a dtype (``services/model_manager.py:218-229,333-337``;
``app_utils/config_schema.py:66-76``: ``torch_dtype: None``), i.e. in fp32, and north_star's score tolerance (1e-3
relative) is an fp32 tolerance.  The fp32-MFMA path (``encoder_f32.py``) meets it at 1/16 of the bf16 matrix rate; this
one meets it at 1/3: every matrix product runs on the bf16 matrix cores with both operands split into two bf16 planes
(``x = hi + lo``; ``a.b ~= a_hi.b_hi + a_hi.b_lo + a_lo.b_hi``, fp32 accumulate), everything else (residual stream,
LayerNorm, softmax, exact-erf GELU, classification head) stays fp32.  Selected by ``precision.resolve()`` -- the process
setting ``TT_PRECISION=reference``, ``ModelManager``'s ``precision`` config key, or ``model_kwargs={"torch_dtype":
"float32"}`` -- whenever the model shape fits (``supports``: hidden a multiple of 128 with 64- or 32-wide heads); other
shapes fall back to ``encoder_f32``.  The planes are bf16 ("bf16x3", 16 significand bits per operand) or fp16 ("f16x3", the
default implementation: 22 bits down to fp16's subnormal grid, ``|x - hi - lo| <= max(2^-22 |x|, 2^-25)`` inside +-65504).
``encoder.Encoder`` runs it (``EncoderX3`` is that class) with the 16-bit path's token packing and surface.
"""
from __future__ import annotations

import dataclasses
from typing import Dict

import torch

from .encoder import Encoder, EncoderConfig, EncoderPath, _CheckpointWeights, _PlainLayerW, _weights_struct

_EncWX = _weights_struct("_EncWX", _PlainLayerW)

BF16X3_PATH = EncoderPath(forward="tt_encoder_forward_x3", workspace="tt_encoder_x3_workspace_bytes",
                          cls_forward="tt_encoder_forward_x3_cls", cls_workspace="tt_encoder_x3_cls_workspace_bytes",
                          pool="tt_embed_pool_f32", pool_mean="tt_embed_pool_mean_f32", head="tt_rerank_head_x3",
                          scratch="encx3", head_scratch="headx3", hidden=torch.float32, row_tile=256, skinny=True,
                          no_fp8="fp8 calibration does not apply to the reference-precision path")
# fp16 planes: the same path on the library's *_f16 entry points
F16X3_PATH = dataclasses.replace(BF16X3_PATH, forward="tt_encoder_forward_x3_f16", workspace="tt_encoder_x3_workspace_bytes_f16",
                                 cls_forward="tt_encoder_forward_x3_cls_f16", cls_workspace="tt_encoder_x3_cls_workspace_bytes_f16",
                                 head="tt_rerank_head_x3_f16")

EncoderX3 = Encoder


def supports(cfg: EncoderConfig) -> bool:
    """Shapes the split-plane kernels take (csrc/x3_path.hip check_weights_x3).  Round 6: hidden a multiple of 128 with 64- or
    32-wide heads -- the 384-wide BERT models the reference names (``BAAI/bge-small-en-v1.5``, BASELINE config 1;
    ``cross-encoder/ms-marco-MiniLM-L-6-v2``, app_utils/config_schema.py:83-87) no longer fall to the fp32 MFMA."""
    return (cfg.hidden % 128 == 0 and cfg.hidden <= 1024 and cfg.hidden in (cfg.heads * 64, cfg.heads * 32) and cfg.ffn % 64 == 0
            and cfg.layers > 0)


def split_planes(w: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """fp32 [out][in] -> planes [out][2 in] of ``dtype``: hi = dtype(w), lo = dtype(w - hi) side by side (``GemmParams.x3``).
    bfloat16: "bf16x3" (16 significand bits per operand); float16: "f16x3" (22, down to fp16's subnormal grid:
    ``|w - hi - lo| <= max(2^-22 |w|, 2^-25)`` inside +-65504 -- lo is an fp16 subnormal for every ``|w| < 2^-3``; values beyond
    +-65504 saturate in hi and lo takes what is left, up to +-131008).  The device split of the activations (``tt_split_planes*``,
    the GEMM and LayerNorm epilogues) gives the same bits: tests/test_gemm_x3_edges_gpu.py."""
    w = w.to(torch.float32)
    if dtype == torch.float16:
        hi = w.clamp(-65504.0, 65504.0).to(torch.float16)
        lo = (w - hi.to(torch.float32)).clamp(-65504.0, 65504.0).to(torch.float16)
    else:
        hi = w.to(torch.bfloat16)
        lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=1).contiguous()


class EncoderWeightsX3(_CheckpointWeights):
    """Device-resident split-plane weights (HF checkpoint names, see ``encoder._CheckpointWeights``): matrices as two bf16
    or fp16 planes (2 x 1.13 GB for the 1024-wide models), tables / biases / LayerNorm / head in fp32."""

    _Struct = _EncWX

    def __init__(self, cfg: EncoderConfig, state: Dict[str, torch.Tensor], device: torch.device, round_weights: bool = False,
                 dtype: torch.dtype = torch.bfloat16):
        """``dtype``: the planes' element type -- bfloat16 ("bf16x3", round 3) or float16 ("f16x3", round 4: the default
        implementation of the reference precision, on the library's ``*_f16`` entry points).
        ``round_weights`` (diagnostic, tools/probes/bf16_error_budget.py): every tensor the bf16 path keeps in bf16 -- the
        matrices and the embedding tables -- is rounded to bf16 first, i.e. the weights' share of the bf16 mode's error."""
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("split planes are bfloat16 or float16")
        self.dtype = dtype
        self.gemm_dtype = "f16x3" if dtype == torch.float16 else "bf16x3"
        self.path = F16X3_PATH if dtype == torch.float16 else BF16X3_PATH
        if not supports(cfg):
            raise ValueError(f"the split-plane path takes hidden % 128 == 0 with 64- or 32-wide heads and ffn % 64 == 0, not {cfg}")
        self._round = round_weights
        self._load(cfg, state, device)

    def _table(self, names, x):
        return super()._table(names, x.to(torch.bfloat16) if self._round else x)

    def _matrix(self, L, field, names, x):
        if self._round:
            x = x.to(torch.bfloat16)
        setattr(L, field, self._kept(names, split_planes(x.to(device=self.device), self.dtype)).data_ptr())

    def set_gemm_dtype(self, dtype: str) -> None:
        if dtype not in ("bf16x3", "f16x3", "reference", "float32", "fp32"):
            raise ValueError(f"split-bf16 weights run in reference precision only (asked for {dtype!r})")
