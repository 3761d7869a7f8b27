"""Reference precision on two matrix-time units: host side of ``tt_encoder_forward_f16c`` (csrc/f16c_path.hip, round 4).

The reference builds its embedder and reranker without a dtype (``services/model_manager.py:218-229,333-337``;
``app_utils/config_schema.py:66-76``: ``torch_dtype: None``), i.e. in fp32, and north_star's score tolerance (1e-3
relative) is an fp32 tolerance.  ``encoder_x3`` (split planes, three products) meets it at a third of the bf16 matrix rate -- on
ordinary AND hostile weights -- and is what the default mode runs; this path is the FAST VARIANT at half the rate
(``TT_REFERENCE_IMPL=f16c``; 9e-5 relative on ordinary weights, 7e-3 on the stress fixture: DESIGN.md section 4.6): every GEMM operand is carried as "c-planes" -- ``hi = fp16(x)`` plus two OCP e4m3 planes (``x`` and ``x - hi``)
with one E8M0 block exponent per 32 elements -- and a product runs as ``hi.hi`` on the fp16 matrix cores plus two
block-scaled e4m3 cross terms at twice the rate (``a.w ~= a_hi.w_hi + e4m3(a).e4m3(w_lo) + e4m3(a_lo).e4m3(w)``; the cross
terms are 2^-12 of the result, the dropped term 2^-24).  Attention on single fp16 products with fp32 softmax; the residual
stream, LayerNorm, exact-erf GELU and the classification head stay fp32.  ``precision.reference_impl()`` selects it only on
request, and only where the model shape fits (hidden a multiple of 256 with 64-wide heads: bge-m3, bge-reranker-v2-m3,
bge-reranker-base); the default is ``f16x3`` (``encoder_x3`` on fp16 planes), ``bf16x3`` / ``fp32`` the older implementations.
``encoder.Encoder`` runs it (``EncoderF16C`` is that class) with the 16-bit path's token packing and surface.
"""
from __future__ import annotations

from ctypes import Structure, c_void_p
from typing import Dict, Tuple

import torch

from . import _lib
from .encoder import Encoder, EncoderConfig, EncoderPath, _CheckpointWeights, _weights_struct


class _LayerWC(Structure):
    """tt_layer_weights_f16c: each projection's c-planes are followed by their block scales (``*_s``)."""
    _fields_ = [(n, c_void_p) for n in ("qkv_w", "qkv_s", "qkv_b", "o_w", "o_s", "o_b", "ln1_g", "ln1_b", "ffn1_w", "ffn1_s",
                                        "ffn1_b", "ffn2_w", "ffn2_s", "ffn2_b", "ln2_g", "ln2_b")]


_EncWC = _weights_struct("_EncWC", _LayerWC)

# the f16c GEMMs run whole 256-row tiles (no skinny kernel yet: one query's 64 rows are padded to one tile)
F16C_PATH = EncoderPath(forward="tt_encoder_forward_f16c", workspace="tt_encoder_f16c_workspace_bytes",
                        cls_forward="tt_encoder_forward_f16c_cls", cls_workspace="tt_encoder_f16c_cls_workspace_bytes",
                        pool="tt_embed_pool_f32", pool_mean="tt_embed_pool_mean_f32", head="tt_rerank_head_f16c",
                        scratch="encf16c", head_scratch="headf16c", hidden=torch.float32, row_tile=256,
                        no_fp8="fp8 calibration does not apply to the reference-precision path")

EncoderF16C = Encoder


def supports(cfg: EncoderConfig) -> bool:
    """Shapes the f16c kernels take (csrc/f16c_path.hip check_weights_c)."""
    return (cfg.hidden % 256 == 0 and cfg.hidden <= 1024 and cfg.hidden == cfg.heads * 64 and cfg.ffn % 256 == 0
            and cfg.layers > 0)


def quantize_planes(x: torch.Tensor, weight: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 [rows][k] on the device -> (c-planes uint8 [rows][4 k], tiled E8M0 scales uint8) through ``tt_f16c_quantize``."""
    lib = _lib.load_library()
    if x.device.type != "cuda" or x.dim() != 2 or x.shape[1] % 256:
        raise ValueError("quantize_planes takes a device fp32 matrix whose width is a multiple of 256")
    x = x.to(torch.float32).contiguous()
    rows, k = x.shape
    planes = torch.empty((rows, 4 * k), dtype=torch.uint8, device=x.device)
    scales = torch.zeros(int(lib.tt_f16c_scale_bytes(rows, k, 1 if weight else 0)), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.tt_f16c_quantize(x.data_ptr(), rows, k, 1 if weight else 0, planes.data_ptr(), scales.data_ptr(),
                                  torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(rc, "tt_f16c_quantize")
    return planes, scales


class EncoderWeightsF16C(_CheckpointWeights):
    """Device-resident f16c weights (HF checkpoint names, see ``encoder._CheckpointWeights``): matrices as c-planes (4 bytes
    per element + 1/16 byte of block scales: 2 x 1.13 GB for the 1024-wide models), tables / biases / LayerNorm / head in fp32."""

    gemm_dtype = "f16c"
    path = F16C_PATH
    _Struct = _EncWC

    def __init__(self, cfg: EncoderConfig, state: Dict[str, torch.Tensor], device: torch.device):
        if not supports(cfg):
            raise ValueError(f"the f16c path takes hidden % 256 == 0 with 64-wide heads and ffn % 256 == 0, not {cfg}")
        self._load(cfg, state, device)
        torch.cuda.synchronize(device)          # (the fp32 sources of the planes may be freed from here on)

    def _matrix(self, L, field, names, x):
        planes, scales = quantize_planes(x.to(device=self.device, dtype=torch.float32), weight=True)
        self._keep += [planes, scales]
        setattr(L, field, planes.data_ptr())
        setattr(L, field[:-1] + "s", scales.data_ptr())         # qkv_w -> qkv_s

    def set_gemm_dtype(self, dtype: str) -> None:
        if dtype not in ("f16c", "reference", "float32", "fp32"):
            raise ValueError(f"f16c weights run in reference precision only (asked for {dtype!r})")
