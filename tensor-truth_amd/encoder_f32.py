"""Reference-precision (fp32) encoder: host side of ``tt_encoder_forward_f32`` (csrc/f32_path.hip).

The reference's embedder / reranker run in fp32 unless configured otherwise
(``src/tensortruth/app_utils/config_schema.py:66-76``: ``torch_dtype: None``;
``services/model_manager.py:218-229``).  ``model_kwargs={"torch_dtype": "float32"}`` on the HIP embedding model or
rerank postprocessor selects this path: fp32 weights and activations, fp32 MFMA -- scores within 1e-3 relative of the
CPU reference (north_star's tolerance), at about 1/10 of the bf16 path's throughput: meant for the interactive case
(one query's candidate pairs), not for bulk ingest.  ``encoder.Encoder`` runs it (``EncoderF32`` is that class) with the
16-bit path's token packing and surface; there is no CLS-only last layer, so pooling and the head read the full forward.
"""
from __future__ import annotations

from typing import Dict

import torch

from .encoder import Encoder, EncoderConfig, EncoderPath, _CheckpointWeights, _PlainLayerW, _weights_struct

_EncWF = _weights_struct("_EncWF", _PlainLayerW)

F32_PATH = EncoderPath(forward="tt_encoder_forward_f32", workspace="tt_encoder_f32_workspace_bytes",
                       cls_forward=None, cls_workspace=None,
                       pool="tt_embed_pool_f32", pool_mean="tt_embed_pool_mean_f32", head="tt_rerank_head_f32",
                       scratch="enc32", head_scratch="head32", hidden=torch.float32,
                       no_fp8="fp8 calibration does not apply to the float32 path")

EncoderF32 = Encoder


class EncoderWeightsF32(_CheckpointWeights):
    """Device-resident fp32 weights (HF checkpoint names, see ``encoder._CheckpointWeights``)."""

    gemm_dtype = "float32"
    path = F32_PATH
    _Struct = _EncWF

    def __init__(self, cfg: EncoderConfig, state: Dict[str, torch.Tensor], device: torch.device):
        self._load(cfg, state, device)

    def set_gemm_dtype(self, dtype: str) -> None:
        if dtype not in ("float32", "fp32", "bf16"):
            raise ValueError(f"the fp32 weights run in float32 only (asked for {dtype!r})")
