"""ctypes binding of libtt_hip.so (include/tt_hip.h).  Fails loudly when the HIP
library has not been built -- there is deliberately no fallback path."""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libtt_hip.so"
_lock = threading.Lock()
_lib = None


class LibraryNotBuiltError(RuntimeError):
    pass


class TTError(RuntimeError):
    """A libtt_hip.so call returned a non-zero status."""


def lib_path() -> str:
    # TT_LIB_NAME=libtt_hip_diag.so: the diagnostic build (csrc `make DIAG=1`), for tools/probes only
    return os.path.join(_HERE, os.environ.get("TT_LIB_NAME") or _LIB_NAME)


def is_diag() -> bool:
    """True when the diagnostic build is the one loaded (TT_LIB_NAME=libtt_hip_diag.so, `make DIAG=1`) -- the only build that
    reads the kernels' A/B environment switches; the product library reads no environment variable at all."""
    return "diag" in (os.environ.get("TT_LIB_NAME") or "")


_isa_ok = None


def isa_checked() -> bool:
    """True when csrc/check_isa.py has disassembled THIS build of the library and found no packed-f32 instruction of the form
    that misbehaves beside another stream's MFMAs (its stamp, ``libtt_hip.so.isa_ok``, holds the library's sha256).  Code that
    runs kernels on two streams at once (the retriever's own stream, vector_index.py) asks first and stays on one stream
    otherwise."""
    global _isa_ok
    if _isa_ok is None:
        import hashlib

        ok = False
        try:
            with open(lib_path() + ".isa_ok") as fh:
                want = fh.read().strip()
            h = hashlib.sha256()
            with open(lib_path(), "rb") as fh:
                for blk in iter(lambda: fh.read(1 << 20), b""):
                    h.update(blk)
            ok = h.hexdigest() == want
        except OSError:
            ok = False
        _isa_ok = ok
    return _isa_ok


_F32P = ctypes.POINTER(c_float)
_I32P = ctypes.POINTER(c_int32)

# name -> (restype, argtypes); must list every symbol include/tt_hip.h declares
SIGNATURES = {
    "tt_version": (c_int, []),
    "tt_arch": (c_char_p, []),
    "tt_last_error": (c_char_p, []),
    "tt_device_cu_count": (c_int, []),
    "tt_scan_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "tt_scan_topk": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int, c_int32, c_void_p, c_void_p,
                             c_void_p, c_size_t, c_void_p, c_void_p]),
    "tt_scan_exact_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "tt_scan_topk_exact": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int, c_int32, c_void_p, c_void_p,
                                   c_void_p, c_size_t, c_void_p]),
    "tt_scan_segmented_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "tt_scan_topk_segmented": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_scan_shadow_bytes": (c_size_t, [c_int64, c_int]),
    "tt_scan_shadow_build": (c_int, [c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_void_p]),
    "tt_scan_shadow_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "tt_scan_topk_shadow": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int, c_int, c_int32, c_void_p, c_void_p,
                                    c_void_p, c_size_t, c_void_p, c_void_p]),
    # MMR over the scan's hits (csrc/mmr.hip)
    "tt_mmr_workspace_bytes": (c_size_t, [c_int, c_int]),
    "tt_mmr_select": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_int32,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_filter_rows_workspace_bytes": (c_size_t, [c_int64]),
    "tt_filter_rows": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                               c_void_p, c_size_t, c_void_p]),
    "tt_scan_topk_rows_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int]),
    "tt_scan_topk_rows": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_int,
                                  c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "tt_topk_merge": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_encoder_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_encoder_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_encoder_cls_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "tt_encoder_forward_cls": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_embed_pool": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_embed_pool_mean": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_embed_pool_mean_f32": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    # fp16 twins of the 16-bit path (same signatures)
    "tt_encoder_workspace_bytes_f16": (c_size_t, [c_void_p, c_int]),
    "tt_encoder_cls_workspace_bytes_f16": (c_size_t, [c_void_p, c_int, c_int]),
    "tt_encoder_forward_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_encoder_forward_cls_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_embed_pool_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_embed_pool_mean_f16": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_rerank_head_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_gemm_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_layernorm_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "tt_attention_varlen_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                    c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_attention_cls_varlen_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                    c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_rerank_head": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_adjacent_cosine": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "tt_gemm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_layernorm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "tt_attention_varlen": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                    c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_attention_cls_varlen": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                    c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_quantize_rows_fp8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_layernorm_bf16_fp8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p,
                                      c_void_p]),
    "tt_gemm_fp8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                            c_void_p]),
    "tt_gemm_fp8_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                               c_int, c_int, c_int, c_int, c_void_p]),
    "tt_encoder_f32_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_encoder_forward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_embed_pool_f32": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_rerank_head_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_gemm_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_encoder_x3_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_encoder_x3_cls_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "tt_encoder_forward_x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_encoder_forward_x3_cls": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_rerank_head_x3": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_split_planes": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "tt_gemm_x3": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_gemm_x3_ex": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                              c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_attention_x3": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "tt_attention_x3_hd": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                   c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    # the split-plane forward with fp16 planes ("f16x3": x3_path.hip's second instantiation)
    "tt_encoder_x3_workspace_bytes_f16": (c_size_t, [c_void_p, c_int]),
    "tt_encoder_x3_cls_workspace_bytes_f16": (c_size_t, [c_void_p, c_int, c_int]),
    "tt_encoder_forward_x3_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_encoder_forward_x3_cls_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_rerank_head_x3_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_split_planes_f16": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "tt_gemm_x3_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_gemm_x3_ex_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                  c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_attention_x3_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                    c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "tt_attention_x3_hd_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int,
                                       c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    # reference precision on two matrix-time units (csrc/f16c_path.hip)
    "tt_encoder_f16c_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_encoder_f16c_cls_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "tt_encoder_forward_f16c": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_encoder_forward_f16c_cls": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                            c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_rerank_head_f16c": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_f16c_scale_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "tt_f16c_quantize": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_gemm_f16c": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                             c_int, c_void_p]),
    "tt_attention_f16c": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                  c_int, c_int, c_void_p]),
    # decoder embedder (Qwen3Model architecture) and its fp16 twins (same signatures)
    "tt_decoder_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_decoder_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                               c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_decoder_rows_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int]),
    "tt_decoder_forward_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_decoder_score": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_embed_pool_last": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_qk_norm_rope": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                             c_void_p, c_int, c_void_p]),
    "tt_attention_causal_gqa": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_decoder_workspace_bytes_f16": (c_size_t, [c_void_p, c_int]),
    "tt_decoder_forward_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_decoder_rows_workspace_bytes_f16": (c_size_t, [c_void_p, c_int, c_int]),
    "tt_decoder_forward_rows_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_decoder_score_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_embed_pool_last_f16": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_qk_norm_rope_f16": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                                 c_void_p, c_int, c_void_p]),
    "tt_attention_causal_gqa_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                         c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    # ModernBERT encoders (csrc/modernbert.hip) and their fp16 twins (same signatures)
    "tt_modernbert_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_modernbert_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_modernbert_head": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_rope_v8": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p]),
    "tt_attention_window": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                    c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_modernbert_workspace_bytes_f16": (c_size_t, [c_void_p, c_int]),
    "tt_modernbert_forward_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_modernbert_head_f16": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_rope_v8_f16": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p]),
    "tt_attention_window_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    # EmbeddingGemma embedders (csrc/gemma.hip): bf16 only, no twins
    "tt_gemma_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_gemma_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                 c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_gemma_pool_dense": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_gemma_qk_norm_rope": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float,
                                      c_void_p, c_int, c_void_p]),
    "tt_gemma_add_norm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "tt_attention_window_gqa": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    # MPNet encoders (csrc/mpnet.hip) and their fp16 twins (same signatures)
    "tt_mpnet_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_mpnet_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                 c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_attention_relbias": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "tt_mpnet_workspace_bytes_f16": (c_size_t, [c_void_p, c_int]),
    "tt_mpnet_forward_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                     c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_attention_relbias_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                         c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    # DeBERTa-v2 / v3 cross-encoders (csrc/deberta.hip) and their fp16 twins (same signatures)
    "tt_deberta_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_deberta_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
        c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_deberta_head": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_attention_disentangled": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
        c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "tt_deberta_workspace_bytes_f16": (c_size_t, [c_void_p, c_int]),
    "tt_deberta_forward_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
        c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_deberta_head_f16": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "tt_attention_disentangled_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
        c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    # RoPE-BERT encoders: NomicBERT, Jina-v3 (csrc/ropebert.hip) and their fp16 twins (same signatures)
    "tt_ropebert_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_ropebert_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_ropebert_workspace_bytes_f16": (c_size_t, [c_void_p, c_int]),
    "tt_ropebert_forward_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    # T5 encoders (csrc/t5.hip): bf16 only, no twins
    "tt_t5_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_t5_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_t5_pool_dense": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    # JinaBERT encoders: jina-embeddings-v2 (csrc/jinabert.hip) and their fp16 twins (same signatures)
    "tt_jinabert_workspace_bytes": (c_size_t, [c_void_p, c_int]),
    "tt_jinabert_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_attention_alibi": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "tt_jinabert_workspace_bytes_f16": (c_size_t, [c_void_p, c_int]),
    "tt_jinabert_forward_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_attention_alibi_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                       c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    # ColBERT late interaction (csrc/colbert.hip; the key-limited forward is encoder_api.hip's) and the fp16 twins (same signatures)
    "tt_maxsim": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                          c_void_p]),
    "tt_maxsim_scan_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "tt_maxsim_scan_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_maxsim_scan_topk_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                                        c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_colbert_project": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "tt_attention_keylimit": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                      c_int, c_int, c_int, c_int, c_void_p]),
    "tt_encoder_forward_keylen": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                          c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_maxsim_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                              c_void_p]),
    "tt_colbert_project_f16": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "tt_attention_keylimit_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                          c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "tt_encoder_forward_keylen_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                              c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    # BGE-M3's lexical head (csrc/lexical.hip): token weights (bf16 / fp16 / fp32 hidden states), lexical + hybrid scores, exact scan
    "tt_lexical_weights": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                   c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tt_lexical_weights_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tt_lexical_weights_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tt_lexical_score": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int, c_void_p, c_void_p, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tt_lexical_scan_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "tt_lexical_scan_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                     c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_hybrid_scan_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "tt_hybrid_scan_topk": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_int64, c_void_p, c_void_p, c_int, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                    c_size_t, c_void_p]),
    # posting lists over the lexical / SPLADE stores (csrc/postings.hip): the build, and the scan's top-k over a query's lists
    "tt_postings_build_workspace_bytes": (c_size_t, [c_int]),
    "tt_postings_build": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p,
                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "tt_lexical_topk_postings_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int]),
    "tt_lexical_topk_postings": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                         c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # BGE-M3's multi-vector head (csrc/multivec.hip): the wide projection (bf16 / fp16 / fp32 in), the wide MaxSim, the three-way mix
    "tt_multivec_project": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "tt_multivec_project_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                        c_void_p]),
    "tt_multivec_project_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                        c_void_p]),
    "tt_maxsim_wide": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                               c_void_p, c_void_p]),
    "tt_maxsim_wide_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_void_p]),
    "tt_m3_mix": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_void_p, c_void_p]),
    # SPLADE (csrc/splade.hip): the vocabulary projection with its segmented maximum (bf16 / fp16), the sparse compaction
    "tt_splade_pool": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                               c_void_p, c_int, c_void_p]),
    "tt_splade_pool_f16": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_void_p, c_int, c_void_p]),
    "tt_sparse_compact": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "tt_prof_enable": (c_int, [c_int]),
    "tt_prof_read": (c_int, [c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int)]),
}


def load_library():
    """Load (once) and return the ctypes handle; raises LibraryNotBuiltError."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.path.exists(path):
            raise LibraryNotBuiltError(
                f"{path} not found. Build it first: `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C {os.path.join(_HERE, 'csrc')}` (needs hipcc, --offload-arch=gfx950). "
                "tensor_truth_amd has no CPU fallback."
            )
        # torch FIRST: its wheel carries its own copy of the HIP runtime, and whichever copy initialises second in a process sees
        # "no ROCm-capable device" -- the library's launches must land on the runtime torch's tensors and streams live in
        import torch  # noqa: F401

        lib = ctypes.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so is stale
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load_library().tt_last_error().decode("utf-8", "replace")
        raise TTError(f"{what} failed with status {status}: {msg}")
