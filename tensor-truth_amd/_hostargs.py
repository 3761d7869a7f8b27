"""What the host wrappers of the retrieval kernels (``colbert.py``, ``lexical.py``, ``splade.py``, ``multivec.py``, ``postings.py``)
share: the checks and uploads of their array arguments, the resolution of a device and a 16-bit type from constructor arguments,
and the doubling growth of a store's arrays.  Each is defined here once; the modules import the names they use."""
from __future__ import annotations

import json
from typing import Optional

import numpy as np
import torch


# ---- kernel arguments ---------------------------------------------------------------------------------------------------------------
def _stream(dev: torch.device):
    return torch.cuda.current_stream(dev).cuda_stream


def _check_range(name: str, a, lo: int, hi) -> None:
    a = np.asarray(a)
    bad = (a < lo) | (a > hi)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{name}[{i}]={int(a.flat[i])} is outside {lo} .. {int(np.asarray(hi).flat[i]) if np.ndim(hi) else hi}")


def _dev_i(a, dtype, dev: torch.device) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        if a.device.type != dev.type or (dev.index is not None and a.device.index != dev.index) or a.dtype != dtype \
                or not a.is_contiguous():
            raise ValueError(f"a contiguous device array of {dtype} on {dev} is expected")
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype={torch.int32: np.int32, torch.int64: np.int64}[dtype])).to(dev)


def _need_device(name: str, *tensors: torch.Tensor) -> torch.device:
    dev = tensors[0].device
    if dev.type != "cuda" or any(t.device != dev for t in tensors):
        raise RuntimeError(f"{name}: device tensors are needed; tensor_truth_amd has no CPU path")
    return dev


def _suffix(dtype: torch.dtype) -> str:
    if dtype == torch.bfloat16:
        return ""
    if dtype == torch.float16:
        return "_f16"
    raise ValueError(f"16-bit operands are bfloat16 or float16, not {dtype}")


# ---- constructor arguments ------------------------------------------------------------------------------------------------------------
def read_json(path: str) -> dict:
    with open(path, encoding="utf-8") as f:
        d = json.load(f)
    if not isinstance(d, dict):
        raise ValueError(f"{path}: a JSON object is expected")
    return d


def resolve_device(device: Optional[str]) -> torch.device:
    """A constructor's ``device`` (None or "cuda": the current one) -> an indexed ``cuda`` device; anything else is refused."""
    dev = torch.device("cuda" if device in (None, "cuda") else device)
    if dev.type != "cuda":
        raise RuntimeError(f"device '{device}': tensor_truth_amd runs on HIP devices only (no CPU path)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def resolve_dtype(model_kwargs: Optional[dict], family: str) -> torch.dtype:
    """``model_kwargs["torch_dtype"]`` (or ``["precision"]``) of a ``family`` ("ColBERT", "SPLADE") model -> bfloat16 (the default)
    or float16; anything else is refused."""
    mk = model_kwargs or {}
    td = mk.get("torch_dtype")
    name = str(td).replace("torch.", "") if td is not None else None
    if name is None and mk.get("precision") is not None:
        name = {"bf16": "bfloat16", "fp16": "float16"}.get(str(mk["precision"]).lower(), str(mk["precision"]))
        if name not in ("bfloat16", "float16"):
            raise NotImplementedError(f"precision={mk['precision']!r} is not available for {family} checkpoints: torch_dtype bfloat16 "
                                      "(the default) or float16")
    if name is None or name in ("bfloat16", "bf16"):
        return torch.bfloat16
    if name in ("float16", "fp16", "half"):
        return torch.float16
    raise NotImplementedError(f"torch_dtype={td!r} is not available for {family} checkpoints: bfloat16 (the default) or float16")


# ---- a store's arrays -----------------------------------------------------------------------------------------------------------------
def grown(t: torch.Tensor, used: int, need: int) -> torch.Tensor:
    """``t`` if it has ``need`` rows, else a zeroed array of twice the rows (and twice again until it has) with the ``used`` first
    rows copied."""
    cap = t.shape[0]
    if need <= cap:
        return t
    while cap < need:
        cap *= 2
    new = torch.zeros((cap,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    new[:used].copy_(t[:used])
    return new
