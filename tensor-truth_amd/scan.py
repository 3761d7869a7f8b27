"""Exact similarity scan + top-k on MI355X (host side of include/tt_hip.h's scan API).

Stands in for the vector search the reference reaches through
``index.as_retriever(similarity_top_k=...)`` (``src/tensortruth/rag_engine.py:639``)
-> ``ChromaVectorStore.query``: given L2-normalised query embeddings it returns,
per query, the ``k`` corpus rows with the largest dot product, ordered by
(score desc, row index asc).  The corpus is a row-major bf16 matrix resident in
HBM (a shard of it under multi-GPU row sharding, see ``sharded.py``).
"""
from __future__ import annotations

import threading
from typing import Optional, Tuple

import torch

from . import _lib


def _require_cuda(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} must live on a HIP device (got {t.device}); tensor_truth_amd has no CPU path"
        )


class _Workspace(threading.local):
    """Per-thread scratch buffers, so concurrent retrieve() calls from the
    reference's executor threads (rag_engine.py:420-424) never share scratch."""

    def __init__(self):
        self.bufs = {}

    def get(self, device: torch.device, nbytes: int) -> torch.Tensor:
        key = (device.type, device.index)
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
            self.bufs[key] = buf
        return buf


_ws = _Workspace()


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class ScanShadow:
    """The fp8 shadow of a corpus matrix (``tt_scan_shadow_build``, csrc/shadow.hip): one e4m3 byte per element plus two floats
    per row, an EXACT prefilter for the scan of a lone caller -- ``scan_topk(..., shadow=)`` then reads half the bytes and returns
    bit-identical scores and indices.  ``rows`` = how many rows of the matrix the block currently mirrors (``extend`` adds the rows
    appended since; a row rewritten in place -- a tombstone -- needs ``rebuild``)."""

    MIN_ROWS = 1 << 20           # below this a bf16 pass is a few hundred microseconds: nothing to win
    MAX_QUERIES = 4

    def __init__(self, corpus: torch.Tensor, cap_rows: Optional[int] = None):
        _require_cuda(corpus, "corpus")
        if corpus.dtype != torch.bfloat16 or corpus.dim() != 2 or not corpus.is_contiguous():
            raise TypeError("the shadow mirrors a contiguous [N, D] torch.bfloat16 matrix")
        self.dim = int(corpus.shape[1])
        self.cap_rows = int(cap_rows if cap_rows is not None else corpus.shape[0])
        lib = _lib.load_library()
        nbytes = lib.tt_scan_shadow_bytes(self.cap_rows, self.dim)
        if nbytes == 0:
            raise ValueError(f"no shadow for {self.cap_rows} rows x {self.dim}")
        self._raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=corpus.device)
        self.ptr = (self._raw.data_ptr() + 255) // 256 * 256
        self.rows = 0
        self.base_ptr = corpus.data_ptr()
        self.ready = torch.cuda.Event()       # recorded behind every build: a search on ANOTHER stream waits for it (scan_topk)
        self.extend(corpus, int(corpus.shape[0]))

    def extend(self, corpus: torch.Tensor, n_rows: int) -> None:
        """Mirror rows [self.rows, n_rows) of ``corpus`` (rows appended since the last call)."""
        if n_rows > self.cap_rows or corpus.shape[1] != self.dim:
            raise ValueError("the shadow's capacity / width does not fit this matrix")
        if n_rows <= self.rows:
            return
        lib = _lib.load_library()
        with torch.cuda.device(corpus.device):
            rc = lib.tt_scan_shadow_build(corpus.data_ptr(), self.dim, self.rows, n_rows, self.ptr, self.cap_rows, _stream_ptr(corpus.device))
            _lib.check(rc, "tt_scan_shadow_build")
            self.ready.record(torch.cuda.current_stream(corpus.device))
        self.rows = n_rows

    def rebuild(self, corpus: torch.Tensor, n_rows: int) -> None:
        self.rows = 0
        self.extend(corpus, n_rows)

    def serves(self, n_rows: int, n_queries: int, k: int) -> bool:
        return (self.rows >= n_rows >= max(self.MIN_ROWS, 128 * k) and 0 < n_queries <= self.MAX_QUERIES)


def scan_topk(
    corpus: torch.Tensor,
    queries: torch.Tensor,
    k: int,
    idx_base: int = 0,
    exact_dense: bool = False,
    check_overflow: bool = True,
    return_flag: bool = False,
    _packed: Optional[torch.Tensor] = None,
    shadow: Optional[ScanShadow] = None,
):
    """corpus [N,D] bf16, queries [Q,D] bf16 (same HIP device) ->
    (scores [Q,k] fp32, idx [Q,k] int32), idx = idx_base + row, padding (-inf, -1).

    ``exact_dense`` forces the dense-score path (N*Q*4 bytes of scratch).
    ``check_overflow`` reads the device status word (one sync) and transparently
    re-runs through the dense path if a candidate list overflowed.
    ``return_flag`` (tests / diagnostics): no fallback, returns ``(scores, idx, overflowed)``.
    """
    lib = _lib.load_library()
    _require_cuda(corpus, "corpus")
    _require_cuda(queries, "queries")
    if corpus.dtype != torch.bfloat16 or queries.dtype != torch.bfloat16:
        raise TypeError("corpus and queries must be torch.bfloat16")
    if corpus.dim() != 2 or queries.dim() != 2 or corpus.shape[1] != queries.shape[1]:
        raise ValueError(f"shape mismatch: corpus {tuple(corpus.shape)} queries {tuple(queries.shape)}")
    if corpus.device != queries.device:
        raise ValueError("corpus and queries must be on the same device")
    if not corpus.is_contiguous() or not queries.is_contiguous():
        raise ValueError("corpus and queries must be contiguous row-major")
    n, d = corpus.shape
    q = queries.shape[0]
    dev = corpus.device
    if _packed is not None:      # scan_topk_host: scores, indices and the status word in ONE buffer (one copy back, one sync)
        out_s = _packed[: q * k].view(torch.float32).view(q, k)
        out_i = _packed[q * k: 2 * q * k].view(q, k)
    else:
        out_s = torch.empty((q, k), dtype=torch.float32, device=dev)
        out_i = torch.empty((q, k), dtype=torch.int32, device=dev)
    if q == 0:
        return out_s, out_i
    with torch.cuda.device(dev):
        st = _stream_ptr(dev)
        if exact_dense:
            need = lib.tt_scan_exact_workspace_bytes(n, d, q, k)
            ws = _ws.get(dev, need)
            rc = lib.tt_scan_topk_exact(corpus.data_ptr(), n, d, queries.data_ptr(), q, k, idx_base,
                                        out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), st)
            _lib.check(rc, "tt_scan_topk_exact")
            return out_s, out_i
        use_shadow = shadow is not None and shadow.dim == d and shadow.serves(n, q, k)
        need = lib.tt_scan_shadow_workspace_bytes(n, d, q, k) if use_shadow else lib.tt_scan_workspace_bytes(n, d, q, k)
        ws = _ws.get(dev, need + 256)
        base = (ws.data_ptr() + 255) // 256 * 256
        if _packed is not None:
            flag = _packed[2 * q * k:]
            flag.zero_()
        else:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if use_shadow:
            torch.cuda.current_stream(dev).wait_event(shadow.ready)     # (built / extended on whatever stream its first user ran on)
            # a lone caller's scan: one pass over the fp8 shadow, the survivors re-scored from the bf16 rows -- the same bits out
            rc = lib.tt_scan_topk_shadow(corpus.data_ptr(), shadow.ptr, shadow.cap_rows, n, d, queries.data_ptr(), q, k, idx_base,
                                         out_s.data_ptr(), out_i.data_ptr(), base, ws.numel() - (base - ws.data_ptr()),
                                         flag.data_ptr(), st)
            _lib.check(rc, "tt_scan_topk_shadow")
        else:
            rc = lib.tt_scan_topk(corpus.data_ptr(), n, d, queries.data_ptr(), q, k, idx_base,
                                  out_s.data_ptr(), out_i.data_ptr(), base, ws.numel() - (base - ws.data_ptr()),
                                  flag.data_ptr(), st)
            _lib.check(rc, "tt_scan_topk")
        if _packed is not None:
            return out_s, out_i
        if return_flag:
            return out_s, out_i, int(flag.item())
        if check_overflow and int(flag.item()) != 0:
            return scan_topk(corpus, queries, k, idx_base, exact_dense=True)
    return out_s, out_i


def scan_topk_host(corpus: torch.Tensor, queries: torch.Tensor, k: int, idx_base: int = 0, shadow: Optional[ScanShadow] = None):
    """``scan_topk`` for callers that need the hits ON THE HOST (the retriever turns rows into nodes): scores, indices and the
    overflow status word live in one device buffer and come back in ONE copy -- the wait for the hits is the only host sync of a
    scan batch (``scan_topk`` itself reads the flag with its own ``.item()`` before the caller's ``.cpu()``: two syncs, 0.04 ms of
    a 0.74 ms shard batch).  A flagged overflow re-runs the dense exact path, as ``scan_topk`` does.
    -> (scores [Q,k] fp32, idx [Q,k] int32), CPU tensors."""
    q = queries.shape[0]
    if q == 0:
        return torch.empty((0, k), dtype=torch.float32), torch.empty((0, k), dtype=torch.int32)
    packed = torch.empty(2 * q * k + 1, dtype=torch.int32, device=corpus.device)
    scan_topk(corpus, queries, k, idx_base, _packed=packed, shadow=shadow)
    host = packed.cpu()                                   # the one sync (current stream only)
    if int(host[-1]) != 0:
        s, i = scan_topk(corpus, queries, k, idx_base, exact_dense=True)
        return s.cpu(), i.cpu()
    return host[: q * k].view(torch.float32).view(q, k), host[q * k: 2 * q * k].view(q, k)


MMR_PENALTIES = {"max": 0, "last": 1}
MMR_MAX_CANDIDATES = 1024
_MMR_WS_CAP = 64 << 20          # mmr_select's Gram matrices per launch: queries go in chunks that stay at or below this


def mmr_select(corpus: torch.Tensor, cand: torch.Tensor, rel: torch.Tensor, k: int, lam: float, penalty: str = "max",
               idx_base: int = 0, _packed: Optional[torch.Tensor] = None):
    """``tt_mmr_select``: maximal marginal relevance over candidate lists.  corpus [N,D] bf16; cand [Q,P] int32 and rel [Q,P] fp32
    exactly as ``scan_topk`` returned them (same device; P <= 1024, entries < 0 are padding) ->
    (mmr [Q,k] fp32, rel [Q,k] fp32, idx [Q,k] int32, pos [Q,k] int32) in selection order: the value each pick won with, its scan
    score, its entry of ``cand`` and its position in the list; padding (-inf, -inf, -1, -1) when fewer than k can be picked.

    ``lam`` in [0, 1] weighs relevance against the similarity penalty (1: plain top-k order).  ``penalty``: "max", the maximum
    similarity to everything picked so far (Carbonell & Goldstein), or "last", the similarity to the most recent pick only.
    Stream-ordered, no host sync; the pairwise similarities live in the thread-local workspace."""
    lib = _lib.load_library()
    _require_cuda(corpus, "corpus")
    _require_cuda(cand, "cand")
    _require_cuda(rel, "rel")
    if corpus.dtype != torch.bfloat16 or cand.dtype != torch.int32 or rel.dtype != torch.float32:
        raise TypeError("corpus must be torch.bfloat16, cand torch.int32 and rel torch.float32")
    if corpus.dim() != 2 or cand.dim() != 2 or cand.shape != rel.shape:
        raise ValueError(f"shape mismatch: corpus {tuple(corpus.shape)} cand {tuple(cand.shape)} rel {tuple(rel.shape)}")
    if corpus.device != cand.device or corpus.device != rel.device:
        raise ValueError("corpus, cand and rel must be on the same device")
    if not corpus.is_contiguous() or not cand.is_contiguous() or not rel.is_contiguous():
        raise ValueError("corpus, cand and rel must be contiguous row-major")
    if penalty not in MMR_PENALTIES:
        raise ValueError(f"penalty {penalty!r}: one of {sorted(MMR_PENALTIES)}")
    n, d = corpus.shape
    q, p = cand.shape
    dev = corpus.device
    if _packed is not None:      # search_mmr_host: the four outputs in one buffer
        m = q * k
        outs = (_packed[:m].view(torch.float32).view(q, k), _packed[m: 2 * m].view(torch.float32).view(q, k),
                _packed[2 * m: 3 * m].view(q, k), _packed[3 * m: 4 * m].view(q, k))
    else:
        outs = (torch.empty((q, k), dtype=torch.float32, device=dev), torch.empty((q, k), dtype=torch.float32, device=dev),
                torch.empty((q, k), dtype=torch.int32, device=dev), torch.empty((q, k), dtype=torch.int32, device=dev))
    if q == 0:
        return outs
    per_query = int(lib.tt_mmr_workspace_bytes(1, p))
    chunk = q if per_query == 0 else max(1, min(q, _MMR_WS_CAP // per_query))     # (per_query == 0: the call below refuses p)
    with torch.cuda.device(dev):
        st = _stream_ptr(dev)
        ws = _ws.get(dev, chunk * per_query + 256)
        base = (ws.data_ptr() + 255) // 256 * 256
        for lo in range(0, q, chunk):
            nq = min(chunk, q - lo)
            rc = lib.tt_mmr_select(corpus.data_ptr(), n, d, cand[lo:].data_ptr(), rel[lo:].data_ptr(), nq, p, k, float(lam),
                                   MMR_PENALTIES[penalty], idx_base, outs[0][lo:].data_ptr(), outs[1][lo:].data_ptr(),
                                   outs[2][lo:].data_ptr(), outs[3][lo:].data_ptr(), base, ws.numel() - (base - ws.data_ptr()), st)
            _lib.check(rc, "tt_mmr_select")
    return outs


def scan_topk_segmented(corpus: torch.Tensor, queries: torch.Tensor, k: int, seg_offsets) -> Tuple[torch.Tensor, torch.Tensor]:
    """Several index modules in one matrix: rows ``[seg_offsets[s], seg_offsets[s+1])`` are module ``s``.
    One pass over the matrix, then an exact top-k per (query, module) ->
    (scores [Q,S,k] fp32, rows [Q,S,k] int32, module-local, padding (-inf, -1)).
    Stands in for the reference's per-module thread fan-out (``rag_engine.py:420-424``)."""
    import ctypes
    lib = _lib.load_library()
    _require_cuda(corpus, "corpus")
    _require_cuda(queries, "queries")
    if corpus.dtype != torch.bfloat16 or queries.dtype != torch.bfloat16:
        raise TypeError("corpus and queries must be torch.bfloat16")
    if corpus.dim() != 2 or queries.dim() != 2 or corpus.shape[1] != queries.shape[1]:
        raise ValueError(f"shape mismatch: corpus {tuple(corpus.shape)} queries {tuple(queries.shape)}")
    if corpus.device != queries.device:
        raise ValueError("corpus and queries must be on the same device")
    if not corpus.is_contiguous() or not queries.is_contiguous():
        raise ValueError("corpus and queries must be contiguous row-major")
    offs = [int(o) for o in seg_offsets]
    n_seg = len(offs) - 1
    if n_seg < 1:
        raise ValueError("seg_offsets needs at least two entries")
    n, d = corpus.shape
    q = queries.shape[0]
    dev = corpus.device
    out_s = torch.empty((q, n_seg, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((q, n_seg, k), dtype=torch.int32, device=dev)
    if q == 0:
        return out_s, out_i
    c_offs = (ctypes.c_int64 * (n_seg + 1))(*offs)
    with torch.cuda.device(dev):
        need = lib.tt_scan_segmented_workspace_bytes(max(offs[-1] - offs[0], 0), d, q, k)
        ws = _ws.get(dev, need + 256)
        base = (ws.data_ptr() + 255) // 256 * 256
        rc = lib.tt_scan_topk_segmented(corpus.data_ptr(), n, d, queries.data_ptr(), q, k, c_offs, n_seg,
                                        out_s.data_ptr(), out_i.data_ptr(), base,
                                        ws.numel() - (base - ws.data_ptr()), _stream_ptr(dev))
        _lib.check(rc, "tt_scan_topk_segmented")
    return out_s, out_i


def filter_rows(compiled, n_rows: int, device, seg_offsets=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``tt_filter_rows``: the rows of ``[0, n_rows)`` (or of the segments ``seg_offsets``) that pass a compiled metadata filter
    (``metadata_filter.compile_filter``) -> (rows int32 [capacity], list offsets int32 [S + 1]), both on the device: the list
    is ascending, segment s is ``rows[offsets[s]:offsets[s+1]]`` and ``offsets[S]`` is the count.  No host sync."""
    import ctypes
    lib = _lib.load_library()
    offs = [0, int(n_rows)] if seg_offsets is None else [int(o) for o in seg_offsets]
    n_seg = len(offs) - 1
    span = offs[-1] - offs[0]
    rows = torch.empty(max(span, 1), dtype=torch.int32, device=device)
    list_off = torch.empty(n_seg + 1, dtype=torch.int32, device=device)
    n_cl = len(compiled.columns)
    c_codes = (ctypes.c_void_p * n_cl)(*[c.data_ptr() for c in compiled.columns])
    c_bits = (ctypes.c_void_p * n_cl)(*[b.data_ptr() for b in compiled.bitsets])
    c_ncodes = (ctypes.c_int32 * n_cl)(*compiled.n_codes)
    c_offs = (ctypes.c_int64 * (n_seg + 1))(*offs) if seg_offsets is not None else None
    with torch.cuda.device(device):
        need = lib.tt_filter_rows_workspace_bytes(span)
        ws = _filter_ws.get(device, need + 256)
        base = (ws.data_ptr() + 255) // 256 * 256
        rc = lib.tt_filter_rows(n_cl, c_codes, c_bits, c_ncodes, 1 if compiled.any else 0, int(n_rows), c_offs, n_seg,
                                rows.data_ptr(), list_off.data_ptr(), base, ws.numel() - (base - ws.data_ptr()), _stream_ptr(device))
        _lib.check(rc, "tt_filter_rows")
    return rows, list_off


_filter_ws = _Workspace()      # (tt_filter_rows' masks live across the call only; own buffers: a rows scan follows on the same thread)


def scan_topk_rows(corpus: torch.Tensor, queries: torch.Tensor, k: int, rows: torch.Tensor, list_offsets: torch.Tensor,
                   max_rows: int, seg_offsets=None, idx_base: int = 0, check_overflow: bool = True, return_flag: bool = False,
                   _packed: Optional[torch.Tensor] = None):
    """``tt_scan_topk_rows``: the exact top-k over exactly the rows a ``filter_rows`` list names -- bit-identical to ``scan_topk``
    over ``corpus.index_select(0, listed rows)`` with the indices mapped back to rows.  ``max_rows`` = the host's upper bound on
    the rows listed per segment.  ``seg_offsets`` None -> (scores [Q, k], idx_base + rows [Q, k]); else (scores [Q, S, k],
    segment-local rows [Q, S, k]).  Padding (-inf, -1).  An overflowed candidate list (status word) re-runs the dense exact path
    over the gathered rows, as ``scan_topk`` does.  The fp8 shadow is not used here."""
    import ctypes
    lib = _lib.load_library()
    _require_cuda(corpus, "corpus")
    _require_cuda(queries, "queries")
    if corpus.dtype != torch.bfloat16 or queries.dtype != torch.bfloat16:
        raise TypeError("corpus and queries must be torch.bfloat16")
    if corpus.dim() != 2 or queries.dim() != 2 or corpus.shape[1] != queries.shape[1]:
        raise ValueError(f"shape mismatch: corpus {tuple(corpus.shape)} queries {tuple(queries.shape)}")
    if not corpus.is_contiguous() or not queries.is_contiguous():
        raise ValueError("corpus and queries must be contiguous row-major")
    n, d = corpus.shape
    q = queries.shape[0]
    dev = corpus.device
    n_seg = 1 if seg_offsets is None else len(seg_offsets) - 1
    shape = (q, k) if seg_offsets is None else (q, n_seg, k)
    if _packed is not None:
        out_s = _packed[: q * n_seg * k].view(torch.float32).view(shape)
        out_i = _packed[q * n_seg * k: 2 * q * n_seg * k].view(shape)
    else:
        out_s = torch.empty(shape, dtype=torch.float32, device=dev)
        out_i = torch.empty(shape, dtype=torch.int32, device=dev)
    if q == 0:
        return out_s, out_i
    c_offs = (ctypes.c_int64 * (n_seg + 1))(*[int(o) for o in seg_offsets]) if seg_offsets is not None else None
    with torch.cuda.device(dev):
        st = _stream_ptr(dev)
        need = lib.tt_scan_topk_rows_workspace_bytes(int(max_rows), d, q, k)
        ws = _ws.get(dev, need + 256)
        base = (ws.data_ptr() + 255) // 256 * 256
        if _packed is not None:
            flag = _packed[2 * q * n_seg * k:]
            flag.zero_()
        else:
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = lib.tt_scan_topk_rows(corpus.data_ptr(), n, d, queries.data_ptr(), q, k, rows.data_ptr(), list_offsets.data_ptr(),
                                   int(max_rows), c_offs, n_seg, idx_base, out_s.data_ptr(), out_i.data_ptr(), base,
                                   ws.numel() - (base - ws.data_ptr()), flag.data_ptr(), st)
        _lib.check(rc, "tt_scan_topk_rows")
        if _packed is not None:
            return out_s, out_i
        if return_flag:
            return out_s, out_i, int(flag.item())
        if check_overflow and int(flag.item()) != 0:
            return scan_topk_rows_exact(corpus, queries, k, rows, list_offsets, seg_offsets, idx_base)
    return out_s, out_i


def scan_topk_rows_exact(corpus, queries, k, rows, list_offsets, seg_offsets=None, idx_base: int = 0):
    """The fallback of ``scan_topk_rows``: the dense exact path over ``index_select``ed rows, per segment (one host sync)."""
    offs = list_offsets.cpu().tolist()
    n_seg = len(offs) - 1
    q = queries.shape[0]
    s_out = torch.full((q, n_seg, k), float("-inf"), dtype=torch.float32, device=corpus.device)
    i_out = torch.full((q, n_seg, k), -1, dtype=torch.int32, device=corpus.device)
    for s in range(n_seg):
        sub = rows[offs[s]:offs[s + 1]].long()
        if sub.numel() == 0:
            continue
        es, ei = scan_topk(corpus.index_select(0, sub).contiguous(), queries, k, exact_dense=True)
        add = idx_base if seg_offsets is None else -int(seg_offsets[s])
        mapped = torch.where(ei >= 0, sub[ei.clamp_min(0).long()].to(torch.int32) + add, ei)
        s_out[:, s], i_out[:, s] = es, mapped
    if seg_offsets is None:
        return s_out[:, 0].contiguous(), i_out[:, 0].contiguous()
    return s_out, i_out


def scan_topk_rows_host(corpus, queries, k, rows, list_offsets, max_rows: int, seg_offsets=None, idx_base: int = 0):
    """``scan_topk_rows`` with the hits on the host: scores, indices and the status word come back in ONE copy (one sync), as
    ``scan_topk_host``; a flagged overflow re-runs the dense exact path over the gathered rows.  -> CPU tensors."""
    q = queries.shape[0]
    n_seg = 1 if seg_offsets is None else len(seg_offsets) - 1
    shape = (q, k) if seg_offsets is None else (q, n_seg, k)
    if q == 0:
        return torch.empty(shape, dtype=torch.float32), torch.empty(shape, dtype=torch.int32)
    m = q * n_seg * k
    packed = torch.empty(2 * m + 1, dtype=torch.int32, device=corpus.device)
    scan_topk_rows(corpus, queries, k, rows, list_offsets, max_rows, seg_offsets, idx_base, _packed=packed)
    host = packed.cpu()
    if int(host[-1]) != 0:
        s, i = scan_topk_rows_exact(corpus, queries, k, rows, list_offsets, seg_offsets, idx_base)
        return s.cpu(), i.cpu()
    return host[:m].view(torch.float32).view(shape), host[m: 2 * m].view(shape)


def topk_merge(scores: torch.Tensor, idx: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge candidate lists [Q, M] (fp32 scores, int32 global indices, idx<0 =
    padding) into the top-k by (score desc, idx asc)."""
    lib = _lib.load_library()
    _require_cuda(scores, "scores")
    _require_cuda(idx, "idx")
    if scores.dtype != torch.float32 or idx.dtype != torch.int32:
        raise TypeError("scores must be float32 and idx int32")
    if scores.shape != idx.shape or scores.dim() != 2:
        raise ValueError("scores/idx must both be [Q, M]")
    scores = scores.contiguous()
    idx = idx.contiguous()
    q, m = scores.shape
    dev = scores.device
    out_s = torch.empty((q, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((q, k), dtype=torch.int32, device=dev)
    if q == 0:
        return out_s, out_i
    with torch.cuda.device(dev):
        rc = lib.tt_topk_merge(scores.data_ptr(), idx.data_ptr(), q, m, k, out_s.data_ptr(), out_i.data_ptr(),
                               _stream_ptr(dev))
        _lib.check(rc, "tt_topk_merge")
    return out_s, out_i


def similarity_from_cosine(cos: torch.Tensor) -> torch.Tensor:
    """Reference score mapping for NodeWithScore.score: ChromaVectorStore returns
    exp(-squared_L2) and squared_L2 = 2 - 2 cos for unit vectors."""
    return torch.exp(-(2.0 - 2.0 * cos))
