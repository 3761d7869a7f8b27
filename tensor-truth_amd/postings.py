"""Posting lists for ``LexicalStore`` / ``SpladeStore``: the exact lexical top-k without scoring every document.

``tt_lexical_scan_topk`` scores all ``n_docs`` documents for every query.  A document that shares no id with a query scores exactly
+0 (or is a tombstone), so the documents that can score above zero are those on the posting lists of the query's own ids.  The lists
(``tt_postings_build``) only CHOOSE candidates; ``tt_lexical_topk_postings`` scores them with the scan's own kernel and selects with
the scan's own selection, so a document's score is the same bits on both paths and the order of equal scores (document number
ascending) is the same.  What is left to decide -- here, on the host, in plain numpy -- is when the candidates provably hold the
whole top-k:

* **Unpruned rule.**  With candidates from ALL of a query's ids, every document outside them scores +0 or is dead.  If the k-th best
  candidate score ``thr`` is > 0, no outsider can enter or tie: the result is final.  Otherwise (fewer than k candidates above zero
  -- products that underflow count --, negative weights through the C API) the query is re-run through ``tt_lexical_scan_topk``.
  No assumption about signs is made.
* **Pruned rule (MaxScore, two passes).**  Only when the index is prunable (every stored weight finite and >= 0 and every document's
  ids strictly ascending, so that none repeats: the scoring kernel adds a repeated id once per occurrence), every query weight
  is finite and >= 0, and pass 1 found ``theta = thr > 0``.  With ``c_t = q_w[t] * term_ub[t]``: pass 1 takes the shortest prefix of
  the ids in descending ``c_t`` whose list lengths sum to ``PASS1_FACTOR * k`` (all ids if they never do) and scores those candidates
  with the FULL query, so theta is a real document's real score and a lower bound of the true k-th score.  N is the longest prefix in
  ascending ``c_t`` with ``upper_bound(N) < theta`` strictly: a document holding only ids of N computes at most that bound, so it
  can neither enter the top-k nor tie with its last place.  Pass 2 takes the other ids E -- skipped when pass 1 already took them.

Everything here but ``PostingsIndex``, the two wrappers and ``search`` is host arithmetic and is tested without a device.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_DOC_NNZ = 8192        # the scoring kernel's clamp of d_nnz: entries behind it are neither scored nor indexed
SPAN = 8192               # TT_POSTINGS_SPAN: documents per workgroup of the compaction
PASS1_FACTOR = 2          # pass 1 stops at the first prefix whose lists hold PASS1_FACTOR * k entries
FLAG_TERM_RANGE, FLAG_WEIGHT, FLAG_ORDER = 1, 2, 4   # tt_postings_build's flag word
_U = 2.0 ** -24           # fp32 unit roundoff
_TINY = 2.0 ** -149       # the smallest fp32 subnormal: the absolute error of one rounding where the result is subnormal


# ---- the planner (numpy) -------------------------------------------------------------------------------------------------------------
def term_bounds(q_terms, q_weights, term_ub, vocab: int) -> np.ndarray:
    """``c_t = q_w[t] * term_ub[t]`` in fp64 (the product of two fp32 is exact there); 0 for an id outside the vocabulary."""
    t = np.asarray(q_terms, dtype=np.int64)
    w = np.asarray(q_weights, dtype=np.float32).astype(np.float64)
    inside = (t >= 0) & (t < vocab)
    ub = np.where(inside, np.asarray(term_ub, dtype=np.float32).astype(np.float64)[np.where(inside, t, 0)], 0.0)
    with np.errstate(invalid="ignore"):
        return np.where(inside, w * ub, 0.0)


def list_lengths(q_terms, post_off, vocab: int) -> np.ndarray:
    """The length of every query id's list (0 for an id outside the vocabulary)."""
    t = np.asarray(q_terms, dtype=np.int64)
    inside = (t >= 0) & (t < vocab)
    ts = np.where(inside, t, 0)
    off = np.asarray(post_off, dtype=np.int64)
    return np.where(inside, off[ts + 1] - off[ts], 0).astype(np.int64)


def may_prune(q_weights, prunable: bool) -> bool:
    """The pruned rule's preconditions that are known before pass 1: a prunable index and query weights all finite and >= 0."""
    w = np.asarray(q_weights, dtype=np.float32)
    return bool(prunable) and bool(np.all(np.isfinite(w) & (w >= 0)))


def upper_bound(c: np.ndarray) -> np.float32:
    """B(N): an fp32 number no smaller than anything the scoring kernel can compute for a document that holds only the ids whose
    ``c_t`` are given (all >= 0).  The exact sum, in fp64, times ``1 + 2 (|N| + 6) 2^-24`` -- at most |N| roundings of a lane's fmaf
    chain and six of the butterfly, each relative 2^-24, with the factor 2 over the first-order term paying for the higher orders
    and for fp64's own roundings -- plus ``(|N| + 6) 2^-149`` for roundings that land among the subnormals, where the error is
    absolute; then rounded UP to fp32."""
    c = np.asarray(c, dtype=np.float64)
    n = c.size
    if n == 0:
        return np.float32(0.0)
    b = float(np.sum(c)) * (1.0 + 2.0 * (n + 6) * _U) + (n + 6) * _TINY
    with np.errstate(over="ignore"):
        f = np.float32(b)
    if float(f) < b:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def pass1_prefix(c: np.ndarray, lengths: np.ndarray, k: int) -> np.ndarray:
    """Positions (into the query's entry) of pass 1's ids: the shortest prefix in descending ``c_t`` (equal bounds: entry order)
    whose list lengths sum to at least ``PASS1_FACTOR * k``; every position if they never do."""
    order = np.argsort(-np.asarray(c, dtype=np.float64), kind="stable")
    cum = np.cumsum(np.asarray(lengths, dtype=np.int64)[order])
    hit = np.flatnonzero(cum >= PASS1_FACTOR * int(k))
    return order if hit.size == 0 else order[: int(hit[0]) + 1]


def non_essential(c: np.ndarray, theta: float) -> np.ndarray:
    """Positions of N: the longest prefix in ascending ``c_t`` (equal bounds: entry order) with ``upper_bound(N) < theta``,
    strictly.  Empty unless theta is a number > 0."""
    c = np.asarray(c, dtype=np.float64)
    if not theta > 0 or c.size == 0:
        return np.zeros(0, dtype=np.int64)
    order = np.argsort(c, kind="stable")
    lo, hi = 0, c.size            # upper_bound grows with the prefix (every c_t >= 0): bisect for the longest that fits
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if float(upper_bound(c[order[:mid]])) < float(theta):
            lo = mid
        else:
            hi = mid - 1
    return order[:lo]


def plan_first(q_terms, q_weights, post_off, term_ub, vocab: int, prunable: bool, k: int):
    """-> (positions of pass 1's ids, c, lengths, prune_ok).  Without the pruned rule's preconditions pass 1 takes every id that
    has a list."""
    lengths = list_lengths(q_terms, post_off, vocab)
    ok = may_prune(q_weights, prunable)
    c = term_bounds(q_terms, q_weights, term_ub, vocab) if ok else np.zeros(len(lengths), dtype=np.float64)
    first = pass1_prefix(c, lengths, k) if ok else np.arange(len(lengths), dtype=np.int64)
    return first[lengths[first] > 0], c, lengths, ok


def plan_second(c: np.ndarray, lengths: np.ndarray, first: np.ndarray, theta: float, prune_ok: bool):
    """What follows pass 1's ``theta`` -> ("done", None): pass 1's result is the scan's; ("pass", positions): score these ids'
    lists; ("scan", None): only the full scan can answer."""
    have = set(int(i) for i in first)
    listed = [int(i) for i in np.flatnonzero(np.asarray(lengths) > 0)]
    if not theta > 0:                                  # -inf, or a k-th best of 0 or below: nothing is known about outsiders
        if all(i in have for i in listed):
            return "scan", None
        return "pass", np.asarray(listed, dtype=np.int64)
    if not prune_ok:                                   # pass 1 took every list, and its k-th best beats every outsider's +0
        return "done", None
    n = set(int(i) for i in non_essential(c, theta))
    rest = [i for i in listed if i not in n]
    if all(i in have for i in rest):
        return "done", None
    return "pass", np.asarray(rest, dtype=np.int64)


def ranges_of(q_terms_list: Sequence[np.ndarray], post_off) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """Per query, the ids whose lists to take -> (range_lo int64, range_hi int64, range_start int32 [n_q + 1], the longest sum of
    lengths)."""
    off = np.asarray(post_off, dtype=np.int64)
    start = np.zeros(len(q_terms_list) + 1, dtype=np.int32)
    los, his, longest = [], [], 0
    for q, t in enumerate(q_terms_list):
        t = np.asarray(t, dtype=np.int64)
        los.append(off[t])
        his.append(off[t + 1])
        start[q + 1] = start[q] + len(t)
        longest = max(longest, int((off[t + 1] - off[t]).sum()))
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, dtype=np.int64)   # noqa: E731
    return cat(los), cat(his), start, longest


# ---- device side ----------------------------------------------------------------------------------------------------------------------
class PostingsIndex:
    """The lists of documents [0, n_sealed) in HBM (``post_off`` int64 [vocab + 1], ``post_doc`` int32, ``term_ub`` fp32 [vocab]:
    4 bytes per entry + 12 per vocabulary id) with host copies of ``post_off`` and ``term_ub`` for the planner."""

    def __init__(self, vocab: int, n_sealed: int, post_off, post_doc, term_ub, flags: int):
        self.vocab, self.n_sealed, self.flags = int(vocab), int(n_sealed), int(flags)
        self.post_off, self.post_doc, self.term_ub = post_off, post_doc, term_ub
        self.off_host = post_off.cpu().numpy()
        self.ub_host = term_ub.cpu().numpy()
        self.n_entries = int(self.off_host[-1])
        self.prunable = not (self.flags & (FLAG_WEIGHT | FLAG_ORDER))

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.post_off, self.post_doc, self.term_ub))


def postings_build(d_terms, d_weights, d_start, d_nnz, n_sealed: int, vocab: int, post_cap: int, post_doc=None) -> PostingsIndex:
    """``tt_postings_build`` over documents [0, n_sealed) of device CSR arrays -> ``PostingsIndex``.  ``post_cap``: the entries
    ``post_doc`` holds (the stored entries of those documents, live or dead, are enough).  An id outside [0, vocab) makes the
    library refuse the build with its own message.  ``post_doc``: an int32 device array of at least ``post_cap`` to fill instead
    of a new one."""
    import torch

    from . import _lib
    from ._hostargs import _need_device, _stream

    dev = _need_device("postings_build", d_terms)
    if not 1 <= int(vocab):
        raise ValueError(f"postings_build: vocab={vocab}")
    lib = _lib.load_library()
    post_off = torch.empty(int(vocab) + 1, dtype=torch.int64, device=dev)
    if post_doc is None:
        post_doc = torch.empty(max(int(post_cap), 1), dtype=torch.int32, device=dev)
    elif post_doc.dtype != torch.int32 or post_doc.device != dev or post_doc.numel() < int(post_cap) or not post_doc.is_contiguous():
        raise ValueError(f"postings_build: post_doc must be a contiguous int32 device array of at least {post_cap}")
    term_ub = torch.empty(int(vocab), dtype=torch.float32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(lib.tt_postings_build_workspace_bytes(int(vocab)))
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.tt_postings_build(d_terms.data_ptr(), d_weights.data_ptr(), d_start.data_ptr(), d_nnz.data_ptr(), int(n_sealed),
                                   int(vocab), post_off.data_ptr(), post_doc.data_ptr(), int(post_cap), term_ub.data_ptr(),
                                   flags.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev))
    _lib.check(rc, "tt_postings_build")
    return PostingsIndex(vocab, n_sealed, post_off, post_doc, term_ub, int(flags.item()))


def lexical_topk_postings(q_terms, q_weights, q_start, q_nnz, d_terms, d_weights, d_start, d_nnz, index: PostingsIndex,
                          ranges: Tuple[np.ndarray, np.ndarray, np.ndarray, int], k: int, workspace=None):
    """``tt_lexical_topk_postings`` -> (scores fp32 [n_q][k], document numbers int32 [n_q][k], thr fp32 [n_q], cnt int32 [n_q],
    cand_cnt int32 [n_q]) on the device: ``lexical_scan_topk``'s result restricted to the union of each query's ``ranges`` of
    ``index.post_doc`` and the documents behind ``index.n_sealed``.  ``q_start`` / ``q_nnz``: host arrays; ``d_start`` / ``d_nnz``:
    device arrays of exactly the stored documents."""
    import torch

    from . import _lib
    from ._hostargs import _dev_i, _need_device, _stream
    from .lexical import MAX_QUERY_NNZ, MAX_SCAN_K, MAX_SCAN_QUERIES, _check_entries

    n_q, n_docs = len(q_nnz), len(d_nnz)
    if not 1 <= n_q <= MAX_SCAN_QUERIES:
        raise ValueError(f"lexical_topk_postings: {n_q} queries (1 .. {MAX_SCAN_QUERIES})")
    if not 1 <= int(k) <= MAX_SCAN_K:
        raise ValueError(f"lexical_topk_postings: k={k} (1 .. {MAX_SCAN_K})")
    if not 0 <= index.n_sealed <= n_docs:
        raise ValueError(f"lexical_topk_postings: an index over {index.n_sealed} documents with {n_docs} stored")
    _check_entries("q", q_terms, q_weights, q_start, q_nnz, 0, MAX_QUERY_NNZ)      # what lexical_scan_topk checks
    _check_entries("d", d_terms, d_weights, d_start, d_nnz, -1, MAX_DOC_NNZ)
    lo, hi, start, longest = ranges
    if len(start) != n_q + 1 or len(lo) != int(start[-1]) or len(hi) != len(lo):
        raise ValueError("lexical_topk_postings: range_start [n_q + 1] and one (lo, hi) per range are needed")
    dev = _need_device("lexical_topk_postings", d_terms)
    qs, qn = _dev_i(q_start, torch.int32, dev), _dev_i(q_nnz, torch.int32, dev)
    lo_t = torch.from_numpy(np.ascontiguousarray(np.append(lo, 0), dtype=np.int64)).to(dev)      # (never empty: a valid pointer)
    hi_t = torch.from_numpy(np.ascontiguousarray(np.append(hi, 0), dtype=np.int64)).to(dev)
    st_t = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int32)).to(dev)
    lib = _lib.load_library()
    need = int(lib.tt_lexical_topk_postings_workspace_bytes(n_docs, index.n_sealed, n_q))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    scores = torch.empty((n_q, int(k)), dtype=torch.float32, device=dev)
    idx = torch.empty((n_q, int(k)), dtype=torch.int32, device=dev)
    thr = torch.empty((n_q,), dtype=torch.float32, device=dev)
    cnt = torch.empty((n_q,), dtype=torch.int32, device=dev)
    cand_cnt = torch.empty((n_q,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.tt_lexical_topk_postings(q_terms.data_ptr(), q_weights.data_ptr(), qs.data_ptr(), qn.data_ptr(), n_q,
                                          d_terms.data_ptr(), d_weights.data_ptr(), d_start.data_ptr(), d_nnz.data_ptr(), n_docs,
                                          index.post_doc.data_ptr(), index.n_entries, index.n_sealed, lo_t.data_ptr(),
                                          hi_t.data_ptr(), st_t.data_ptr(), int(longest), int(k), scores.data_ptr(), idx.data_ptr(),
                                          thr.data_ptr(), cnt.data_ptr(), cand_cnt.data_ptr(), workspace.data_ptr(),
                                          workspace.numel() * workspace.element_size(), _stream(dev))
    _lib.check(rc, "tt_lexical_topk_postings")
    return scores, idx, thr, cnt, cand_cnt, workspace


def search(store, lexical, k: int):
    """``LexicalStore.search`` through ``store.index`` -> (scores, document numbers) equal to the full scan's, bit for bit and
    index for index, and the search's figures in ``store.stats``.  One readback of the queries' entries before pass 1 and one of
    ``thr`` after each pass."""
    import torch

    from . import _lib
    from .lexical import MAX_QUERY_NNZ, _check_entries, lexical_scan_topk

    ix: PostingsIndex = store.index
    n_q, n_docs = len(lexical), store.n_docs
    q_start = store._check_query(lexical)
    q_nnz = np.ascontiguousarray(lexical.nnz, dtype=np.int32)
    _check_entries("q", lexical.terms, lexical.weights, q_start, q_nnz, 0, MAX_QUERY_NNZ)      # before anything is sliced or launched
    qt_h, qw_h = lexical.terms.cpu().numpy(), lexical.weights.cpu().numpy()
    d_start, d_nnz = store.d_start[:n_docs], store.d_nnz[:n_docs]
    entries = [(qt_h[s:s + n], qw_h[s:s + n]) for s, n in zip(q_start, q_nnz)]
    plans = [plan_first(t, w, ix.off_host, ix.ub_host, ix.vocab, ix.prunable, k) for t, w in entries]

    def run(which: List[int], positions: List[np.ndarray]):
        rg = ranges_of([entries[q][0][p] for q, p in zip(which, positions)], ix.off_host)
        s, i, thr, _, cc, store._pws = lexical_topk_postings(lexical.terms, lexical.weights, q_start[which], q_nnz[which], store.terms,
                                                            store.weights, d_start, d_nnz, ix, rg, k, workspace=store._pws)
        back = torch.stack((thr.view(torch.int32), cc)).cpu().numpy()      # one readback: the thresholds' bits and the counts
        return s, i, back[0].view(np.float32), back[1].astype(np.int64)

    everyone = list(range(n_q))
    scores, idx, theta, cand = run(everyone, [p[0] for p in plans])
    candidates, passes = int(cand.sum()), 1
    again, again_pos, scan = [], [], []
    for q, (first, c, lengths, ok) in enumerate(plans):
        what, pos = plan_second(c, lengths, first, float(theta[q]), ok)
        if what == "pass":
            again.append(q)
            again_pos.append(pos)
        elif what == "scan":
            scan.append(q)
    if again:
        s2, i2, theta2, cand2 = run(again, again_pos)
        rows = torch.as_tensor(again, device=scores.device)
        scores[rows], idx[rows] = s2, i2
        candidates, passes = candidates + int(cand2.sum()), 2
        scan += [q for q, t in zip(again, theta2) if not t > 0]
    if scan:
        scan.sort()
        need = int(_lib.load_library().tt_lexical_scan_workspace_bytes(n_docs, len(scan)))
        if store._ws is None or store._ws.numel() < need:
            store._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=scores.device)
        s3, i3 = lexical_scan_topk(lexical.terms, lexical.weights, q_start[scan], q_nnz[scan], store.terms, store.weights, d_start,
                                   d_nnz, k, workspace=store._ws)
        rows = torch.as_tensor(scan, device=scores.device)
        scores[rows], idx[rows] = s3, i3
    store.stats = {"queries": n_q, "candidates": candidates, "documents": n_docs, "passes": passes, "fallbacks": len(scan),
                   "sealed": ix.n_sealed}
    return scores, idx
