"""Numpy reference for the device build of posting lists (``tt_postings_build``): what tests/test_postings_gpu.py compares the
kernels with, tested on its own in tests/test_postings_host.py.  Independent of the product module but for the flag values."""
from typing import List

import numpy as np

MAX_DOC_NNZ = 8192        # the scoring kernel's clamp of d_nnz: entries behind it are neither scored nor indexed
FLAG_TERM_RANGE, FLAG_WEIGHT, FLAG_ORDER = 1, 2, 4


def reference_postings(terms, weights, d_start, d_nnz, n_sealed: int, vocab: int):
    """What ``tt_postings_build`` must produce, from host arrays -> (post_off int64 [vocab + 1], lists: one SORTED int32 array of
    document numbers per id, term_ub fp32 [vocab], flags).  Tombstones (``d_nnz`` < 0) contribute nothing, ``d_nnz`` is clamped to
    8192, an id outside [0, vocab) raises bit 0 and is left out, a weight that is negative, NaN or infinite raises bit 1 and takes
    no part in ``term_ub``, a document whose ids are not strictly ascending raises bit 2 (and is listed once per occurrence)."""
    terms, weights = np.asarray(terms, dtype=np.int32), np.asarray(weights, dtype=np.float32)
    d_start, d_nnz = np.asarray(d_start, dtype=np.int64), np.asarray(d_nnz, dtype=np.int32)
    flags = 0
    docs: List[List[int]] = [[] for _ in range(vocab)]
    ub = np.zeros(vocab, dtype=np.float32)
    for doc in range(int(n_sealed)):
        n = int(d_nnz[doc])
        if n < 0:
            continue
        s = int(d_start[doc])
        ids = terms[s:s + min(n, MAX_DOC_NNZ)]
        if (np.diff(ids.astype(np.int64)) <= 0).any():
            flags |= FLAG_ORDER
        for t, w in zip(ids, weights[s:s + min(n, MAX_DOC_NNZ)]):
            if not (w >= 0 and np.isfinite(w)):
                flags |= FLAG_WEIGHT
            if not 0 <= t < vocab:
                flags |= FLAG_TERM_RANGE
                continue
            docs[t].append(doc)
            if w > 0 and np.isfinite(w):
                ub[t] = max(ub[t], w)
    off = np.zeros(vocab + 1, dtype=np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return off, [np.sort(np.asarray(d, dtype=np.int32)) for d in docs], ub, flags
