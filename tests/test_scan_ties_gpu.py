"""GPU: every scan surface at k > 64 on a corpus where ties are the rule, exact on scores AND indices for every query.

The integer family: corpus and query entries drawn uniformly from {-2, ..., 2}, stored as bf16.  Every product is an integer of
magnitude <= 4 and every dot product an integer of magnitude <= 4 * 1024 < 2^24: exact in fp32 in any summation order and on any
MFMA shape, so the fp64 oracle (``Q.double() @ C.double().T`` on the device, stable descending sort: score descending, row
ascending) is the ONE right answer -- no tie-free exemption, no score tolerance, ``torch.equal`` on both outputs.  With a standard
deviation of sqrt(4 d) the scores near the k-th place share their value with tens of rows: each test recomputes, from its own
oracle, the share of queries whose k-th and (k + 1)-th scores are equal and requires it to be at least one half.

About 1 % of the rows are NaN tombstones, some of them the lowest rows of the tie class that holds a query's k-th place; a
tombstoned row must never come back.  Shapes are the smallest that reach each path of ``make_plan`` (csrc/scan_api.hip): dense
when n <= 8192 or n < 128 k; the tiled filter when q > 64, n >= 262144 and n >= 2048 k; the sampled threshold with the streaming
filter otherwise.  Status flag: a call that returns 0 must itself be exact; one that returns non-zero must be exact through the
wrapper's dense fallback; the named cases of the sampled and of the tiled path must return 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

IDX_BASE = 7_000_000


def _is_dense(n, k):
    return n <= 8192 or n < 128 * k


def _is_tiled(n, q, k):
    return q > 64 and n >= 262144 and n >= 2048 * k and not _is_dense(n, k)


class _Family:
    """corpus [n, d] and queries [q, d] of the integer family on the device, tombstones written, fp64 scores kept."""

    def __init__(self, dev, n, d, q, k, seed, span=2, query_columns=None):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.n, self.d, self.q, self.k = n, d, q, k
        self.corpus = torch.randint(-span, span + 1, (n, d), generator=g, device=dev).to(torch.bfloat16)
        self.queries = torch.randint(-span, span + 1, (q, d), generator=g, device=dev).to(torch.bfloat16).contiguous()
        if query_columns:       # +-2 in a few columns, 0 elsewhere: a handful of score levels, the best one n / 5^columns rows wide
            keep = torch.rand((q, d), generator=g, device=dev).argsort(1)[:, :query_columns]
            sign = torch.randint(0, 2, (q, query_columns), generator=g, device=dev) * 4 - 2
            self.queries = torch.zeros_like(self.queries).scatter_(1, keep, sign.to(torch.bfloat16)).contiguous()
        self.scores = self.queries.double() @ self.corpus.double().T          # [q, n] fp64: exact integers
        assert float(self.scores.abs().max()) < 2 ** 24
        dead = torch.rand((n,), generator=g, device=dev) < 0.01
        # ... and, for the first queries, the three lowest rows of the tie class that holds the k-th place, and the best row
        self.in_class = 0
        if n > k + 8:
            for t in range(min(q, 2)):
                live = self.scores[t].masked_fill(dead, float("-inf"))
                level = torch.topk(live, k).values[-1]
                rows = torch.nonzero(live == level).flatten()[:3]
                dead[rows] = True
                self.in_class += int(rows.numel())
            dead[torch.argmax(self.scores[0].masked_fill(dead, float("-inf")))] = True
        self.dead = dead
        self.corpus[dead] = float("nan")
        self.corpus = self.corpus.contiguous()
        self.scores[:, dead] = float("-inf")


def _expect(scores, k):
    """fp64 scores [q, rows] (-inf = tombstoned) -> (scores [q, k] fp32, rows [q, k] int64 with -1 padding, [q] bool: the k-th and
    (k + 1)-th scores are equal, [q] rows at the k-th level)."""
    q, rows = scores.shape
    kk = min(k, rows)
    want_s = torch.full((q, k), float("-inf"), dtype=torch.float32, device=scores.device)
    want_i = torch.full((q, k), -1, dtype=torch.int64, device=scores.device)
    tied = torch.zeros(q, dtype=torch.bool, device=scores.device)
    size = torch.zeros(q, dtype=torch.int64, device=scores.device)
    if kk:
        vals, order = torch.sort(scores, dim=1, descending=True, stable=True)
        want_s[:, :kk] = vals[:, :kk].float()
        want_i[:, :kk] = torch.where(torch.isfinite(vals[:, :kk]), order[:, :kk], torch.full_like(order[:, :kk], -1))
        if rows > k:
            tied = (vals[:, k - 1] == vals[:, k]) & torch.isfinite(vals[:, k])
            size = (scores == vals[:, k - 1:k]).sum(1)
    return want_s, want_i, tied, size


def _levels(want_s):
    return [int(torch.unique(r[torch.isfinite(r)]).numel()) for r in want_s]


def _report(tag, fam_or_none, want_s, tied, size, flag):
    share = float(tied.float().mean())
    lv = _levels(want_s)
    print(f"\n{tag}: flag {flag}; k-th == (k+1)-th score on {share:.2f} of the queries, {int(size.min())}-{int(size.max())} rows at the "
          f"k-th level, {min(lv)}-{max(lv)} score levels inside the top k"
          + (f", {int(fam_or_none.dead.sum())} tombstones ({fam_or_none.in_class} in a winning tie class)" if fam_or_none else ""))
    return share


def _assert_exact(got_s, got_i, want_s, want_i, tag):
    wrong_i = int((got_i.long() != want_i).any(1).sum())
    wrong_s = int((got_s != want_s).any(1).sum())
    print(f"  {tag}: queries with a wrong index {wrong_i}, with a wrong score {wrong_s}, of {want_i.shape[0]}")
    assert torch.equal(got_i.long(), want_i), (tag, "indices")
    assert torch.equal(got_s, want_s), (tag, "scores")


def _scan_case(dev, n, d, q, k, must_clear=False, seed=None, **family):
    from tensor_truth_amd import scan as tscan

    fam = _Family(dev, n, d, q, k, seed=n + d + q + k if seed is None else seed, **family)
    want_s, want_i, tied, size = _expect(fam.scores, k)
    want_i = torch.where(want_i >= 0, want_i + IDX_BASE, want_i)
    s, i, flag = tscan.scan_topk(fam.corpus, fam.queries, k, idx_base=IDX_BASE, return_flag=True)
    torch.cuda.synchronize()
    tag = f"scan {n} x {d}, {q} queries, k {k}"
    share = _report(tag, fam, want_s, tied, size, flag)
    assert share >= 0.5 and fam.in_class > 0
    if flag != 0:
        assert not must_clear, (tag, "the status flag is raised: this case has to finish on its own path")
        s, i = tscan.scan_topk(fam.corpus, fam.queries, k, idx_base=IDX_BASE)        # the wrapper's dense fallback
        torch.cuda.synchronize()
    dead_rows = torch.nonzero(fam.dead).flatten() + IDX_BASE
    assert not torch.isin(i.long(), dead_rows).any(), (tag, "a tombstoned row came back")
    _assert_exact(s, i, want_s, want_i, tag + (" (fallback)" if flag else ""))
    return fam, want_s, want_i


@pytest.mark.parametrize("n,d,q,k", [(8192, 128, 8, 65), (16383, 128, 8, 128), (131071, 128, 4, 1024)])
def test_dense_path(dev, built_lib, n, d, q, k):
    """Every score written, select_kernel over the n dense scores with implicit indices: 8192 = room + 128 at k = 65 (two flushes),
    two chunks at k = 128, nineteen chunks of 7168 at kpad = 1024."""
    assert _is_dense(n, k)
    _scan_case(dev, n, d, q, k, must_clear=True)


@pytest.mark.parametrize("n,d,q,k,must_clear", [
    (8320, 128, 8, 65, False), (16384, 128, 8, 128, True), (70000, 384, 8, 129, False), (131072, 128, 4, 1024, False),
    (70000, 1024, 4, 256, False),
])
def test_sampled_threshold_streaming_filter(dev, built_lib, n, d, q, k, must_clear):
    """The first n past each dense bound: the threshold is select_kernel's unfused ``thr_out`` (only k > 64 takes it), a score
    level that tens of rows share -- the filter has to let the whole class through --, and the final selection reads the
    lane-private sub-lists (source 2) and the shared list."""
    assert not _is_dense(n, k) and not _is_tiled(n, q, k)
    _scan_case(dev, n, d, q, k, must_clear=must_clear)


@pytest.mark.parametrize("k", [128, 1024])
def test_a_tie_class_wider_than_an_lds_chunk(dev, built_lib, k):
    """Queries with two non-zero entries: nine score levels, the best one about n / 25 = 10 000 rows wide and the sampled
    threshold itself.  More private candidates than one LDS chunk holds arrive in ONE round of sub-lists (select_kernel's
    sub-list-by-sub-list staging with a flush in between), the prefilter's threshold falls inside the class, and the answer is
    the k lowest live rows of the class -- with the status flag clear."""
    n, d, q = 262_143, 128, 4
    fam, want_s, want_i = _scan_case(dev, n, d, q, k, must_clear=True, query_columns=2)
    width = (fam.scores == want_s[:, k - 1:k].double()).sum(1)
    print(f"  the k-th level holds {int(width.min())}-{int(width.max())} rows")
    assert int(width.min()) > 8192 and (want_s == want_s[:, :1]).all()


@pytest.mark.parametrize("n,d,q,k,must_clear", [(262144, 128, 65, 128, True), (262144 + 231, 128, 70, 100, False)])
def test_tiled_filter(dev, built_lib, n, d, q, k, must_clear):
    """65+ queries: sample on the contraction, ``thr_out`` + ``relax_thr_kernel`` (an integer threshold lowered by a fraction must
    not reach the next level down, and must keep its own), every survivor through the shared list, ``min_valid`` armed; the
    ragged shard's last tile overlaps its predecessor."""
    assert _is_tiled(n, q, k)
    _scan_case(dev, n, d, q, k, must_clear=must_clear)


@pytest.mark.parametrize("n,q", [(140_000, 3), (262_144, 65)])
def test_one_tie_class_overflows_the_lists_and_says_so(dev, built_lib, n, q):
    """Every live row is the same row: the sampled threshold IS the one score, the filter lets the whole class through, and no
    candidate list holds it -- select_kernel (k = 128: the LDS network's ``cnt > cap`` branch) has to raise the status flag, on the
    streaming and on the tiled path; the wrapper's fallback then returns the k lowest live rows."""
    from tensor_truth_amd import scan as tscan

    d, k = 128, 128
    assert not _is_dense(n, k) and _is_tiled(n, q, k) == (q > 64)
    g = torch.Generator(device=dev).manual_seed(n + q)
    row = torch.randint(-2, 3, (1, d), generator=g, device=dev).to(torch.bfloat16)
    corpus = row.repeat(n, 1)
    dead = torch.rand((n,), generator=g, device=dev) < 0.01
    dead[:3] = True
    corpus[dead] = float("nan")
    queries = torch.randint(-2, 3, (q, d), generator=g, device=dev).to(torch.bfloat16)
    queries[0] = row[0]
    scores = (queries.double() @ row.double().T).repeat(1, n)
    scores[:, dead] = float("-inf")
    want_s, want_i, tied, size = _expect(scores, k)
    _, _, flag = tscan.scan_topk(corpus, queries, k, idx_base=IDX_BASE, return_flag=True)
    print(f"\none class of {int(size.min())} rows, {q} queries over {n} rows, k {k}: flag {flag}")
    assert tied.all() and flag != 0
    s, i = tscan.scan_topk(corpus, queries, k, idx_base=IDX_BASE)
    torch.cuda.synchronize()
    _assert_exact(s, i, want_s, want_i + IDX_BASE, "one tie class (fallback)")


def test_segmented_scan(dev, built_lib):
    """``tt_scan_topk_segmented`` at k = 100: six modules -- an empty one, one shorter than k, one longer than a 65536-row piece
    (cut in two, merged by a second select_kernel launch in segmented mode) -- module-local rows, padding where a module runs out."""
    from tensor_truth_amd import scan as tscan

    k, q, d = 100, 4, 128
    offsets = [5, 5, 60, 3000, 70000, 78000, 90000]
    fam = _Family(dev, offsets[-1] + 17, d, q, k, seed=99)
    s, i = tscan.scan_topk_segmented(fam.corpus, fam.queries, k, offsets)
    torch.cuda.synchronize()
    assert s.shape == (q, len(offsets) - 1, k)
    all_tied = []
    for m in range(len(offsets) - 1):
        lo, hi = offsets[m], offsets[m + 1]
        want_s, want_i, tied, size = _expect(fam.scores[:, lo:hi], k)
        if hi - lo > k:
            _report(f"module {m}: rows [{lo}, {hi})", fam if m == 3 else None, want_s, tied, size, "-")
            all_tied.append(tied)
        _assert_exact(s[:, m], i[:, m], want_s, want_i, f"segmented, module {m} of {hi - lo} rows")
        local_dead = torch.nonzero(fam.dead[lo:hi]).flatten()
        assert not torch.isin(i[:, m].long(), local_dead).any()
    share = float(torch.cat(all_tied).float().mean())
    print(f"  k-th == (k+1)-th score on {share:.2f} of the (query, module) pairs with more than k rows")
    assert share >= 0.5


def test_row_list_scan(dev, built_lib):
    """``tt_scan_topk_rows`` at k = 128 over a filter list at pass rate 0.5: one list of ~40000 rows (sampled path over the list)
    with an index base, then the same list cut into two segments (~15000 listed rows: dense; ~25000: sampled) whose outputs are
    written with stride 2 k -- select_kernel's ``out_stride`` -- as segment-local rows."""
    from tensor_truth_amd import scan as tscan

    n, d, q, k = 80_000, 128, 8, 128
    fam = _Family(dev, n, d, q, k, seed=5)
    g = torch.Generator(device=dev).manual_seed(6)
    rows = torch.nonzero(torch.rand((n,), generator=g, device=dev) < 0.5).flatten()
    rows32 = rows.to(torch.int32).contiguous()
    cnt = int(rows.numel())
    assert not _is_dense(cnt, k)

    def run(offs, bound, **kw):
        s, i, flag = tscan.scan_topk_rows(fam.corpus, fam.queries, k, rows32, offs, bound, return_flag=True, **kw)
        if flag != 0:
            s, i = tscan.scan_topk_rows(fam.corpus, fam.queries, k, rows32, offs, bound, **kw)
        torch.cuda.synchronize()
        return s, i, flag

    offs = torch.tensor([0, cnt], dtype=torch.int32, device=dev)
    s, i, flag = run(offs, cnt, idx_base=IDX_BASE)
    want_s, pos, tied, size = _expect(fam.scores[:, rows], k)
    assert _report(f"row list of {cnt} of {n} rows, k {k}", fam, want_s, tied, size, flag) >= 0.5
    _assert_exact(s, i, want_s, rows[pos] + IDX_BASE, "row list")
    assert not torch.isin(i.long() - IDX_BASE, torch.nonzero(fam.dead).flatten()).any()

    seg = [0, 30_000, n]
    seg_offs = torch.searchsorted(rows, torch.tensor(seg, device=dev)).to(torch.int32)
    per = (seg_offs[1:] - seg_offs[:-1]).tolist()
    assert _is_dense(per[0], k) and not _is_dense(per[1], k)
    s, i, flag = run(seg_offs, max(per), seg_offsets=seg)
    assert s.shape == (q, 2, k)
    for m in range(2):
        part = rows[int(seg_offs[m]):int(seg_offs[m + 1])]
        want_s, pos, tied, size = _expect(fam.scores[:, part], k)
        assert _report(f"segment {m}: {per[m]} listed rows", None, want_s, tied, size, flag) >= 0.5
        _assert_exact(s[:, m], i[:, m], want_s, part[pos] - seg[m], f"row list, segment {m}")


def test_shadow_scan(dev, built_lib, monkeypatch):
    """``tt_scan_topk_shadow``, 2 queries at k = 128: its threshold is select_kernel's ``thr_out`` again, its final selection
    reads (score, row) pairs from the survivor table.  (+-2 saturates the e4m3 shadow: the per-row bound covers it.)"""
    from tensor_truth_amd import scan as tscan

    n, d, q, k = 32_768, 128, 2, 128
    monkeypatch.setattr(tscan.ScanShadow, "MIN_ROWS", 8193)
    fam = _Family(dev, n, d, q, k, seed=41)
    sh = tscan.ScanShadow(fam.corpus)
    assert sh.serves(n, q, k), "the call below would not take the shadow path"
    want_s, want_i, tied, size = _expect(fam.scores, k)
    s, i, flag = tscan.scan_topk(fam.corpus, fam.queries, k, idx_base=IDX_BASE, return_flag=True, shadow=sh)
    torch.cuda.synchronize()
    assert _report(f"shadow scan {n} x {d}, k {k}", fam, want_s, tied, size, flag) >= 0.5
    if flag != 0:
        s, i = tscan.scan_topk(fam.corpus, fam.queries, k, idx_base=IDX_BASE, shadow=sh)
        torch.cuda.synchronize()
    _assert_exact(s, i, want_s, want_i + IDX_BASE, "shadow scan")


def test_mmr_over_a_1024_long_tied_list(dev, built_lib):
    """The MMR prefetch: ``scan_topk(k = 1024)`` feeds ``mmr_select``, whose rule "ties go to the LOWER position" makes the order
    of the list decide the picks.  With lambda = 1 the picks are the list's own order: the oracle's first 200, in order."""
    from tensor_truth_amd import scan as tscan

    fam, want_s, want_i = _scan_case(dev, 131_072, 128, 2, 1024, seed=23)
    cand_s, cand_i = tscan.scan_topk(fam.corpus, fam.queries, 1024, idx_base=IDX_BASE)
    mmr, rel, idx, pos = tscan.mmr_select(fam.corpus, cand_i, cand_s, 200, 1.0, idx_base=IDX_BASE)
    torch.cuda.synchronize()
    levels = _levels(want_s[:, :200])
    print(f"  mmr lambda 1, 200 of 1024: {min(levels)}-{max(levels)} score levels among the picks; picks off the oracle's order: "
          f"{int((idx.long() != want_i[:, :200]).sum())}")
    assert torch.equal(idx.long(), want_i[:, :200])
    assert torch.equal(pos.long(), torch.arange(200, device=dev).repeat(2, 1))
    assert torch.equal(rel, want_s[:, :200]) and torch.equal(mmr, want_s[:, :200])
