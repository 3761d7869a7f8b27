"""GPU: tt_mmr_select on the entry point (include/tt_hip.h, csrc/mmr.hip) -- the pairwise similarities against fp64, their bits
(symmetry, independence of list position / list length / batch), the greedy selection against its numpy.float32 restatement
(tests/mmr_refs.py) bit for bit, a constructed near-duplicate case through the real scan, and every refusal."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import mmr_refs as mr
import tensor_truth_amd  # noqa: F401
from tensor_truth_amd import _lib
from tensor_truth_amd import scan as tscan

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N_ROWS = 4096
ZERO_ROW = 77
DUPS = [(10, 2000), (11, 2001), (500, 501)]           # (row, its exact copy)
UNSUPPORTED, INVALID, WORKSPACE = -2, -1, -3


@functools.lru_cache(maxsize=None)
def _corpus(dim):
    """4096 random unit rows in bf16 with a few exact duplicates and one all-zero row (shared by the tests, never modified)."""
    g = torch.Generator().manual_seed(1000 + dim)
    c = torch.randn(N_ROWS, dim, generator=g)
    c = (c / c.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    for a, b in DUPS:
        c[b] = c[a]
    c[ZERO_ROW] = 0
    return c.to(DEV).contiguous()


def _ppad(p):
    return (p + 15) // 16 * 16


def _call(corpus, cand, rel, k, lam=0.5, penalty=0, idx_base=0, n_rows=None):
    """One tt_mmr_select with its own workspace -> (mmr, rel, idx, pos) [Q, k] numpy and G [Q, Ppad, Ppad] fp32 numpy."""
    lib = _lib.load_library()
    cand = torch.as_tensor(np.asarray(cand, dtype=np.int32)).reshape(-1, np.asarray(cand).shape[-1]).to(DEV).contiguous()
    rel = torch.as_tensor(np.asarray(rel, dtype=np.float32)).reshape(cand.shape).to(DEV).contiguous()
    q, p = cand.shape
    need = lib.tt_mmr_workspace_bytes(q, p)
    assert need == q * _ppad(p) ** 2 * 4
    ws = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=DEV)
    outs = [torch.empty((q, k), dtype=dt, device=DEV) for dt in (torch.float32, torch.float32, torch.int32, torch.int32)]
    rc = lib.tt_mmr_select(corpus.data_ptr(), corpus.shape[0] if n_rows is None else n_rows, corpus.shape[1], cand.data_ptr(),
                           rel.data_ptr(), q, p, k, float(lam), int(penalty), idx_base, *[o.data_ptr() for o in outs],
                           ws.data_ptr(), need, torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(rc, "tt_mmr_select")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], ws.view(q, _ppad(p), _ppad(p)).cpu().numpy()


def _list(p, seed, n_pad=0):
    """A candidate list of p positions: distinct random rows, among them (where p allows) a duplicated pair and the zero row; the
    last n_pad entries are padding.  Scores descend, with a tie at the front."""
    rng = np.random.default_rng(seed)
    rows = rng.permutation(N_ROWS)[:p].astype(np.int64)
    special = [DUPS[0][0], DUPS[0][1], ZERO_ROW]
    rows = np.array([r for r in rows if r not in special], dtype=np.int64)[: max(p - 3, 0)]
    rows = np.concatenate([rows, np.array(special[: p - len(rows)], dtype=np.int64)])
    rows = rows[rng.permutation(len(rows))][:p]
    assert len(rows) == p and len(set(rows.tolist())) == p
    rel = np.sort(rng.uniform(0.2, 0.9, size=p).astype(np.float32))[::-1].copy()
    if p > 1:
        rel[1] = rel[0]
    if n_pad:
        rows[p - n_pad:] = -1
        rel[p - n_pad:] = -np.inf
    return rows.astype(np.int32), rel


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


# ---- 1. G against fp64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [128, 384, 1024])
@pytest.mark.parametrize("p", [1, 15, 16, 17, 33, 200, 1024])
def test_gram_within_the_fp32_accumulation_bound(dim, p):
    corpus = _corpus(dim)
    cand, rel = _list(p, seed=p, n_pad=2 if p >= 15 else 0)
    _, G = _call(corpus, cand, rel, 1)
    g64, bound, valid = mr.gram_fp64(corpus, cand)
    pair = valid[:, None] & valid[None, :]
    err = np.abs(G[0, :p, :p].astype(np.float64) - g64)
    assert np.isfinite(G[0, :p, :p][pair]).all()
    nz = pair & (bound > 0)
    ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    print(f"dim {dim} P {p}: max |G - G64| / bound = {ratio:.3f} over {int(pair.sum())} pairs")
    assert (err[pair] <= bound[pair]).all()                     # (the zero row: bound 0, and G is exactly 0)
    assert (G[0][~np.pad(pair, (0, _ppad(p) - p))] == 0).all()  # entries with a padding position: +0


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [128, 1024])
def test_gram_bits_depend_on_the_two_rows_alone(dim):
    corpus = _corpus(dim)
    cand, rel = _list(200, seed=5)
    _, G = _call(corpus, cand, rel, 1)
    g = _i32(G[0, :200, :200])
    assert np.array_equal(g, g.T)                               # one value written twice
    # the duplicated rows: equal rows, equal entries
    i, j = int(np.flatnonzero(cand == DUPS[0][0])[0]), int(np.flatnonzero(cand == DUPS[0][1])[0])
    assert np.array_equal(g[i], g[j]) and g[i, j] == g[i, i] == g[j, j]
    # permuted list
    perm = np.random.default_rng(6).permutation(200)
    _, G2 = _call(corpus, cand[perm], rel, 1)
    assert np.array_equal(_i32(G2[0, :200, :200]), g[np.ix_(perm, perm)])
    # P grows from 17 to 200 with the same 17 in front
    _, G17 = _call(corpus, cand[:17], rel[:17], 1)
    assert np.array_equal(_i32(G17[0, :17, :17]), g[:17, :17])
    # alone, first of 3, last of 64
    others, orel = zip(*[_list(200, seed=100 + s) for s in range(63)])
    _, G3 = _call(corpus, np.stack([cand, others[0], others[1]]), np.stack([rel, orel[0], orel[1]]), 1)
    assert np.array_equal(_i32(G3[0, :200, :200]), g)
    _, G64 = _call(corpus, np.stack(list(others) + [cand]), np.stack(list(orel) + [rel]), 1)
    assert np.array_equal(_i32(G64[63, :200, :200]), g)
    assert np.array_equal(_i32(G64[0, :200, :200]), _i32(G3[1, :200, :200]))


# ---- 3. selection ----------------------------------------------------------------------------------------------------------------
def _check_selection(corpus, cand, rel, k, lam, penalty, **kw):
    """All four outputs equal greedy_f32 fed the device's own G and rel, bit for bit; returns them."""
    cand, rel = np.atleast_2d(cand), np.atleast_2d(rel)
    (o_mmr, o_rel, o_idx, o_pos), G = _call(corpus, cand, rel, k, lam, penalty, **kw)
    n_rows, base = kw.get("n_rows", corpus.shape[0]), kw.get("idx_base", 0)
    p = cand.shape[1]
    for q in range(cand.shape[0]):
        row = cand[q].astype(np.int64) - base
        valid = (cand[q] >= 0) & (row >= 0) & (row < n_rows)
        w_mmr, w_rel, w_pos = mr.greedy_f32(rel[q], G[q, :p, :p], k, lam, penalty, valid=valid)
        w_idx = np.where(w_pos >= 0, cand[q][np.maximum(w_pos, 0)], -1).astype(np.int32)
        what = f"q {q} P {p} k {k} lambda {lam} penalty {penalty}"
        assert np.array_equal(o_pos[q], w_pos), what
        assert np.array_equal(o_idx[q], w_idx), what
        assert np.array_equal(_i32(o_mmr[q]), _i32(w_mmr)), what
        assert np.array_equal(_i32(o_rel[q]), _i32(w_rel)), what
    return o_mmr, o_rel, o_idx, o_pos


@pytest.mark.parametrize("penalty", [0, 1])
@pytest.mark.parametrize("p,dim", [(17, 128), (40, 1024), (200, 384), (300, 128), (1024, 128)])
def test_selection_equals_the_float32_replay(p, dim, penalty):
    """P = 17 / 40: one wave; 200: four waves, one candidate per thread; 300 and 1024: two and four candidates per thread."""
    corpus = _corpus(dim)
    cand, rel = _list(p, seed=10 + p)
    for lam in (0.0, 0.25, 0.5, 1.0):
        for k in sorted({1, 2, p // 2, p}):
            o_mmr, o_rel, o_idx, o_pos = _check_selection(corpus, cand, rel, k, lam, penalty)
            assert (o_pos[0] >= 0).all() and len(set(o_pos[0].tolist())) == k          # k distinct picks
            if lam == 1.0:                                                              # plain top-k: the first k, mmr == rel
                assert np.array_equal(o_pos[0], np.arange(k)) and np.array_equal(_i32(o_mmr[0]), _i32(o_rel[0]))
    # a batch: every query is its own selection
    lists = [_list(p, seed=50 + s) for s in range(3)]
    _check_selection(corpus, np.stack([c for c, _ in lists]), np.stack([r for _, r in lists]), min(p, 9), 0.5, penalty)


@pytest.mark.parametrize("penalty", [0, 1])
def test_selection_padding_duplicates_and_rows_outside_the_matrix(penalty):
    corpus = _corpus(128)
    # trailing padding: fewer than k can be picked, the padding outputs appear
    cand, rel = _list(40, seed=3, n_pad=30)
    o_mmr, o_rel, o_idx, o_pos = _check_selection(corpus, cand, rel, 20, 0.5, penalty)
    assert (o_pos[0, :10] >= 0).all() and (o_pos[0, 10:] == -1).all() and (o_idx[0, 10:] == -1).all()
    assert np.isneginf(o_mmr[0, 10:]).all() and np.isneginf(o_rel[0, 10:]).all()
    # nothing but padding
    o_mmr, o_rel, o_idx, o_pos = _check_selection(corpus, np.full(5, -1, np.int32), np.full(5, -np.inf, np.float32), 3, 0.5, penalty)
    assert (o_pos == -1).all() and np.isneginf(o_mmr).all()
    # the same row twice in one list: its second copy pays the full penalty, both are returned when k = P
    cand = np.array([9, 300, 9, 1200], dtype=np.int32)
    rel = np.array([0.8, 0.7, 0.6, 0.5], dtype=np.float32)
    _, _, _, o_pos = _check_selection(corpus, cand, rel, 4, 0.5, penalty)
    assert sorted(o_pos[0].tolist()) == [0, 1, 2, 3] and o_pos[0, 0] == 0 and o_pos[0, 1] == 1
    # entries whose row falls outside [0, n_rows) are padding: with idx_base, and behind a shortened matrix
    cand, rel = _list(33, seed=4)
    a = _check_selection(corpus, cand + 1000, rel, 33, 0.5, penalty, idx_base=1000)
    short = _check_selection(corpus, cand, rel, 33, 0.5, penalty, n_rows=2048)
    n_in = int((cand < 2048).sum())
    assert (a[3] >= 0).all() and (short[3][0, :n_in] >= 0).all() and (short[3][0, n_in:] == -1).all()
    assert (cand[short[3][0, :n_in]] < 2048).all()
    low = _check_selection(corpus, cand, rel, 33, 0.5, penalty, idx_base=2048)            # rows < 0 after the subtraction
    assert int((low[3] >= 0).sum()) == int((cand >= 2048).sum())


@pytest.mark.parametrize("penalty", [0, 1])
def test_selection_never_picks_a_nan_row(penalty):
    """A row tombstoned (NaN-filled) between the scan and the selection: its scan score is still finite, its similarities are NaN.
    It sits behind the first pick, so from step 1 on its value is NaN and it is never picked; the others' pen stays finite."""
    corpus = _corpus(128).clone()
    cand, rel = _list(40, seed=8)
    dead = 5
    corpus[int(cand[dead])] = float("nan")
    for lam in (0.0, 0.25, 0.5):
        (o_mmr, o_rel, o_idx, o_pos) = _check_selection(corpus, cand, rel, 40, lam, penalty)
        assert dead not in o_pos[0].tolist()
        assert (o_pos[0, :39] >= 0).all() and o_pos[0, 39] == -1
        assert np.isfinite(o_mmr[0, :39]).all()
    # and a NaN scan score is never picked either, at any lambda
    rel2 = rel.copy()
    rel2[dead] = np.nan
    for lam in (0.0, 0.5, 1.0):
        o_pos = _check_selection(_corpus(128), cand, rel2, 40, lam, penalty)[3]
        assert dead not in o_pos[0].tolist() and (o_pos[0, :39] >= 0).all()


# ---- 4. the constructed case through the real scan -------------------------------------------------------------------------------
def test_near_duplicate_is_traded_for_the_next_topic():
    """a, its near-duplicate a', b and f (tests/mmr_refs.py) among 1024 rows of filler orthogonal to the query: plain top-3 is
    a, a', b; MMR at 0.5 returns a, b, f."""
    dim = 128
    rows4, q = mr.constructed_rows(dim)
    g = torch.Generator().manual_seed(9)
    filler = torch.zeros(1024, dim)
    filler[:, 16:] = torch.randn(1024, dim - 16, generator=g)
    filler = filler / filler.norm(dim=1, keepdim=True)
    where = [100, 700, 40, 900]                                   # a before a': their scores tie, the scan orders by row
    filler[where] = torch.from_numpy(rows4)
    corpus = filler.to(torch.bfloat16).to(DEV).contiguous()
    qq = torch.from_numpy(q).to(torch.bfloat16).to(DEV)[None, :].contiguous()
    c_s, c_i = tscan.scan_topk(corpus, qq, 8)
    assert c_i[0, :4].tolist() == where
    assert c_s[0, :4].tolist() == [0.70703125, 0.70703125, 0.671875, 0.287109375]
    mmr, rel, idx, pos = tscan.mmr_select(corpus, c_i, c_s, 3, 0.5)
    assert idx[0].tolist() == [100, 40, 900] and pos[0].tolist() == [0, 2, 3]
    assert torch.equal(rel[0], c_s[0, [0, 2, 3]])
    # the values within the bound of test 1: v = 0.5 rel - 0.5 max G over the picks so far, each term off by at most half its
    # accumulation bound, plus three roundings of values below 1 (2^-24 each)
    cand = c_i[0].cpu().numpy()
    g64, gb, _ = mr.gram_fp64(corpus, cand)
    r64 = corpus[cand.astype(np.int64)].double().cpu().numpy() @ q.astype(np.float64)
    rb = dim * 2.0 ** -23 * (np.abs(corpus[cand.astype(np.int64)].double().cpu().numpy()) @ np.abs(q.astype(np.float64)))
    want = [0.5 * r64[0], 0.5 * r64[2] - 0.5 * g64[0, 2], 0.5 * r64[3] - 0.5 * max(g64[0, 3], g64[2, 3])]
    tol = [0.5 * rb[0], 0.5 * rb[2] + 0.5 * gb[0, 2], 0.5 * rb[3] + 0.5 * max(gb[0, 3], gb[2, 3])]
    got = mmr[0].cpu().numpy().astype(np.float64)
    for s in range(3):
        print(f"step {s}: v {got[s]:.8f} fp64 {want[s]:.8f} |err| {abs(got[s] - want[s]):.2e} tolerance {tol[s] + 3 * 2.0 ** -24:.2e}")
        assert abs(got[s] - want[s]) <= tol[s] + 3 * 2.0 ** -24
    assert got[1] == pytest.approx(0.0984, abs=1e-4)
    # lambda 1 is the scan's own order; "last" agrees with "max" on the first two picks by definition
    assert tscan.mmr_select(corpus, c_i, c_s, 3, 1.0)[2][0].tolist() == [100, 700, 40]
    assert tscan.mmr_select(corpus, c_i, c_s, 3, 0.5, penalty="last")[2][0, :2].tolist() == [100, 40]


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_code_and_writes_nothing():
    lib = _lib.load_library()
    corpus = _corpus(128)
    q, p, k = 2, 20, 5
    cand = torch.arange(q * p, dtype=torch.int32, device=DEV).view(q, p).contiguous()
    rel = torch.rand(q, p, device=DEV).sort(dim=1, descending=True).values.contiguous()
    need = lib.tt_mmr_workspace_bytes(q, p)
    assert need == q * 32 * 32 * 4 and lib.tt_mmr_workspace_bytes(1, 1024) == 4 << 20 and lib.tt_mmr_workspace_bytes(0, 40) == 0
    ws = torch.full((need // 4,), 7.0, dtype=torch.float32, device=DEV)
    outs = [torch.full((q, k), 7, dtype=dt, device=DEV) for dt in (torch.float32, torch.float32, torch.int32, torch.int32)]
    st = torch.cuda.current_stream(DEV).cuda_stream
    good = dict(corpus=corpus.data_ptr(), n_rows=N_ROWS, dim=128, cand=cand.data_ptr(), rel=rel.data_ptr(), n_queries=q, n_cand=p,
                k=k, lam=0.5, penalty=0, idx_base=0, o0=outs[0].data_ptr(), o1=outs[1].data_ptr(), o2=outs[2].data_ptr(),
                o3=outs[3].data_ptr(), ws=ws.data_ptr(), ws_bytes=need)

    def run(**change):
        a = dict(good, **change)
        return lib.tt_mmr_select(a["corpus"], a["n_rows"], a["dim"], a["cand"], a["rel"], a["n_queries"], a["n_cand"], a["k"],
                                 ctypes.c_float(a["lam"]), a["penalty"], a["idx_base"], a["o0"], a["o1"], a["o2"], a["o3"], a["ws"],
                                 a["ws_bytes"], st)

    cases = [(UNSUPPORTED, dict(dim=d)) for d in (0, 64, 100, 1152, 2048)]
    cases += [(UNSUPPORTED, dict(n_cand=c)) for c in (0, -1, 1025)]
    cases += [(UNSUPPORTED, dict(k=kk)) for kk in (0, -1, p + 1)]
    cases += [(UNSUPPORTED, dict(penalty=x)) for x in (-1, 2)]
    cases += [(INVALID, dict(lam=x)) for x in (float("nan"), -0.001, 1.001, float("inf"))]
    cases += [(INVALID, {name: None}) for name in ("corpus", "cand", "rel", "o0", "o1", "o2", "o3")]
    cases += [(INVALID, dict(n_queries=-1)), (INVALID, dict(n_rows=-1))]
    cases += [(WORKSPACE, dict(ws_bytes=need - 1)), (WORKSPACE, dict(ws=None)), (WORKSPACE, dict(ws_bytes=0))]
    cases += [(0, dict(n_queries=0))]                                   # an empty batch: fine, and nothing is written
    for code, change in cases:
        assert run(**change) == code, change
        if code:
            assert lib.tt_last_error(), change
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs) and bool((ws == 7.0).all())
    assert run() == 0                                                   # and the unchanged call goes through
    torch.cuda.synchronize()
    assert bool((outs[3] >= 0).all()) and bool((outs[3] < p).all())
