"""GPU: tt_filter_rows (metadata filter -> ascending row list) and tt_scan_topk_rows (exact top-k over the listed rows).

The row-list scan must be BIT-identical to tt_scan_topk over ``mat.index_select(0, rows)`` with the indices mapped back: the
streaming kernel scores every row with the same fragments and MFMA order wherever the row sits."""
import numpy as np
import pytest
import torch

import tensor_truth_amd  # noqa: F401
from oracle import scan as osc
from tensor_truth_amd import metadata_filter as mf
from tensor_truth_amd import scan as tscan

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N_CODES = 100_000          # codes 1..N_CODES spread uniformly: a pass rate p allows codes 1..round(p * N_CODES)


def _corpus(n, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((n, d), generator=g, device=DEV, dtype=torch.float32)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()


def _queries(q, d, seed):
    return _corpus(q, d, seed + 7)


def _codes(n, seed, absent=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    c = torch.randint(1, N_CODES + 1, (n,), generator=g, device=DEV, dtype=torch.int32)
    if absent:
        c[torch.rand((n,), generator=g, device=DEV) < absent] = 0
    return c


def _compiled(columns, alloweds, any_=False, bound=None):
    bits = [torch.from_numpy(mf.pack_bits(a).view(np.int32)).to(DEV) for a in alloweds]
    if bound is None:
        bound = int(columns[0].shape[0])
    return mf.CompiledFilter(list(columns), bits, [len(a) for a in alloweds], any_, bound)


def _allowed_rate(p):
    a = np.zeros(N_CODES + 1, dtype=bool)
    a[1: 1 + int(round(p * N_CODES))] = True
    return a


def _host_rows(columns, alloweds, any_, lo=0, hi=None):
    ok = None
    for col, a in zip(columns, alloweds):
        c = col.cpu().numpy()
        m = np.where(c < len(a), a[np.minimum(c, len(a) - 1)], False)
        ok = m if ok is None else (ok | m if any_ else ok & m)
    hi = len(ok) if hi is None else hi
    return np.nonzero(ok[lo:hi])[0] + lo


def _reference(mat, q, k, rows_np, idx_base=0):
    """tt_scan_topk over the gathered rows, indices mapped back."""
    if len(rows_np) == 0:
        return (torch.full((q.shape[0], k), float("-inf"), device=DEV), torch.full((q.shape[0], k), -1, dtype=torch.int32, device=DEV))
    sub = torch.from_numpy(rows_np).to(DEV)
    s, i = tscan.scan_topk(mat.index_select(0, sub).contiguous(), q, k)
    mapped = torch.where(i >= 0, sub[i.clamp_min(0).long()].to(torch.int32) + idx_base, i)
    return s, mapped


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- tt_filter_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("any_", [False, True])
def test_filter_rows_is_the_host_evaluator(any_):
    n = 1_000_003
    ca, cb = _codes(n, 1, absent=0.05), _codes(n, 2)
    aa, ab = _allowed_rate(0.3), _allowed_rate(0.6)
    aa[17] = False                       # holes in the allowed set
    comp = _compiled([ca, cb], [aa, ab], any_)
    rows, offs = tscan.filter_rows(comp, n, DEV)
    want = _host_rows([ca, cb], [aa, ab], any_)
    cnt = int(offs[-1])
    assert cnt == len(want) and int(offs[0]) == 0
    assert np.array_equal(rows[:cnt].cpu().numpy(), want)


def test_filter_rows_segments_and_short_bitsets():
    n = 600_000
    c = _codes(n, 3, absent=0.1)
    a = _allowed_rate(0.2)[:50_000]       # a bitset shorter than the codes: larger codes never pass
    seg = [1000, 1000, 4096, 250_001, 599_999]
    comp = _compiled([c], [a])
    rows, offs = tscan.filter_rows(comp, n, DEV, seg_offsets=seg)
    want = _host_rows([c], [a], False, seg[0], seg[-1])
    offs = offs.cpu().numpy()
    assert offs[-1] == len(want)
    assert np.array_equal(rows[: len(want)].cpu().numpy(), want)
    for s in range(len(seg)):
        assert offs[s] == np.searchsorted(want, seg[s]), s


def test_filter_rows_empty_range():
    c = _codes(100, 4)
    rows, offs = tscan.filter_rows(_compiled([c], [_allowed_rate(1.0)]), 100, DEV, seg_offsets=[40, 40])
    assert offs.cpu().tolist() == [0, 0]


# ---- tt_scan_topk_rows ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    mat = _corpus(1_000_000, 1024, 11)
    codes = _codes(1_000_000, 12)
    yield mat, codes
    del mat, codes
    torch.cuda.empty_cache()


@pytest.mark.parametrize("rate", [0.0, 1e-5, 1e-3, 0.1, 0.5, 1.0])
def test_rows_scan_is_bit_identical_1m_x_1024(big, rate):
    mat, codes = big
    a = _allowed_rate(rate)
    comp = _compiled([codes], [a])
    rows, offs = tscan.filter_rows(comp, mat.shape[0], DEV)
    listed = _host_rows([codes], [a], False)
    bound = int(min(len(listed) + 10, mat.shape[0]))          # any upper bound will do
    for nq in (1, 4, 64):
        q = _queries(nq, 1024, 100 + nq)
        for k in (1, 10, 50, 1024):
            s, i = tscan.scan_topk_rows(mat, q, k, rows, offs, bound, idx_base=5)
            ws, wi = _reference(mat, q, k, listed, idx_base=5)
            assert _bits_equal(s, ws), (rate, nq, k)
            assert torch.equal(i, wi), (rate, nq, k)
            if rate <= 1e-3 and nq <= 4:          # small subsets: the CPU oracle too
                sub = mat.index_select(0, torch.from_numpy(listed).to(DEV)).cpu() if len(listed) else None
                if sub is not None:
                    os_, oi, gap = osc.scan_topk(sub, q.cpu(), k)
                    tie_free = gap > 1e-6
                    got = i.cpu().to(torch.int64)
                    want = torch.where(oi >= 0, torch.from_numpy(listed)[oi.clamp_min(0)] + 5, oi)
                    assert torch.equal(got[tie_free], want[tie_free])


def test_full_pass_rate_equals_the_unfiltered_scan(big):
    mat, codes = big
    comp = _compiled([codes], [_allowed_rate(1.0)])
    rows, offs = tscan.filter_rows(comp, mat.shape[0], DEV)
    for nq, k in ((1, 10), (64, 50)):
        q = _queries(nq, 1024, 900 + nq)
        s, i = tscan.scan_topk_rows(mat, q, k, rows, offs, mat.shape[0])
        ws, wi = tscan.scan_topk(mat, q, k)
        assert _bits_equal(s, ws) and torch.equal(i, wi)


@pytest.mark.parametrize("d", [384, 768])
@pytest.mark.parametrize("rate", [0.0, 1e-3, 0.1, 0.5, 1.0])
def test_rows_scan_100k(d, rate):
    mat = _corpus(100_000, d, 21 + d)
    codes = _codes(100_000, 22)
    a = _allowed_rate(rate)
    rows, offs = tscan.filter_rows(_compiled([codes], [a]), mat.shape[0], DEV)
    listed = _host_rows([codes], [a], False)
    for nq in (1, 4, 64):
        q = _queries(nq, d, 300 + nq)
        for k in (1, 10, 50, 1024):
            s, i = tscan.scan_topk_rows(mat, q, k, rows, offs, len(listed))
            ws, wi = _reference(mat, q, k, listed)
            assert _bits_equal(s, ws) and torch.equal(i, wi), (d, rate, nq, k)
    if len(listed):
        q = _queries(4, d, 77)
        s, i = tscan.scan_topk_rows(mat, q, 50, rows, offs, len(listed))
        os_, oi, gap = osc.scan_topk(mat.index_select(0, torch.from_numpy(listed).to(DEV)).cpu(), q.cpu(), 50)
        tie_free = gap > 1e-6
        want = torch.where(oi >= 0, torch.from_numpy(listed)[oi.clamp_min(0)], oi)
        assert torch.equal(i.cpu().to(torch.int64)[tie_free], want[tie_free])


def test_fewer_matches_than_k_pads():
    mat = _corpus(200_000, 512, 31)
    codes = torch.zeros(200_000, dtype=torch.int32, device=DEV)
    pick = torch.tensor([5, 70_000, 199_999], device=DEV)
    codes[pick] = 1
    a = np.array([False, True])
    rows, offs = tscan.filter_rows(_compiled([codes], [a]), mat.shape[0], DEV)
    q = _queries(3, 512, 32)
    for bound in (3, 200_000):         # the dense path and the streaming path over a short list
        s, i = tscan.scan_topk_rows(mat, q, 10, rows, offs, bound)
        assert (i[:, :3].sort(dim=1).values.cpu() == torch.tensor([5, 70_000, 199_999], dtype=torch.int32)).all()
        assert torch.isfinite(s[:, :3]).all()
        assert (i[:, 3:] == -1).all() and torch.isinf(s[:, 3:]).all() and (s[:, 3:] < 0).all()


def test_tombstoned_rows_never_come_back():
    mat = _corpus(300_000, 1024, 41)
    codes = _codes(300_000, 42)
    a = _allowed_rate(0.3)
    listed = _host_rows([codes], [a], False)
    dead = torch.from_numpy(listed[::3]).to(DEV)
    mat[dead] = float("nan")
    rows, offs = tscan.filter_rows(_compiled([codes], [a]), mat.shape[0], DEV)
    q = _queries(8, 1024, 43)
    s, i = tscan.scan_topk_rows(mat, q, 100, rows, offs, len(listed))
    got = set(i.flatten().cpu().tolist())
    assert not (got & set(listed[::3].tolist()))
    ws, wi = _reference(mat, q, 100, listed)
    assert _bits_equal(s, ws) and torch.equal(i, wi)


def test_overflowing_candidate_lists_fall_back_exactly():
    """Every listed row scores the same: every one passes the threshold and the candidate lists overflow."""
    n, d = 400_000, 256
    mat = _corpus(n, d, 51)
    codes = _codes(n, 52)
    a = _allowed_rate(0.5)
    listed = _host_rows([codes], [a], False)
    same = _corpus(1, d, 53)
    mat[torch.from_numpy(listed[: 200_000]).to(DEV)] = same
    rows, offs = tscan.filter_rows(_compiled([codes], [a]), n, DEV)
    q = torch.cat([same, _queries(1, d, 54)]).contiguous()
    _, _, flag = tscan.scan_topk_rows(mat, q, 64, rows, offs, len(listed), return_flag=True)
    assert flag != 0, "the adversarial set did not overflow: the test does not reach the fallback"
    s, i = tscan.scan_topk_rows(mat, q, 64, rows, offs, len(listed))
    ws, wi = _reference(mat, q, 64, listed)
    assert _bits_equal(s, ws) and torch.equal(i, wi)
    assert i[0].cpu().tolist() == listed[:64].tolist()        # ties: rows ascending
    hs, hi = tscan.scan_topk_rows_host(mat, q, 64, rows, offs, len(listed))
    assert torch.equal(hi, wi.cpu()) and _bits_equal(hs, ws.cpu())


def test_segmented_form_matches_per_segment_runs():
    n, d = 500_000, 768
    mat = _corpus(n, d, 61)
    codes = _codes(n, 62)
    a = _allowed_rate(0.2)
    seg = [0, 120_000, 120_000, 125_000, 400_000, 500_000]
    rows, offs = tscan.filter_rows(_compiled([codes], [a]), n, DEV, seg_offsets=seg)
    q = _queries(5, d, 63)
    k = 20
    bound = max(len(_host_rows([codes], [a], False, seg[s], seg[s + 1])) for s in range(len(seg) - 1))
    s, i = tscan.scan_topk_rows(mat, q, k, rows, offs, bound, seg_offsets=seg)
    hs, hi = tscan.scan_topk_rows_host(mat, q, k, rows, offs, bound, seg_offsets=seg)
    assert s.shape == (5, len(seg) - 1, k)
    for m in range(len(seg) - 1):
        listed = _host_rows([codes], [a], False, seg[m], seg[m + 1])
        ws, wi = _reference(mat, q, k, listed, idx_base=-seg[m])
        assert _bits_equal(s[:, m], ws) and torch.equal(i[:, m], wi), m
        assert _bits_equal(hs[:, m], ws.cpu()) and torch.equal(hi[:, m], wi.cpu()), m
