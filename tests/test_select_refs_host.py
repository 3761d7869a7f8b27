"""CPU: the numpy selection contract of tests/select_refs.py -- against ``oracle.scan.merge_topk`` where that one is defined,
against hand-written cases for every pinned rule, and the teeth of the inputs that tests/test_select_edges_gpu.py feeds the LDS
network: every wrong oracle must differ from the right one on every batch of query rows."""
import numpy as np
import pytest
import torch

import select_refs as refs
from oracle import scan as osc

INF = float("inf")
NAN = float("nan")


def _one(scores, idx, k):
    s, i = refs.select_topk(np.array([scores], dtype=np.float32), np.array([idx], dtype=np.int32), k)
    return s[0].tolist(), i[0].tolist()


# ---- 1. the oracle of today's merge tests -------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_contract_equals_merge_topk_on_its_domain(seed):
    """The inputs of test_topk_merge_random_lists (padding is the pair (-inf, -1), no NaN, unique indices, exact ties), plus
    zeros of both signs and live -inf entries, which ``merge_topk`` orders the same way."""
    rng = np.random.default_rng(900 + seed)
    q, lists, k = int(rng.integers(1, 40)), int(rng.integers(1, 17)), int(rng.integers(1, 300))
    m = lists * (int(rng.integers(1, k + 1)) if seed % 3 == 0 else k)
    vals = (rng.integers(-20, 20, (q, m)) / 8.0).astype(np.float32) if seed % 2 else rng.standard_normal((q, m)).astype(np.float32)
    vals[rng.random((q, m)) < 0.05] = -0.0
    vals[rng.random((q, m)) < 0.05] = -INF                                # live: the index stays
    idx = np.stack([rng.permutation(m) * 1000 + rng.integers(0, 1000, m) for _ in range(q)]).astype(np.int32)
    pad = rng.random((q, m)) < 0.15
    vals[pad], idx[pad] = -INF, -1
    want_v, want_i = osc.merge_topk(torch.from_numpy(vals), torch.from_numpy(idx).to(torch.int64), k)
    got_v, got_i = refs.select_topk(vals, idx, k)
    assert np.array_equal(got_i, want_i.numpy().astype(np.int32))
    assert refs.same_bits(got_v, got_i, want_v.numpy(), want_i.numpy().astype(np.int32)).all()
    assert np.array_equal(got_v, want_v.numpy())                          # (== : a zero of either sign)


# ---- 2. the pinned rules, by hand ---------------------------------------------------------------------------------------------
def test_live_entries_and_order():
    assert _one([1.0, 3.0, 2.0], [7, 8, 9], 2) == ([3.0, 2.0], [8, 9])
    assert _one([1.0, 1.0, 1.0], [9, 2, 5], 3) == ([1.0, 1.0, 1.0], [2, 5, 9])                   # index ascending
    assert _one([1.0, NAN, 2.0], [1, 0, 2], 3) == ([2.0, 1.0, -INF], [2, 1, -1])                 # NaN never ranks
    assert _one([NAN, NAN], [0, 1], 2) == ([-INF, -INF], [-1, -1])
    assert _one([5.0], [3], 4) == ([5.0, -INF, -INF, -INF], [3, -1, -1, -1])                     # fewer entries than k


def test_infinities_and_mismatched_entries():
    big = 2.0 ** 127
    assert _one([-INF, -big, -INF], [4, 5, 2], 3) == ([-big, -INF, -INF], [5, 2, 4])             # (-inf, id >= 0) is live, last
    assert _one([1.0, INF, big], [1, 2, 3], 2) == ([INF, big], [2, 3])                           # +inf ranks first
    assert _one([9.0, 1.0, -INF], [-1, 3, -5], 3) == ([1.0, -INF, -INF], [3, -1, -1])            # (finite, idx < 0) never ranks
    assert _one([-INF, -INF, 0.5], [-1, 6, -1], 2) == ([-INF, -INF], [6, -1])                    # a live -inf before the padding
    assert _one([1.0, 1.0], [0, refs.I32_MAX], 2) == ([1.0, 1.0], [0, refs.I32_MAX])


def test_zeros_are_one_value_and_duplicates_all_return():
    s, i = _one([-0.0, 0.0, -0.0, 0.0, -1.0], [8, 6, 2, 4, 0], 4)
    assert i == [2, 4, 6, 8] and all(v == 0 for v in s)                                           # index decides, not the sign
    got = refs.select_topk(np.array([[0.0, -0.0]], dtype=np.float32), np.array([[1, 0]], dtype=np.int32), 2)
    other_sign = (np.array([[-0.0, 0.0]], dtype=np.float32), got[1])
    assert refs.same_bits(*got, *other_sign).all()                                                # a returned zero of either sign
    assert not refs.same_bits(*got, np.array([[0.0, 1e-45]], dtype=np.float32), got[1]).any()     # ... but nothing else
    assert _one([2.0, 1.0, 2.0, 2.0, 3.0], [5, 1, 5, 4, 5], 4) == ([3.0, 2.0, 2.0, 2.0], [5, 4, 5, 5])   # duplicates, adjacent


def test_wrong_oracles_break_one_rule_each():
    w = refs.wrong_oracles(65)
    s = np.array([[1.0, 1.0, NAN, -0.0, 0.0]], dtype=np.float32)
    i = np.array([[3, 2, 1, 5, 6]], dtype=np.int32)
    assert w["ties by index descending"](s, i)[1][0, :4].tolist() == [3, 2, 6, 5]
    assert w["NaN ranks as +inf"](s, i)[1][0, :3].tolist() == [1, 2, 3]
    assert w["-0 below +0"](s, i)[1][0, :4].tolist() == [2, 3, 6, 5]
    room = refs.room_of(65)
    assert room == 8064 and refs.kpad_of(65) == 128 and refs.kpad_of(1024) == 1024 and refs.kpad_of(1000) == 1024
    long_s = np.zeros((1, room + 2), dtype=np.float32)
    long_s[0, room:] = 1.0
    long_i = np.arange(room + 2, dtype=np.int32)[None, :]
    assert w["last room-sized piece ignored"](long_s, long_i)[1][0, :2].tolist() == [0, 1]
    assert refs.select_topk(long_s, long_i, 65)[1][0, :3].tolist() == [room, room + 1, 0]


def test_list_lengths_name_every_threshold():
    assert refs.list_lengths(65) == [64, 65, 66, 128, 256, 2047, 2048, 2049, 32768, 32769, 8063, 8064, 8065, 8192, 16128, 16129,
                                     20000, 70001]
    assert refs.list_lengths(1024) == [1023, 1024, 1025, 2048, 2047, 2049, 4096, 4097, 7167, 7168, 7169, 8192, 14336, 14337,
                                       20000, 70001]
    for k in refs.KS:
        kpad = refs.kpad_of(k)
        m = refs.PREFILTER_KEYS // kpad * 1024
        assert -(-m // 1024) * kpad <= 4096 < -(-(m + 1) // 1024) * kpad


# ---- 3. teeth: no input batch may be blind to a broken rule --------------------------------------------------------------------
@pytest.mark.parametrize("k", refs.KS + (64,))
def test_every_batch_of_query_rows_tells_the_wrong_oracles_apart(k):
    """For every (k, list length) of the GPU sweep (and its k = 64 control): each wrong oracle disagrees with the contract on at
    least one query row of the batch -- a kernel that broke that rule would fail that case."""
    lengths = refs.list_lengths(k) if k != 64 else [5000]
    fewest = {}
    for m in lengths:
        s, ix = refs.query_rows(k, m)
        assert s.shape == (len(refs.ROW_NAMES), m) and s.dtype == np.float32 and ix.dtype == np.int32
        want = refs.select_topk(s, ix, k)
        assert (want[1][5] == -1).all() and (want[1][7] >= 0).sum() == min(k, m)
        for name, wrong in refs.wrong_oracles(k).items():
            differs = ~refs.same_bits(*wrong(s, ix), *want)
            fewest[name] = min(fewest.get(name, 99), int(differs.sum()))
            assert differs.any(), (k, m, name)
    print(f"\nk {k}: {len(lengths)} list lengths, fewest differing rows per wrong oracle {fewest}")


@pytest.mark.parametrize("m", refs.FALLBACK_LENGTHS)
def test_duplicate_pair_lists_tell_the_wrong_oracles_apart(m):
    k = refs.FALLBACK_K
    s, ix = refs.fallback_rows(m)
    want_s, want_i = refs.select_topk(s, ix, k)
    assert (want_i[0] == 12345).all() and (want_i[1] == 11).all()                                 # the copies first
    assert want_i[6, 0] == 1 and (want_i[6, 1:] == 5).all()
    assert (want_i[2, 40:] == 2).all() and (want_i[2, :40] != 2).all() and (want_i[5] == 7).all()
    assert (want_i[3, :30] != 4).all() and (want_s[3, 30:] == 0).all()
    for name, wrong in refs.wrong_oracles(k).items():
        assert (~refs.same_bits(*wrong(s, ix), want_s, want_i)).any(), (m, name)
