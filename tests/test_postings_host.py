"""CPU: the host side of the posting-list search (tensor_truth_amd/postings.py) -- the numpy planner that decides which lists a pass
takes and when the candidates provably hold the whole top-k -- and the numpy reference builder the GPU tests compare the device
build with (tests/postings_refs.py).  No device is touched.

The planner's rules: N's bound is below theta STRICTLY and one more id breaks that; a theta that is 0, negative
or -inf, a query weight that is NaN or negative, or an index that is not prunable prune nothing; pass 1 is the shortest prefix in
descending bound whose lists hold PASS1_FACTOR * k entries; the bound is never below the exact fp64 sum, nor below what fp32
arithmetic of the kernel's shape gives.
"""
import numpy as np
import postings_refs as R
import pytest

from tensor_truth_amd import postings as P

VOCAB = 300


def _instance(rng, n_terms=None):
    """A random query over a random index -> (q_terms, q_weights, post_off, term_ub)."""
    lengths = rng.integers(0, 400, VOCAB)
    lengths[rng.random(VOCAB) < 0.2] = 0
    off = np.zeros(VOCAB + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    ub = np.where(lengths > 0, rng.random(VOCAB) * 4, 0).astype(np.float32)
    n = int(rng.integers(1, 40)) if n_terms is None else n_terms
    qt = np.sort(rng.choice(VOCAB, n, replace=False)).astype(np.int32)
    qw = (rng.random(n) * 3).astype(np.float32)
    return qt, qw, off, ub


def test_upper_bound_is_never_below_the_fp64_sum_nor_below_fp32_arithmetic():
    rng = np.random.default_rng(5)
    assert P.upper_bound(np.zeros(0)) == 0
    for trial in range(300):
        n = int(rng.integers(1, 513))
        scale = 10.0 ** rng.integers(-44, 30)
        c32 = (rng.random(n) * scale).astype(np.float32)
        c = c32.astype(np.float64)
        b = P.upper_bound(c)
        assert b.dtype == np.float32 and float(b) >= float(np.sum(c)), (trial, n)
        # fp32 sums of the same terms in the kernel's shape: 64 strided chains, then a butterfly
        lanes = np.zeros(64, dtype=np.float32)
        for j, v in enumerate(c32):
            lanes[j % 64] = np.float32(lanes[j % 64] + v)
        o = 32
        while o:
            lanes = (lanes + lanes[np.arange(64) ^ o]).astype(np.float32)
            o >>= 1
        assert float(b) >= float(lanes[0]), (trial, n)
        assert float(b) >= float(np.sum(c32, dtype=np.float32))
    # a sum that fp32 cannot hold rounds UP to the next fp32, never down
    c = np.asarray([1.0, 2.0 ** -30])
    assert float(P.upper_bound(c)) > 1.0 + 2.0 ** -30


def test_non_essential_set_is_strictly_below_theta_and_maximal():
    rng = np.random.default_rng(11)
    hits = 0
    for trial in range(300):
        qt, qw, off, ub = _instance(rng)
        c = P.term_bounds(qt, qw, ub, VOCAB)
        assert (c >= 0).all() and np.array_equal(c, qw.astype(np.float64) * ub[qt].astype(np.float64))
        theta = float(np.float32(rng.random() * np.sum(c) * 1.2))
        n = P.non_essential(c, theta)
        order = np.argsort(c, kind="stable")
        assert np.array_equal(n, order[:len(n)]), "N is a prefix in ascending bound"
        if theta > 0:
            assert float(P.upper_bound(c[n])) < theta
        if len(n) < len(c):
            assert not float(P.upper_bound(c[order[:len(n) + 1]])) < theta, "one more id must break the bound"
            hits += 1
        assert float(np.sum(c[n])) <= float(P.upper_bound(c[n]))
    assert hits > 100
    # strictness: a bound EQUAL to theta excludes nothing
    c = np.asarray([0.5])
    b = float(P.upper_bound(c))
    assert len(P.non_essential(c, b)) == 0 and len(P.non_essential(c, float(np.nextafter(np.float32(b), np.float32(2))))) == 1


@pytest.mark.parametrize("theta", [0.0, -0.0, -1.5, -np.inf, np.nan])
def test_a_theta_that_is_not_positive_prunes_nothing(theta):
    rng = np.random.default_rng(3)
    qt, qw, off, ub = _instance(rng, 12)
    c = P.term_bounds(qt, qw, ub, VOCAB)
    assert len(P.non_essential(c, theta)) == 0
    first, c, lengths, ok = P.plan_first(qt, qw, off, ub, VOCAB, True, 3)
    what, pos = P.plan_second(c, lengths, first, theta, ok)
    listed = np.flatnonzero(lengths > 0)
    if set(listed) <= set(first):
        assert what == "scan" and pos is None
    else:
        assert what == "pass" and np.array_equal(pos, listed), "every list is taken: the unpruned rule"


@pytest.mark.parametrize("case", ["nan weight", "negative weight", "infinite weight", "index not prunable"])
def test_a_query_or_an_index_outside_the_preconditions_prunes_nothing(case):
    rng = np.random.default_rng(8)
    for _ in range(20):
        qt, qw, off, ub = _instance(rng, 16)
        prunable = case != "index not prunable"
        if case == "nan weight":
            qw[3] = np.nan
        elif case == "negative weight":
            qw[5] = -0.25
        elif case == "infinite weight":
            qw[7] = np.inf
        assert not P.may_prune(qw, prunable)
        first, c, lengths, ok = P.plan_first(qt, qw, off, ub, VOCAB, prunable, 5)
        listed = np.flatnonzero(lengths > 0)
        assert not ok and np.array_equal(np.sort(first), listed), "pass 1 takes every list"
        assert P.plan_second(c, lengths, first, 7.5, ok) == ("done", None)
        assert P.plan_second(c, lengths, first, 0.0, ok) == ("scan", None)
        assert P.plan_second(c, lengths, first, -np.inf, ok) == ("scan", None)
    assert P.may_prune(np.asarray([0.0, 1.0], dtype=np.float32), True)


def test_pass1_is_the_shortest_prefix_in_descending_bound_that_holds_enough_entries():
    rng = np.random.default_rng(21)
    for _ in range(200):
        qt, qw, off, ub = _instance(rng)
        k = int(rng.integers(1, 300))
        c = P.term_bounds(qt, qw, ub, VOCAB)
        lengths = P.list_lengths(qt, off, VOCAB)
        assert np.array_equal(lengths, off[qt.astype(np.int64) + 1] - off[qt])
        first = P.pass1_prefix(c, lengths, k)
        order = np.argsort(-c, kind="stable")
        assert np.array_equal(first, order[:len(first)])
        need = P.PASS1_FACTOR * k
        if lengths.sum() < need:
            assert len(first) == len(qt)
        else:
            assert lengths[first].sum() >= need and lengths[first[:-1]].sum() < need
        planned = P.plan_first(qt, qw, off, ub, VOCAB, True, k)[0]
        assert np.array_equal(planned, first[lengths[first] > 0]), "lists of length 0 are not taken"


def test_the_second_pass_takes_the_ids_outside_n_unless_pass1_had_them():
    # id 10: short list, heavy; id 11: in every document, light (the GPU suite's pruning case, on the host)
    off = np.zeros(VOCAB + 1, dtype=np.int64)
    off[11:] = 20
    off[12:] = 1020
    ub = np.zeros(VOCAB, dtype=np.float32)
    ub[10], ub[11] = 2.0, 0.01
    qt, qw = np.asarray([10, 11], dtype=np.int32), np.ones(2, dtype=np.float32)
    first, c, lengths, ok = P.plan_first(qt, qw, off, ub, VOCAB, True, 10)
    assert ok and first.tolist() == [0] and lengths.tolist() == [20, 1000]
    assert P.plan_second(c, lengths, first, 2.01, ok) == ("done", None), "id 11 alone cannot reach theta: no second pass"
    what, pos = P.plan_second(c, lengths, first, 0.01, ok)
    assert what == "pass" and pos.tolist() == [0, 1], "theta from documents that hold only id 11: nothing is pruned"
    first50 = P.plan_first(qt, qw, off, ub, VOCAB, True, 50)[0]
    assert sorted(first50.tolist()) == [0, 1] and P.plan_second(c, lengths, first50, 0.01, ok) == ("done", None)
    # ids outside the vocabulary or without a list bound nothing and list nothing
    qt2 = np.asarray([10, 11, 200, VOCAB + 5], dtype=np.int32)
    first, c, lengths, ok = P.plan_first(qt2, np.ones(4, dtype=np.float32), off, ub, VOCAB, True, 10)
    assert c.tolist() == [2.0, float(np.float32(0.01)), 0.0, 0.0] and lengths.tolist() == [20, 1000, 0, 0] and first.tolist() == [0]
    lo, hi, start, longest = P.ranges_of([qt2[first], qt2[[0, 1]]], off)
    assert lo.tolist() == [0, 0, 20] and hi.tolist() == [20, 20, 1020] and start.tolist() == [0, 1, 3] and longest == 1020


def test_reference_builder():
    terms = np.asarray([5, 7, 9, 5, 9, 7, 5, 300, 2], dtype=np.int32)
    weights = np.asarray([1.0, 0.5, 2.0, 3.0, -1.0, 0.25, 9.0, 1.0, np.inf], dtype=np.float32)
    d_start = np.asarray([0, 3, 5, 5, 6, 7], dtype=np.int64)
    d_nnz = np.asarray([3, 2, 0, 1, -1, 2], dtype=np.int32)           # document 2 empty, document 4 a tombstone (holds id 5 at 9.0)
    off, lists, ub, flags = R.reference_postings(terms, weights, d_start, d_nnz, 5, 10)
    assert lists[5].tolist() == [0, 1] and lists[7].tolist() == [0, 3] and lists[9].tolist() == [0, 1] and off[-1] == 6
    assert ub[5] == 3.0 and ub[7] == 0.5 and ub[9] == 2.0 and flags == P.FLAG_WEIGHT
    off, lists, ub, flags = R.reference_postings(terms, weights, d_start, d_nnz, 6, 10)
    # document 5 holds (300, 2): an id outside the vocabulary, an infinite weight, and ids that do not ascend
    assert flags == P.FLAG_WEIGHT | P.FLAG_TERM_RANGE | P.FLAG_ORDER and lists[2].tolist() == [5] and ub[2] == 0 and off[-1] == 7
    off, lists, ub, flags = R.reference_postings(terms, weights, d_start, d_nnz, 0, 10)
    assert off.tolist() == [0] * 11 and flags == 0 and not ub.any()
    assert (R.FLAG_TERM_RANGE, R.FLAG_WEIGHT, R.FLAG_ORDER) == (P.FLAG_TERM_RANGE, P.FLAG_WEIGHT, P.FLAG_ORDER)
    # a repeated id, and ids out of order: bit 2; the document is listed once per occurrence
    for ids in ([5, 5, 7], [7, 5, 9]):
        off, lists, ub, flags = R.reference_postings(np.asarray(ids, dtype=np.int32), np.ones(3, dtype=np.float32), [0], [3], 1, 10)
        assert flags == P.FLAG_ORDER and off[-1] == 3 and lists[5].tolist() == [0] * ids.count(5)
