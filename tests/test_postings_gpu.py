"""GPU: posting lists for the lexical / SPLADE stores (csrc/postings.hip, tensor_truth_amd/postings.py).

One sentence is the acceptance test: whatever ``LexicalStore.search`` returns through the lists equals ``tt_lexical_scan_topk``'s
result on the same arrays, bit for bit and index for index.  Every comparison here is exact -- scores by ``.tobytes()``, document
numbers by ``==`` -- so there is no tolerance to derive.

* The device build against the numpy reference builder (tests/postings_refs.py): every list as a sorted set (the order
  inside a list is unspecified), ``post_off`` and ``term_ub`` exactly, the flag word, a refused build's guard words.
* Equality with the scan on the scan test's own generator (coarse weight grids: ties are the rule; about a third zero scores; every
  seventh document a tombstone), at sizes around the wave (31 .. 65), at 1000, and one past the compaction's per-workgroup span and
  one past twice it; sealed nowhere, everywhere, and with tails of 1, 37 and half the documents.
* Store behaviour, pruning that is both safe and real, and both retrievers with ``postings`` on.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import postings_refs as R
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M3 = os.path.join(GOLDEN, "m3_l2")
SPLADE = os.path.join(GOLDEN, "splade_l2")
VOCAB = 600
SPAN = 8192                                # TT_POSTINGS_SPAN: documents per workgroup of the compaction
GUARD = 64


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _pack(parts, dtype):
    nn = np.asarray([len(p) for p in parts], dtype=np.int64)
    st = np.zeros(len(parts), dtype=np.int64)
    np.cumsum(nn[:-1], out=st[1:])
    flat = np.concatenate([np.asarray(p, dtype=dtype) for p in parts]) if nn.sum() else np.zeros(0, dtype=dtype)
    return flat.astype(dtype), st, nn.astype(np.int32)


# ---- the build ---------------------------------------------------------------------------------------------------------------------
def _build_inputs(n_docs, seed, negative=False):
    """Documents over ids 10 .. 409 of a vocabulary of 600: id 5 in every document, id 6 in none, every fifth document empty,
    every seventh a tombstone that keeps its entries."""
    rng = np.random.default_rng(seed)
    terms, weights, nnz = [], [], []
    for d in range(n_docs):
        n = 0 if d % 5 == 4 else int(rng.integers(0, 12))
        ids = np.sort(np.concatenate(([5], rng.choice(np.arange(10, 410), n, replace=False)))) if d % 5 != 4 else np.zeros(0)
        terms.append(ids.astype(np.int32))
        weights.append((rng.integers(1, 9, len(ids)) * 0.25).astype(np.float32))
        nnz.append(-1 if d % 7 == 3 else len(ids))
    dt_, ds, _ = _pack(terms, np.int32)
    dw = _pack(weights, np.float32)[0]
    if negative and len(dw):
        dw[len(dw) // 2] = -0.5
    return dt_, dw, ds, np.asarray(nnz, dtype=np.int32)


def _device_lists(ix):
    off, doc = ix.off_host, ix.post_doc.cpu().numpy()
    return [np.sort(doc[off[t]:off[t + 1]]) for t in range(ix.vocab)]


@pytest.mark.parametrize("n_docs", [0, 1, 64, 1000])
def test_build_equals_the_numpy_reference(dev, built_lib, n_docs):
    from tensor_truth_amd import postings as P

    dt_, dw, ds, dn = _build_inputs(n_docs, 7 + n_docs)
    pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)  # noqa: E731
    args = (_t(pad(dt_), dev), _t(pad(dw), dev), _t(pad(ds), dev), _t(pad(dn), dev))
    for n_sealed in sorted({0, n_docs // 2, n_docs}):
        want_off, want_lists, want_ub, want_flags = R.reference_postings(dt_, dw, ds, dn, n_sealed, VOCAB)
        ix = P.postings_build(*args, n_sealed, VOCAB, len(dt_))
        assert ix.flags == want_flags == 0 and ix.prunable and ix.n_sealed == n_sealed
        assert np.array_equal(ix.off_host, want_off) and ix.n_entries == int(want_off[-1])
        got = _device_lists(ix)
        assert all(np.array_equal(g, w) for g, w in zip(got, want_lists)), "a list differs from the reference as a sorted set"
        assert ix.ub_host.tobytes() == want_ub.tobytes(), "term_ub"
        live = int(((dn[:n_sealed] >= 0) & (np.arange(n_sealed) % 5 != 4)).sum())
        assert len(got[5]) == live and len(got[6]) == 0 and ix.ub_host[6] == 0, "an id in every live document, an id in none"
        assert ix.nbytes == 12 * VOCAB + 8 + 4 * max(len(dt_), 1)
    print(f"\nbuild n_docs {n_docs}: {ix.n_entries} entries, {int((np.diff(ix.off_host) > 0).sum())} lists")


def test_build_refuses_an_id_outside_the_vocabulary_and_writes_nothing_behind_post_doc(dev, built_lib):
    from tensor_truth_amd import _lib
    from tensor_truth_amd import postings as P

    dt_, dw, ds, dn = _build_inputs(1000, 99)
    total = int(R.reference_postings(dt_, dw, ds, dn, 1000, VOCAB)[0][-1])
    pattern = 0x5A5A5A5A
    for what, bad_id, cap in (("id == vocab", VOCAB, total), ("negative id", -1, total), ("huge id", 2 ** 31 - 1, total),
                              ("post_doc too short", None, total - 1)):
        terms = dt_.copy()
        if bad_id is not None:
            terms[int(ds[np.flatnonzero(dn > 0)[10]])] = bad_id                                     # a live document's first entry
        buf = torch.full((cap + GUARD,), pattern, dtype=torch.int32, device=dev)
        with pytest.raises(_lib.TTError, match="outside the vocabulary" if bad_id is not None else "entries for post_doc"):
            P.postings_build(_t(terms, dev), _t(dw, dev), _t(ds, dev), _t(dn, dev), 1000, VOCAB, cap, post_doc=buf)
        assert (buf[cap:].cpu().numpy() == pattern).all(), f"{what}: the guard words behind post_doc changed"
        assert (buf.cpu().numpy() == pattern).all(), f"{what}: a refused build filled something"
    # the same arrays with room: built, and the guard still intact
    buf = torch.full((total + GUARD,), pattern, dtype=torch.int32, device=dev)
    ix = P.postings_build(_t(dt_, dev), _t(dw, dev), _t(ds, dev), _t(dn, dev), 1000, VOCAB, total, post_doc=buf)
    assert ix.n_entries == total and (buf[total:].cpu().numpy() == pattern).all() and (buf[:total].cpu().numpy() != pattern).all()
    # a tombstone's out-of-range id is never read
    terms = dt_.copy()
    terms[int(ds[3])] = VOCAB + 7
    assert dn[3] == -1 and P.postings_build(_t(terms, dev), _t(dw, dev), _t(ds, dev), _t(dn, dev), 1000, VOCAB, total).flags == 0


def test_a_negative_weight_marks_the_index_not_prunable(dev, built_lib):
    from tensor_truth_amd import postings as P

    for bad in (-0.5, np.nan, np.inf):
        dt_, dw, ds, dn = _build_inputs(64, 5)
        slot = int(ds[np.flatnonzero(dn > 1)[2]]) + 1
        dw[slot] = bad
        want_off, want_lists, want_ub, want_flags = R.reference_postings(dt_, dw, ds, dn, 64, VOCAB)
        ix = P.postings_build(_t(dt_, dev), _t(dw, dev), _t(ds, dev), _t(dn, dev), 64, VOCAB, len(dt_))
        assert ix.flags == want_flags == P.FLAG_WEIGHT and not ix.prunable
        assert all(np.array_equal(g, w) for g, w in zip(_device_lists(ix), want_lists)), "the document stays on its lists"
        assert ix.ub_host.tobytes() == want_ub.tobytes()


def test_a_repeated_or_descending_id_marks_the_index_not_prunable(dev, built_lib):
    """The scoring kernel adds a repeated id once per occurrence, so ``term_ub`` would not bound its contribution: the build says so,
    the lists stay complete (the document once per occurrence), and the store's answers stay the scan's."""
    from tensor_truth_amd import postings as P
    from tensor_truth_amd.lexical import LexicalWeights
    from tensor_truth_amd.splade import SpladeStore

    for what in ("repeated", "descending"):
        dt_, dw, ds, dn = _build_inputs(64, 5)
        slot = int(ds[np.flatnonzero(dn > 2)[1]]) + 1
        dt_[slot] = dt_[slot - 1] if what == "repeated" else dt_[slot + 1] + 1
        want_off, want_lists, want_ub, want_flags = R.reference_postings(dt_, dw, ds, dn, 64, VOCAB)
        ix = P.postings_build(_t(dt_, dev), _t(dw, dev), _t(ds, dev), _t(dn, dev), 64, VOCAB, len(dt_))
        assert ix.flags == want_flags == P.FLAG_ORDER and not ix.prunable, what
        assert all(np.array_equal(g, w) for g, w in zip(_device_lists(ix), want_lists))
        assert ix.ub_host.tobytes() == want_ub.tobytes()
    # document 30 holds id 11 twice at 1.5: it scores 3.0 and beats the twenty documents that hold id 10 at 2.0, although id 11's
    # bound, 1.5, is below theta = 2.0 -- the case a per-term maximum would prune wrongly
    docs = [{10: 2.0} for _ in range(20)] + [{12: 0.25} for _ in range(10)] + [None] + [{12: 0.25} for _ in range(9)]
    on, off = SpladeStore(dev, postings=True, vocab_size=VOCAB), SpladeStore(dev)
    twice = LexicalWeights(_t(np.asarray([11, 11], dtype=np.int32), dev), _t(np.asarray([1.5, 1.5], dtype=np.float32), dev),
                           np.zeros(1, dtype=np.int64), np.asarray([2], dtype=np.int32))
    for st in (on, off):
        st.add(list(range(30)), _lw(dev, docs[:30]))
        st.add([30], twice)
        st.add(list(range(31, 40)), _lw(dev, docs[31:]))
    on.seal()
    assert on.index.flags == P.FLAG_ORDER and not on.index.prunable
    q = _lw(dev, [{10: 1.0, 11: 1.0}])
    _same(on.search(q, 10), off.search(q, 10), "a document that repeats an id")
    assert on.search(q, 10)[1].cpu().numpy()[0, 0] == 30 and on.search(q, 10)[0].cpu().numpy()[0, 0] == 3.0
    assert on.stats["candidates"] == 21 and on.stats["fallbacks"] == 0, on.stats      # the twenty and document 30, once


def test_a_malformed_query_is_refused_as_the_scan_refuses_it(dev, built_lib):
    from tensor_truth_amd.lexical import LexicalWeights
    from tensor_truth_amd.splade import SpladeStore

    on, off = SpladeStore(dev, postings=True, vocab_size=VOCAB), SpladeStore(dev)
    for st in (on, off):
        st.add(list(range(8)), _lw(dev, [{10 + d: 1.0} for d in range(8)]))
    on.seal()
    good = _lw(dev, [{10: 1.0, 11: 1.0}])
    past_the_end = LexicalWeights(good.terms, good.weights, np.asarray([1], dtype=np.int64), np.asarray([2], dtype=np.int32))
    too_long = LexicalWeights(good.terms, good.weights, np.asarray([0], dtype=np.int64), np.asarray([3], dtype=np.int32))
    for bad in (past_the_end, too_long):
        for st in (off, on):
            with pytest.raises(ValueError, match="q_start"):
                st.search(bad, 3)
    _same(on.search(good, 3), off.search(good, 3), "the well-formed query")


def test_refusals_come_before_a_launch(dev, built_lib):
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    i = torch.zeros(8, dtype=torch.int32, device=dev)
    l = torch.zeros(8, dtype=torch.int64, device=dev)
    f = torch.zeros(8, dtype=torch.float32, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)

    def call(n_q, k, n_docs=4, n_sealed=4, ws_bytes=1 << 16):
        return lib.tt_lexical_topk_postings(i.data_ptr(), f.data_ptr(), i.data_ptr(), i.data_ptr(), n_q, i.data_ptr(), f.data_ptr(),
                                            l.data_ptr(), i.data_ptr(), n_docs, i.data_ptr(), 0, n_sealed, l.data_ptr(), l.data_ptr(),
                                            i.data_ptr(), 0, k, f.data_ptr(), i.data_ptr(), f.data_ptr(), i.data_ptr(), i.data_ptr(),
                                            ws.data_ptr(), ws_bytes, None)

    assert call(65, 2) == -2 and b"n_q=65" in lib.tt_last_error()
    assert call(0, 2) == -2 and call(1, 0) == -2 and call(1, 1025) == -2
    assert call(1, 2, n_docs=4, n_sealed=5) == -1
    assert call(1, 2, ws_bytes=8) == -3
    assert lib.tt_lexical_topk_postings_workspace_bytes(1000, 1000, 3) >= 3 * (1000 * 8 + 1000 // 8)
    assert lib.tt_lexical_topk_postings_workspace_bytes(10, 11, 1) == 0 and lib.tt_postings_build_workspace_bytes(VOCAB) >= 4 * VOCAB


# ---- equality with the scan ------------------------------------------------------------------------------------------------------
def _scan_inputs(n_docs, n_q, seed):
    """test_lexical_gpu.py's generator of test_lexical_scan_topk_is_the_sorted_score, unchanged."""
    rng = np.random.default_rng(seed)
    vocab = np.arange(10, 10 + 400)
    d_terms, d_nnz = [], []
    for d in range(n_docs):
        n = int(rng.integers(0, 12))
        d_terms.append(np.sort(rng.choice(vocab, n, replace=False)).astype(np.int32))
        d_nnz.append(-1 if (d % 7 == 3 and n_docs > 1) else n)         # tombstones keep their entries
    q_terms = [np.sort(rng.choice(vocab, int(rng.integers(1, 5)), replace=False)).astype(np.int32) for _ in range(n_q)]
    def pack(parts):
        nn = np.asarray([len(p) for p in parts], dtype=np.int64)
        st = np.zeros(len(parts), dtype=np.int64)
        np.cumsum(nn[:-1], out=st[1:])
        return (np.concatenate(parts) if nn.sum() else np.zeros(1, dtype=np.int32)).astype(np.int32), st
    qt, qs = pack(q_terms)
    dt_, ds = pack(d_terms)
    # weights on a coarse grid: equal scores between different documents are the rule, not the exception
    qw = rng.integers(1, 4, len(qt)).astype(np.float32) * 0.5
    dw = rng.integers(1, 3, len(dt_)).astype(np.float32) * 0.5
    return qt, qw, qs.astype(np.int32), np.asarray([len(p) for p in q_terms], dtype=np.int32), dt_, dw, ds, np.asarray(d_nnz, dtype=np.int32)


def _arrays_store(dev, dt_, dw, ds, dn):
    """What ``postings.search`` reads of a store, over arrays that were never ``add``-ed (tombstones that keep their entries)."""
    from tensor_truth_amd.lexical import LexicalStore

    return SimpleNamespace(terms=_t(dt_, dev), weights=_t(dw, dev), d_start=_t(ds, dev), d_nnz=_t(dn, dev), n_docs=len(dn), index=None,
                           _pws=None, _ws=None, _check_query=LexicalStore._check_query, stats={})


@pytest.mark.parametrize("n_q", [1, 3, 64])
@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 63, 64, 65, 1000, SPAN + 1, 2 * SPAN + 1])
def test_search_through_the_lists_equals_the_scan(dev, built_lib, n_docs, n_q):
    from tensor_truth_amd import lexical
    from tensor_truth_amd import postings as P

    assert P.SPAN == SPAN
    qt, qw, qs, qn, dt_, dw, ds, dn = _scan_inputs(n_docs, n_q, 31 * n_docs + n_q)
    store = _arrays_store(dev, dt_, dw, ds, dn)
    lw = lexical.LexicalWeights(_t(qt, dev), _t(qw, dev), qs.astype(np.int64), qn)
    want = {k: tuple(v.cpu().numpy() for v in lexical.lexical_scan_topk(lw.terms, lw.weights, qs, qn, store.terms, store.weights, ds, dn,
                                                                        k=k)) for k in (1, 10, 64, 65, 1024)}
    full = lexical.lexical_score(lw.terms, lw.weights, qs, qn, store.terms, store.weights, ds, dn)[0].cpu().numpy()
    zeros = int((want[1024][0] == 0).sum())
    q_lists = [qt[s:s + n] for s, n in zip(qs, qn)]
    seen = []
    for n_sealed in sorted({0, n_docs} | {n_docs - t for t in (1, 37, n_docs // 2) if 0 < t <= n_docs}):
        store.index = P.postings_build(store.terms, store.weights, store.d_start, store.d_nnz, n_sealed, VOCAB, len(dt_))
        ref_lists = R.reference_postings(dt_, dw, ds, dn, n_sealed, VOCAB)[1]
        union = np.asarray([len(np.unique(np.concatenate([ref_lists[t] for t in ids]))) for ids in q_lists]) + (n_docs - n_sealed)
        # the entry point alone, every list of every query: an ascending candidate list of exactly the union and the tail
        s, i, thr, cnt, cc, _ = P.lexical_topk_postings(lw.terms, lw.weights, qs, qn, store.terms, store.weights, store.d_start,
                                                        store.d_nnz, store.index, P.ranges_of(q_lists, store.index.off_host), 1024)
        assert cc.cpu().numpy().tolist() == union.tolist(), f"n_sealed {n_sealed}: candidates are not the union of the lists + the tail"
        s, i, thr, cnt = s.cpu().numpy(), i.cpu().numpy(), thr.cpu().numpy(), cnt.cpu().numpy()
        for a in range(n_q):
            cand = np.union1d(np.concatenate([ref_lists[t] for t in q_lists[a]]), np.arange(n_sealed, n_docs)).astype(np.int64)
            cand = cand[dn[cand] >= 0]
            order = cand[np.argsort(-full[a, cand], kind="stable")][:1024]        # (score desc, document asc) over the candidates
            m = len(order)
            assert i[a, :m].tolist() == order.tolist() and s[a, :m].tobytes() == full[a, order].tobytes(), f"n_sealed {n_sealed} query {a}"
            assert (i[a, m:] == -1).all() and np.isneginf(s[a, m:]).all() and cnt[a] == m
            assert thr[a].tobytes() == (full[a, order[-1]] if m == 1024 else np.float32(-np.inf)).tobytes()
        for k, (want_s, want_i) in want.items():
            got_s, got_i = (v.cpu().numpy() for v in P.search(store, lw, k))
            assert (got_i == want_i).all(), f"n_docs {n_docs} n_sealed {n_sealed} k {k}: indices"
            assert got_s.tobytes() == want_s.tobytes(), f"n_docs {n_docs} n_sealed {n_sealed} k {k}: scores"
            seen.append((n_sealed, k, store.stats["passes"], store.stats["fallbacks"], store.stats["candidates"]))
    assert n_docs < 1000 or any(f == 0 for _, k, _, f, _ in seen if k == 1), "no search was answered from the lists alone"
    assert n_docs != 1000 or all(f == n_q for _, k, _, f, _ in seen if k == 1024), "k beyond the store: every query falls back"
    print(f"\npostings n_docs {n_docs} n_q {n_q}: {zeros} zero scores in the scan's top 1024; (n_sealed, k, passes, fallbacks, candidates) "
          f"{seen[:3]} .. {seen[-3:]}")


# ---- the stores --------------------------------------------------------------------------------------------------------------------
def _lw(dev, entries):
    """[{id: weight}] -> LexicalWeights on the device."""
    from tensor_truth_amd.lexical import LexicalWeights

    ids = [np.asarray(sorted(e), dtype=np.int32) for e in entries]
    t, st, nn = _pack(ids, np.int32)
    w = _pack([[e[int(i)] for i in row] for e, row in zip(entries, ids)], np.float32)[0]
    pad = lambda a: a if len(a) else np.zeros(0, dtype=a.dtype)  # noqa: E731
    return LexicalWeights(_t(pad(t), dev), _t(pad(w), dev), st, nn)


def _same(a, b, what):
    (sa, ia), (sb, ib) = a, b
    assert (ia.cpu().numpy() == ib.cpu().numpy()).all(), f"{what}: indices"
    assert sa.cpu().numpy().tobytes() == sb.cpu().numpy().tobytes(), f"{what}: scores"


def _random_docs(rng, n, ids=np.arange(10, 300)):
    return [{int(t): float(rng.integers(1, 5)) * 0.25 for t in rng.choice(ids, int(rng.integers(0, 9)), replace=False)} for _ in range(n)]


@pytest.mark.parametrize("kind", ["splade", "lexical"])
def test_store_with_postings_equals_the_store_without(dev, built_lib, kind):
    from tensor_truth_amd.lexical import LexicalStore
    from tensor_truth_amd.splade import SpladeStore

    rng = np.random.default_rng(17)
    if kind == "splade":
        make = lambda **kw: SpladeStore(dev, **kw)  # noqa: E731
        add = lambda st, ids, lw: st.add(ids, lw)  # noqa: E731
    else:
        make = lambda **kw: LexicalStore(128, dev, **kw)  # noqa: E731
        add = lambda st, ids, lw: st.add(ids, lw, torch.zeros(len(ids), 128))  # noqa: E731
    with pytest.raises(ValueError, match="vocab_size"):
        make(postings=True)
    on, off = make(postings=True, vocab_size=VOCAB), make()
    with pytest.raises(RuntimeError, match="postings=True"):
        off.seal()
    docs = _random_docs(rng, 300)
    queries = _lw(dev, [{int(t): 1.0 for t in rng.choice(np.arange(10, 300), 4, replace=False)} for _ in range(5)]
                  + [{500: 1.0, 501: 2.0}, {VOCAB + 40: 1.0, 5: 0.5}])     # ids with no list; ids outside the vocabulary
    for st in (on, off):
        add(st, [f"d{i}" for i in range(200)], _lw(dev, docs[:200]))
    assert on.index is None and on.n_sealed == 0
    _same(on.search(queries, 10), off.search(queries, 10), "before seal(): the full scan")
    assert on.stats == {}
    before = on.nbytes
    on.seal()
    assert on.n_sealed == 200 and on.nbytes == before + on.index.nbytes and on.index.nbytes == 12 * VOCAB + 8 + 4 * on.n_terms
    for st in (on, off):
        add(st, [f"d{i}" for i in range(200, 300)], _lw(dev, docs[200:]))                    # the tail
        assert st.remove("d7") and st.remove("d150") and st.remove("d250") and not st.remove("d250")   # sealed, sealed, in the tail
        add(st, ["d7", "d260"], _lw(dev, [docs[150], docs[3]]))                              # re-added ids: new copies in the tail
    assert on.n_sealed == 200 and on.n_docs == 302 and len(on) == len(off) == 298
    fallbacks = {}
    for k in (1, 10, 50, 400):
        want = off.search(queries, k)
        _same(on.search(queries, k), want, f"{kind} k {k}")
        assert on.stats["documents"] == 302 and on.stats["queries"] == 7 and on.stats["sealed"] == 200
        # a query falls back exactly when the scan's own k-th best score is not above zero
        fallbacks[k] = on.stats["fallbacks"]
        assert fallbacks[k] == int((~(want[0][:, k - 1].cpu().numpy() > 0)).sum()), on.stats
    assert fallbacks[1] == 2 and fallbacks[400] == 7, "the two queries without a list always fall back; k beyond the store: all do"
    got = on.search(queries, 10)[1].cpu().numpy()
    assert not np.isin(got, [7, 150, 250, 260]).any(), "a tombstone was returned"
    with pytest.raises(ValueError, match="outside the vocabulary"):
        add(on, ["x"], _lw(dev, [{VOCAB: 1.0}]))
    assert on.n_docs == 302
    on.seal()
    assert on.n_sealed == 302
    _same(on.search(queries, 10), off.search(queries, 10), "after a second seal()")
    # a query that shares no id with any document: the full scan answers it -- the first k live documents at score 0
    nothing = _lw(dev, [{550: 1.0}, {551: 3.0, VOCAB + 1: 1.0}])
    s, i = on.search(nothing, 5)
    _same((s, i), off.search(nothing, 5), "no shared id")
    live = [d for d in range(302) if on.node_id(d) is not None][:5]
    assert i.cpu().numpy().tolist() == [live, live] and (s.cpu().numpy() == 0).all()
    assert on.stats["fallbacks"] == 2 and on.stats["candidates"] == 0 and on.stats["passes"] == 1, on.stats


def test_a_store_without_dense_rows_is_the_same_store(dev, built_lib):
    """``LexicalStore`` with ``dim`` 0, ``SpladeStore`` and ``LexicalStore`` with dense rows hold the same CSR arrays and give the
    same lexical scores; only the dense array, what ``add`` takes and ``nbytes`` differ.  Capacity 1, documents of 1 and 0
    entries: every array grows."""
    from tensor_truth_amd.lexical import LexicalStore
    from tensor_truth_amd.splade import SpladeStore

    docs = [{11: 2.0}, {}, {11: 0.5, 12: 1.0}]
    q = _lw(dev, [{11: 1.0, 12: 3.0}])
    cand = np.arange(3, dtype=np.int32)[None]
    plain, bare, dense = SpladeStore(dev, 1, 1), LexicalStore(0, dev, 1, 1), LexicalStore(128, dev, 1, 1)
    for st in (plain, bare):
        assert st.dense is None and st.dim == 0 and st.nbytes == 8 + 12
        with pytest.raises(ValueError, match="dense rows are not taken"):
            st.add(["a"], _lw(dev, docs[:1]), torch.zeros(1, 128))
        assert st.add(["a", "b"], _lw(dev, docs[:2])).tolist() == [0, 1] and st.add(["c"], _lw(dev, docs[2:])).tolist() == [2]
        assert st.nbytes == 8 * 4 + 12 * 4, "capacity doubles: 4 entries, 4 documents, no dense rows"
    assert dense.nbytes == 8 + 12 + 256
    with pytest.raises(ValueError, match="dense rows are needed"):
        dense.add(["a"], _lw(dev, docs[:1]))
    dense.add(["a", "b"], _lw(dev, docs[:2]), torch.ones(2, 128))
    dense.add(["c"], _lw(dev, docs[2:]), torch.ones(1, 128))
    assert dense.nbytes == 8 * 4 + (12 + 256) * 4
    want = [[2.0, 0.0, 3.5]]
    assert plain.score(q, cand).cpu().tolist() == want
    for st in (bare, dense):
        lex, none_d, none_h = st.score(q, cand)
        assert lex.cpu().tolist() == want and none_d is None and none_h is None
        assert all(torch.equal(getattr(st, a)[:n], getattr(plain, a)[:n]) for a, n in (("terms", 3), ("weights", 3), ("d_start", 3), ("d_nnz", 3)))
    lex, dn, hy = dense.score(q, cand, dense=torch.ones(1, 128), hybrid_weights=(1.0, 1.0))
    assert lex.cpu().tolist() == want and dn.cpu().tolist() == [[128.0] * 3] and hy.cpu().tolist() == [[65.0, 64.0, 65.75]]
    # tombstones: a re-added id buries its older copy, remove writes d_nnz = -1
    for st in (plain, bare, dense):
        st.add(["a"], _lw(dev, docs[2:]), *([torch.ones(1, 128)] if st.dim else []))
        assert st.remove("b") and not st.remove("b") and len(st) == 2
        assert st.d_nnz[:4].cpu().tolist() == [-1, -1, 2, 2] and st.lookup(["a", "b", "c"]).tolist() == [3, -1, 2]
        assert [st.node_id(d) for d in range(5)] == [None, None, "c", "a", None]
        assert st.search(q, 4)[1].cpu().tolist() == [[2, 3, -1, -1]]


def test_add_reseals_once_the_tail_outgrows_the_lists(dev, built_lib):
    from tensor_truth_amd.splade import SpladeStore

    st = SpladeStore(dev, postings=True, vocab_size=VOCAB)
    one = _lw(dev, [{10 + (i % 50): 1.0} for i in range(32768)])
    st.add([("a", i) for i in range(32768)], one)
    st.add([("b", i) for i in range(32768)], one)
    assert st.index is None and st.n_docs == 65536, "a tail of 65536 is not yet beyond max(65536, n_sealed / 4)"
    st.add([("c", 0)], _lw(dev, [{11: 2.0}]))
    assert st.n_sealed == 65537, "the tail outgrew 65536: sealed inside add"
    st.add([("d", i) for i in range(32768)], one)
    assert st.n_sealed == 65537 and st.n_docs == 98305
    q = _lw(dev, [{11: 1.0}])
    s, i = st.search(q, 3)
    assert i.cpu().numpy().tolist() == [[65536, 1, 51]] and s.cpu().numpy().tolist() == [[2.0, 1.0, 1.0]]
    assert st.stats["candidates"] == 2 * 656 + 1 + 32768 and st.stats["fallbacks"] == 0, st.stats


# ---- pruning is both safe and real ------------------------------------------------------------------------------------------------
def _pruning_stores(dev, docs, n_sealed=None):
    from tensor_truth_amd.splade import SpladeStore

    on, off = SpladeStore(dev, postings=True, vocab_size=VOCAB), SpladeStore(dev)
    n_sealed = len(docs) if n_sealed is None else n_sealed
    for st in (on, off):
        st.add(list(range(n_sealed)), _lw(dev, docs[:n_sealed]))
    on.seal()
    if n_sealed < len(docs):
        for st in (on, off):
            st.add(list(range(n_sealed, len(docs))), _lw(dev, docs[n_sealed:]))
    return on, off


def test_a_short_heavy_list_prunes_a_long_light_one(dev, built_lib):
    # id 10 in 20 documents at 2.0, id 11 in all 1000 at 0.01; the query holds both at 1.0
    heavy = set(range(3, 1000, 50))
    assert len(heavy) == 20 and max(heavy) < 960
    docs = [({10: 2.0, 11: 0.01} if d in heavy else {11: 0.01}) for d in range(1000)]
    q = _lw(dev, [{10: 1.0, 11: 1.0}])
    on, off = _pruning_stores(dev, docs)
    _same(on.search(q, 10), off.search(q, 10), "k 10")
    assert on.stats == {"queries": 1, "candidates": 20, "documents": 1000, "passes": 1, "fallbacks": 0, "sealed": 1000}
    assert on.search(q, 10)[1].cpu().numpy().tolist() == [sorted(heavy)[:10]]
    # k = 50: theta comes from documents that hold only id 11 -- its bound is not below theta, nothing is pruned, and the equal
    # scores come out by document number as the scan has them
    _same(on.search(q, 50), off.search(q, 50), "k 50")
    assert on.stats["candidates"] == 1000 and on.stats["passes"] == 1 and on.stats["fallbacks"] == 0, on.stats
    light = [d for d in range(1000) if d not in heavy][:30]
    assert on.search(q, 50)[1].cpu().numpy().tolist() == [sorted(heavy) + light]
    # with a tail, the tail is scored whole beside the 20
    on, off = _pruning_stores(dev, docs, n_sealed=960)
    _same(on.search(q, 10), off.search(q, 10), "k 10 with a tail")
    assert on.stats["candidates"] == 20 + 40 and on.stats["passes"] == 1 and on.stats["fallbacks"] == 0, on.stats
    # a negative stored weight: the index is not prunable, every list is taken
    docs[500] = {11: 0.01, 12: -1.0}
    on, off = _pruning_stores(dev, docs)
    assert not on.index.prunable
    _same(on.search(q, 10), off.search(q, 10), "not prunable")
    assert on.stats["candidates"] == 1000 and on.stats["fallbacks"] == 0
    # a negative query weight through the same store: scores below zero exist, only the scan can answer
    qn = _lw(dev, [{10: 1.0, 11: -1.0}])
    _same(on.search(qn, 30), off.search(qn, 30), "negative query weight")
    assert on.stats["fallbacks"] == 1


@pytest.mark.parametrize("case", ["under", "over"])
def test_two_hundred_light_ids_just_under_and_just_over_theta(dev, built_lib, case):
    """theta = 2.0 (ten documents that hold id 10 at 2.0 and nothing else).  200 light ids, each in four documents of its own: 199
    with bound 2^-7 and one with bound v, all multiples of 2^-10, so the fp64 sum is exact: 2 - 2^-10 (under) or 2 (over).  Under:
    (2 - 2^-10) (1 + 412 2^-24) < 2, all 200 are pruned and only id 10's 20 documents are scored.  Over: the sum itself is not
    below theta, so the id that tips it is scored in a second pass (its four documents beside the 20); the 199 before it stay
    pruned.  Both equal the scan."""
    from tensor_truth_amd import postings as P

    v = 455 * 2.0 ** -10 + (2.0 ** -10 if case == "over" else 0.0)
    bounds = [2.0 ** -7] * 199 + [v]
    assert sum(bounds) == (2.0 if case == "over" else 2.0 - 2.0 ** -10)
    docs = [{10: 2.0} for _ in range(20)]
    for j, b in enumerate(bounds):
        docs += [{100 + j: b * (1.0 if r == 0 else 0.5)} for r in range(4)]
    docs += [{} for _ in range(1000 - len(docs))]
    q = _lw(dev, [{10: 1.0, **{100 + j: 1.0 for j in range(200)}}])
    on, off = _pruning_stores(dev, docs)
    c = P.term_bounds(np.arange(100, 300), np.ones(200, dtype=np.float32), on.index.ub_host, VOCAB)
    assert float(np.sum(c)) == sum(bounds) and (float(P.upper_bound(c)) < 2.0) == (case == "under")
    _same(on.search(q, 10), off.search(q, 10), case)
    assert on.search(q, 10)[0].cpu().numpy().tolist() == [[2.0] * 10]
    want = {"under": (20, 1), "over": (20 + 20 + 4, 2)}[case]
    assert (on.stats["candidates"], on.stats["passes"]) == want and on.stats["fallbacks"] == 0, on.stats


# ---- the retrievers ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_texts(name):
    z = np.load(os.path.join(GOLDEN, f"{name}_expected.npz"))
    n_q = int(z["n_queries"])
    texts = [str(t) for t in z["texts"]]
    return texts[:n_q], texts[n_q:], (int(z["max_length"]) if "max_length" in z.files else None)


def _nodes(passages):
    from tensor_truth_amd.schema import NodeWithScore, TextNode

    return [NodeWithScore(node=TextNode(text=t, id_=f"p{i}"), score=0.0) for i, t in enumerate(passages)]


def _hits(retr, q):
    return [(n.node.id_, n.score) for n in retr.retrieve(q)]


def test_splade_retriever_with_postings_returns_the_same_nodes_and_scores(dev, built_lib):
    from tensor_truth_amd.splade import HipSpladeRetriever

    queries, passages, max_length = _fixture_texts("splade_l2")
    make = lambda **kw: HipSpladeRetriever(model=SPLADE, similarity_top_k=6,  # noqa: E731
                                           model_kwargs=dict({"torch_dtype": "bfloat16", "max_length": max_length}, **kw))
    on, off = make(postings=True), make()
    assert on.store.postings and on.store.vocab_size == on.config.vocab_size and not off.store.postings
    for r in (on, off):
        r.index_nodes(_nodes(passages))
    for q in queries:
        a, b = _hits(on, q), _hits(off, q)
        assert a == b and len(a) > 0, "postings on and off return different nodes or scores"
    assert on.store.index is not None and on.store.n_sealed == len(passages) and on.store.stats["passes"] >= 1 and off.store.index is None
    on.index_nodes(_nodes(passages[:3]))            # re-added ids: tombstones on the lists, new copies in the tail
    off.index_nodes(_nodes(passages[:3]))
    best = _hits(off, queries[0])[0][0]
    assert on.remove_node(best) and off.remove_node(best)
    for q in queries:
        assert _hits(on, q) == _hits(off, q)
    assert on.store.n_sealed == len(passages) and on.store.n_docs == len(passages) + 3


def test_lexical_retriever_with_postings_returns_the_same_nodes_and_scores(dev, built_lib):
    from tensor_truth_amd import lexical
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    queries, passages, _ = _fixture_texts("m3_l2")
    emb = HipHuggingFaceEmbedding(model_name=M3, device="cuda:0", model_kwargs={"precision": "bf16"})
    make = lambda **kw: lexical.HipM3HybridRerank(model=M3, top_n=24,  # noqa: E731
                                                  model_kwargs=dict({"hybrid_weights": (0.4, 0.2), "embedder": emb}, **kw))
    on, off = make(postings=True), make()
    assert on.store.postings and on.store.vocab_size == emb.config.vocab_size and not off.store.postings
    for r in (on, off):
        assert r.index_nodes(_nodes(passages)) == len(passages)
    r_on, r_off = lexical.HipLexicalRetriever(on, similarity_top_k=10), lexical.HipLexicalRetriever(off, similarity_top_k=10)
    for q in queries:
        a, b = _hits(r_on, q), _hits(r_off, q)
        assert a == b and len(a) > 0, "postings on and off return different nodes or scores"
    assert on.store.index is not None and on.store.n_sealed == len(passages) and off.store.index is None
    best = _hits(r_off, queries[0])[0][0]
    assert on.remove_node(best) and off.remove_node(best)
    assert _hits(r_on, queries[0]) == _hits(r_off, queries[0]) and best not in [h[0] for h in _hits(r_on, queries[0])]
