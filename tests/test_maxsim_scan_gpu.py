"""GPU: exact MaxSim retrieval over the whole token store (``tt_maxsim_scan_topk[_f16]``, ``TokenVectorStore.search``,
``HipColbertRetriever``).

One sentence is the acceptance test: whatever the scan returns equals ``tt_maxsim``'s own scores with ``cand == NULL`` for the same
operands, sorted on the host by (score descending, document number ascending) and padded with (-inf, -1) -- ``torch.equal`` on
scores and on numbers.  ``tt_maxsim`` is itself held to fp64 by tests/test_colbert_gpu.py; one configuration here holds the
returned scores to that fp64 bound directly.

The shapes are the smallest at which the scan kernel can go wrong: every dim it is instantiated for, document lengths around the
16-row tile and at both limits, query lengths around the 16-row block and at the limit, k on both select kernels and past the
store, more documents than one sweep of the persistent grid holds (a wave takes CHUNK = 2 consecutive documents per step, four
waves per workgroup, two workgroups per compute unit: 4096 documents on 256 compute units), stores smaller than one workgroup's
first step, and query batches that need more than one LDS pass (16 blocks of 16 query rows per pass).
"""
import os

import numpy as np
import pytest
import torch

from test_colbert_gpu import (_DT, _IDS, LAYOUTS, _check_scores, _maxsim_reference, _packed, _text, expected)  # noqa: F401

pytestmark = pytest.mark.gpu

CHUNK = 2                                   # colbert.hip kScanChunk
D_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 180, 511, 512]
Q_LENS = [1, 15, 16, 17, 32, 33, 128]
NEG_INF = float("-inf")


def _host_topk(scores: np.ndarray, k: int, alive=None):
    """The expected output for dense fp32 ``scores`` [n_q][n_docs]: (score descending, number ascending), padded."""
    n_q, n_docs = scores.shape
    out_s = np.full((n_q, k), -np.inf, dtype=np.float32)
    out_i = np.full((n_q, k), -1, dtype=np.int32)
    live = np.arange(n_docs) if alive is None else np.flatnonzero(np.asarray(alive) != 0)
    for a in range(n_q):
        s = scores[a, live]
        order = np.lexsort((live, -s))[:k]
        out_s[a, :len(order)] = s[order]
        out_i[a, :len(order)] = live[order]
    return torch.from_numpy(out_s), torch.from_numpy(out_i)


def _assert_scan_equals_rerank(q, qs, ql, d, ds, dl, ks, alive=None, what=""):
    """The acceptance sentence, for every k of ``ks`` -> the dense rerank scores (host)."""
    from tensor_truth_amd import colbert

    dense = colbert.maxsim(q, qs.astype(np.int32), ql, d, ds, dl).cpu().numpy()
    for k in ks:
        got_s, got_i = colbert.maxsim_scan_topk(q, qs.astype(np.int32), ql, d, ds, dl, k, alive=alive)
        want_s, want_i = _host_topk(dense, k, alive)
        assert got_s.shape == (len(ql), k) and got_i.dtype == torch.int32
        assert torch.equal(got_i.cpu(), want_i), f"{what} k={k}: document numbers differ"
        assert torch.equal(got_s.cpu(), want_s), f"{what} k={k}: scores differ from tt_maxsim's bits"
    return dense


def _scan_all(q, qs, ql, d, ds, dl, alive=None):
    """Every score the scan computes, as a dense host matrix (k = n_docs; a number that is not returned stays NaN)."""
    from tensor_truth_amd import colbert

    n = len(dl)
    s, i = colbert.maxsim_scan_topk(q, qs.astype(np.int32), ql, d, ds, dl, n, alive=alive)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    out = np.full((len(ql), n), np.nan, dtype=np.float32)
    for a in range(len(ql)):
        keep = i[a] >= 0
        out[a, i[a][keep]] = s[a][keep]
    return out


# ---- 1. bit equality with the rerank kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("n_q", [1, 3])
@pytest.mark.parametrize("dim", [32, 64, 96, 128])
def test_scan_returns_the_rerank_kernels_bits(dev, built_lib, dim, n_q, dt):
    from tensor_truth_amd import colbert

    gen = torch.Generator(device=dev).manual_seed(500 + dim + n_q)
    d, ds, dl = _packed((D_LENS * 4)[:40], dim, dt, dev, gen)
    n_docs = len(dl)
    for qlens in ([[n] for n in Q_LENS] if n_q == 1 else [[1, 15, 16], [17, 32, 33], [128, 16, 1]]):
        q, qs, ql = _packed(qlens, dim, dt, dev, gen)
        dense = _assert_scan_equals_rerank(q, qs, ql, d, ds, dl, [1, 10, 64, 65, n_docs + 3], what=f"dim {dim} q_len {qlens} {dt}")
    assert (dense[:, 0] == 0).all(), "a document of length 0 scores 0"
    if dim == 128 and n_q == 3:
        # the returned scores against fp64 directly, with tests/test_colbert_gpu.py's bound (padding: -inf for candidate -1)
        got_s, got_i = colbert.maxsim_scan_topk(q, qs.astype(np.int32), ql, d, ds, dl, n_docs + 3)
        want, bound = _maxsim_reference(q, qs, ql, d, ds, dl, got_i.cpu().numpy())
        _check_scores(got_s, want, bound, f"scan dim {dim} q_len {qlens} {dt} vs fp64")


# ---- 2. the persistent walk wraps ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("n_docs", [6000, 1, CHUNK + 1, 4 * CHUNK + 1])
def test_the_walk_wraps_and_ragged_ends(dev, built_lib, n_docs, dt):
    """6000 documents are more than one sweep of the grid holds, so every wave takes several chunks; 1, 3 (one chunk + 1) and 9
    (one workgroup's first step + 1) leave waves idle and end on a ragged chunk."""
    dim = 64
    gen = torch.Generator(device=dev).manual_seed(n_docs)
    rng = np.random.default_rng(n_docs)
    d, ds, dl = _packed(rng.integers(1, 41, n_docs), dim, dt, dev, gen)
    q, qs, ql = _packed([32, 17], dim, dt, dev, gen)
    _assert_scan_equals_rerank(q, qs, ql, d, ds, dl, [50], what=f"{n_docs} documents {dt}")


# ---- 3. constructed traps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", _DT, ids=_IDS)
def test_negative_maxima_document_ends_and_layout(dev, built_lib, dt):
    """tests/test_colbert_gpu.py's two traps through the scan -- a document whose every row is -q_5 (a maximum started at 0 is
    caught), a document followed in memory by one whose first row is a query row (a read past d_len is caught) -- and the same
    store laid out in reverse order behind filler rows, with a non-zero first d_start."""
    dim = 96
    gen = torch.Generator(device=dev).manual_seed(7)
    q, qs, ql = _packed([17], dim, dt, dev, gen)
    neg = (-q[5]).repeat(16, 1)
    body, _, _ = _packed([15], dim, dt, dev, gen)
    nxt = torch.cat([q[9:10], _packed([7], dim, dt, dev, gen)[0]])
    d = torch.cat([neg, body, nxt]).contiguous()
    ds, dl = np.array([0, 16, 31], dtype=np.int64), np.array([16, 15, 8], dtype=np.int32)
    _assert_scan_equals_rerank(q, qs, ql, d, ds, dl, [1, 3, 5], what=f"constructed {dt}")
    got = _scan_all(q, qs, ql, d, ds, dl)
    cand = np.arange(3, dtype=np.int32)[None]
    want, bound = _maxsim_reference(q, qs, ql, d, ds, dl, cand)
    _check_scores(torch.from_numpy(got), want, bound, f"scan constructed {dt}")
    Q, D0 = q.double().cpu(), neg.double().cpu()
    from_zero = (Q @ D0.T).max(-1).values.clamp_min(0).sum()
    assert abs(from_zero - want[0, 0]) > 100 * bound[0, 0] and abs(float(got[0, 0]) - from_zero) > bound[0, 0]
    past, _ = _maxsim_reference(q, qs, ql, d, ds, np.array([16, 16, 8], dtype=np.int32), cand)
    assert abs(past[0, 1] - want[0, 1]) > 100 * bound[0, 1] and abs(float(got[0, 1]) - past[0, 1]) > bound[0, 1]

    # the same documents at other offsets of a store
    dim = 128
    q, qs, ql = _packed([32, 5, 128], dim, dt, dev, gen)
    d, ds, dl = _packed([180, 33, 512, 1, 64], dim, dt, dev, gen)
    fwd = _scan_all(q, qs, ql, d, ds, dl)
    order = [4, 3, 2, 1, 0]
    d2 = torch.cat([torch.ones(3, dim, dtype=dt, device=dev)] + [d[ds[c]:ds[c] + dl[c]] for c in order]).contiguous()
    dl2 = dl[order]
    ds2 = 3 + np.concatenate([[0], np.cumsum(dl2[:-1])]).astype(np.int64)
    moved = _scan_all(q, qs, ql, d2, ds2, dl2)
    assert not np.isnan(fwd).any() and np.array_equal(moved, fwd[:, order])
    _assert_scan_equals_rerank(q, qs, ql, d2, ds2, dl2, [5], what=f"reverse layout {dt}")


# ---- 4. batch and pass invariance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("n_q", [9, 64])
def test_a_query_scores_the_same_alone_and_in_any_pass(dev, built_lib, n_q, dt):
    """One 32-token query alone, then at positions 0 and 8 of a batch whose other queries hold 128 tokens: two of those fill an LDS
    pass at dim 128, so the copies are scored by different passes, beside different neighbours."""
    from tensor_truth_amd import colbert

    dim = 128
    gen = torch.Generator(device=dev).manual_seed(40 + n_q)
    d, ds, dl = _packed([180, 33, 512, 1, 64, 0, 17, 16, 300, 31, 2], dim, dt, dev, gen)
    one, _, _ = _packed([32], dim, dt, dev, gen)
    k = len(dl)
    alone = colbert.maxsim_scan_topk(one, np.zeros(1, np.int32), np.array([32], np.int32), d, ds, dl, k)
    qlens = [128] * n_q
    qlens[0] = qlens[8] = 32
    q, qs, ql = _packed(qlens, dim, dt, dev, gen)
    for at in (0, 8):
        q[qs[at]:qs[at] + 32] = one
    got_s, got_i = colbert.maxsim_scan_topk(q, qs.astype(np.int32), ql, d, ds, dl, k)
    for at in (0, 8):
        assert torch.equal(got_s[at], alone[0][0]) and torch.equal(got_i[at], alone[1][0]), f"position {at} of {n_q}"
    _assert_scan_equals_rerank(q, qs, ql, d, ds, dl, [3], what=f"batch of {n_q} {dt}")


# ---- 5. ties and tombstones ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", _DT, ids=_IDS)
def test_ties_and_tombstones(dev, built_lib, dt):
    from tensor_truth_amd import colbert

    dim = 64
    gen = torch.Generator(device=dev).manual_seed(5)
    lens = [20, 9, 0, 33, 16, 5, 40, 33, 12, 1, 17, 33, 8, 25]
    d, ds, dl = _packed(lens, dim, dt, dev, gen)
    for c in (7, 11):                                                    # documents 3, 7 and 11 are one passage
        d[ds[c]:ds[c] + 33] = d[ds[3]:ds[3] + 33]
    q, qs, ql = _packed([32, 16], dim, dt, dev, gen)
    q[:20] = d[ds[3]:ds[3] + 20]                                         # ... which query 0 is cut from: it ranks first
    n = len(lens)
    qs32 = qs.astype(np.int32)
    s, i = colbert.maxsim_scan_topk(q, qs32, ql, d, ds, dl, n)
    assert i[0, :3].tolist() == [3, 7, 11] and s[0, 0] == s[0, 1] == s[0, 2]
    row = i[1].tolist()
    assert [row[row.index(3) + j] for j in range(3)] == [3, 7, 11], "equal scores: adjacent, in ascending number"
    # a zero-length live document is a valid result with score 0 once k reaches it
    at = row.index(2)
    assert s[1, at].item() == 0.0 and sorted(row) == list(range(n))
    # alive NULL = all ones
    ones = np.ones(n, dtype=np.uint8)
    s1, i1 = colbert.maxsim_scan_topk(q, qs32, ql, d, ds, dl, n, alive=ones)
    assert torch.equal(s1, s) and torch.equal(i1, i)
    # alive[7] = 0 removes 7 and only 7
    alive = ones.copy()
    alive[7] = 0
    _assert_scan_equals_rerank(q, qs, ql, d, ds, dl, [1, 5, n], alive=alive, what=f"tombstone {dt}")
    s7, i7 = colbert.maxsim_scan_topk(q, qs32, ql, d, ds, dl, n, alive=torch.from_numpy(alive).to(dev))
    assert i7[0, :2].tolist() == [3, 11] and sorted(i7[0].tolist()) == [-1] + [x for x in range(n) if x != 7]
    assert s7[0, -1].item() == NEG_INF
    # all dead: every output is the padding
    s0, i0 = colbert.maxsim_scan_topk(q, qs32, ql, d, ds, dl, 4, alive=np.zeros(n, dtype=np.uint8))
    assert (s0 == NEG_INF).all() and (i0 == -1).all()
    # an empty store pads without a scoring launch
    se, ie = colbert.maxsim_scan_topk(q, qs32, ql, d, np.zeros(0, np.int64), np.zeros(0, np.int32), 4)
    assert (se == NEG_INF).all() and (ie == -1).all()


# ---- 6. refusals before a launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["", "_f16"])
def test_refusals_come_before_a_launch(dev, built_lib, sfx):
    from tensor_truth_amd import _lib, colbert

    lib = _lib.load_library()
    fn = getattr(lib, "tt_maxsim_scan_topk" + sfx)
    dt = torch.float16 if sfx else torch.bfloat16
    v = torch.zeros(64, 128, dtype=dt, device=dev)
    i32 = torch.ones(8, dtype=torch.int32, device=dev)                    # lengths: 1
    z32 = torch.zeros(8, dtype=torch.int32, device=dev)                   # starts: 0
    i64 = torch.zeros(8, dtype=torch.int64, device=dev)
    out_s = torch.full((8,), 7.0, dtype=torch.float32, device=dev)
    out_i = torch.full((8,), 7, dtype=torch.int32, device=dev)
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev)

    def call(n_q=1, dim=128, k=2, ws_bytes=4096, outs=True):
        return fn(v.data_ptr(), z32.data_ptr(), i32.data_ptr(), n_q, v.data_ptr(), i64.data_ptr(), i32.data_ptr(), None, 4, dim, k,
                  out_s.data_ptr() if outs else None, out_i.data_ptr() if outs else None, ws.data_ptr(), ws_bytes, None)

    assert call(dim=48) == -2 and b"dim=48" in lib.tt_last_error()
    assert call(dim=160) == -2 and b"dim=160" in lib.tt_last_error()
    assert call(n_q=0) == -2 and b"n_q=0" in lib.tt_last_error()
    assert call(n_q=65) == -2
    assert call(k=0) == -2 and call(k=1025) == -2 and b"k=1025" in lib.tt_last_error()
    assert call(ws_bytes=8) == -3 and b"workspace" in lib.tt_last_error()
    assert call(outs=False) == -1 and b"null output" in lib.tt_last_error()
    torch.cuda.synchronize()
    assert (out_s == 7.0).all() and (out_i == 7).all(), "a refused call wrote its outputs"
    assert lib.tt_maxsim_scan_workspace_bytes(1000, 3) >= 3 * 1024 * 4 and lib.tt_maxsim_scan_workspace_bytes(-1, 3) == 0
    assert call() == 0                                                        # the same arguments, unrefused, run
    torch.cuda.synchronize()
    # the host wrapper holds the lengths: one outside the kernel's range is refused
    q = torch.zeros(200, 128, dtype=dt, device=dev)
    d = torch.zeros(600, 128, dtype=dt, device=dev)
    with pytest.raises(ValueError, match="q_len"):
        colbert.maxsim_scan_topk(q, [0], [129], d, [0], [16], 1)
    with pytest.raises(ValueError, match="d_len"):
        colbert.maxsim_scan_topk(q, [0], [32], d, [0], [513], 1)
    with pytest.raises(ValueError, match="queries"):
        colbert.maxsim_scan_topk(q, [0] * 65, [1] * 65, d, [0], [16], 1)
    with pytest.raises(ValueError, match="k=1025"):
        colbert.maxsim_scan_topk(q, [0], [32], d, [0], [16], 1025)
    with pytest.raises(ValueError, match="alive"):
        colbert.maxsim_scan_topk(q, [0], [32], d, [0], [16], 1, alive=np.ones(2, dtype=np.uint8))


# ---- 7. through the surface, on the committed fixture ----------------------------------------------------------------------------
def _all_ranked(rr, nodes, query):
    top_n, rr.top_n = rr.top_n, len(nodes)
    try:
        return [(n.node.id_, n.score) for n in rr.postprocess_nodes(nodes, query_str=query)]
    finally:
        rr.top_n = top_n


@pytest.mark.parametrize("dtype", _IDS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_retriever_returns_the_rerank_ranking_over_the_fixture(dev, built_lib, expected, layout, dtype):
    from tensor_truth_amd.colbert import HipColbertRerank, HipColbertRetriever
    from tensor_truth_amd.schema import NodeWithScore, QueryBundle, TextNode

    rr = HipColbertRerank(model=LAYOUTS[layout], top_n=5, device=str(dev), model_kwargs={"torch_dtype": dtype})
    texts = [_text(b) for b in expected["d_bodies"]]

    def nodes():
        return [NodeWithScore(node=TextNode(text=t, id_=f"n{i}"), score=0.5) for i, t in enumerate(texts)]

    assert HipColbertRetriever(rr, similarity_top_k=3).retrieve("w1 w2") == []          # nothing indexed yet
    assert rr.index_nodes(nodes()) == len(texts) and sorted(rr.nodes) == sorted(f"n{i}" for i in range(len(texts)))
    retr = HipColbertRetriever(rr, similarity_top_k=len(texts))
    for body in expected["q_bodies"]:
        query = _text(body)
        ranked = _all_ranked(rr, nodes(), query)
        hits = retr.retrieve(query)
        assert all(type(h.score) is float for h in hits)
        assert [(h.node.id_, h.score) for h in hits] == ranked
        assert hits[0].node is rr.nodes[hits[0].node.id_]
        top5 = HipColbertRetriever(rr, similarity_top_k=5)._retrieve(QueryBundle(query_str=query))
        assert [(h.node.id_, h.score) for h in top5] == ranked[:5]
    # remove_node drops a passage from the hits
    query = _text(expected["q_bodies"][2])
    ranked = _all_ranked(rr, nodes(), query)
    best = ranked[0][0]
    number = int(rr.store.lookup([best])[0])
    assert rr.store.node_id(number) == best
    assert rr.remove_node(best) and not rr.remove_node(best) and best not in rr.nodes
    hits = retr.retrieve(query)
    assert [(h.node.id_, h.score) for h in hits] == ranked[1:]
    assert int(rr.store.alive[: rr.store.n_docs].sum()) == len(texts) - 1
    # re-indexing a node under the same id returns it once (the new copy; the older number is dead)
    second = ranked[1][0]
    rr.index_nodes([n for n in nodes() if n.node.id_ in (best, second)])
    assert rr.store.n_docs == len(texts) + 2 and int(rr.store.alive[: rr.store.n_docs].sum()) == len(texts)
    # similarity_top_k above the store size returns every live node
    hits = HipColbertRetriever(rr, similarity_top_k=1024).retrieve(query)
    assert [(h.node.id_, h.score) for h in hits] == ranked
    assert rr.store.node_id(number) is None and rr.store.node_id(int(rr.store.lookup([best])[0])) == best
    # search itself: two queries at once, the rows of the single-query searches
    qv = rr.encode_queries([_text(b) for b in expected["q_bodies"][:2]])
    s, i = rr.store.search(qv, 7)
    for a in range(2):
        one = rr.encode_queries([_text(expected["q_bodies"][a])])
        s1, i1 = rr.store.search(one, 7)
        assert torch.equal(s[a], s1[0]) and torch.equal(i[a], i1[0])


def test_the_wide_store_refuses_to_search(dev, built_lib):
    from tensor_truth_amd.colbert import TokenVectors
    from tensor_truth_amd.multivec import MultiVectorStore

    store = MultiVectorStore(128, torch.bfloat16, dev)
    v = torch.zeros(4, 128, dtype=torch.bfloat16, device=dev)
    store.add(["a"], v, [4])
    with pytest.raises(NotImplementedError, match="rerank-stage"):
        store.search(TokenVectors(v, np.zeros(1, np.int64), np.array([4], np.int32)), 1)
