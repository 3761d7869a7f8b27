"""GPU: the exact top-k by BGE-M3's hybrid score over the whole store (csrc/lexical.hip ``tt_hybrid_scan_topk``,
``lexical.hybrid_scan_topk``, ``LexicalStore.search_hybrid``, ``HipM3HybridRetriever``).

The oracle throughout is ``lexical.lexical_score(..., q_dense=, d_dense=, hybrid_weights=)`` with ``cand=None`` -- the rerank kernel,
which tests/test_lexical_gpu.py holds to fp64.  Nothing here has a tolerance: the scan's workspace must hold that kernel's
``out_hybrid`` byte for byte on every live pair and NaN on every dead one, and the selection must be the stable descending sort of
those scores over the live documents.

The kernel takes the queries in passes: 16 per pass while no query holds more than 64 ids, 8 per pass up to 512 ids.
``N_Q`` below holds 1, 3, 64 and one value on each side of every pass boundary of both classes.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M3 = os.path.join(GOLDEN, "m3_l2")
HW = (0.4, 0.2)
N_Q = {"short": sorted({1, 3, 64} | {b + s for b in (16, 32, 48) for s in (0, 1)}),
       "long": sorted({1, 3, 64} | {b + s for b in range(8, 64, 8) for s in (0, 1)})}
MAX_Q_NNZ = {"short": 64, "long": 512}
KS = (1, 10, 64, 65, 1024)
DUPLICATES = (1, 30, 60)                  # three documents with the same entries and the same dense row
LONG_DOCS = {5: 65, 20: 513, 41: 8192}    # document number -> nnz (none of them a tombstone)


def _pack(parts, dtype):
    nn = np.asarray([len(p) for p in parts], dtype=np.int64)
    st = np.zeros(len(parts), dtype=np.int64)
    np.cumsum(nn[:-1], out=st[1:])
    flat = np.concatenate(parts) if nn.sum() else np.zeros(0, dtype=dtype)
    return np.concatenate([flat, np.zeros(1, dtype=dtype)]).astype(dtype), st      # (one slot behind the last entry: never empty)


def _bf16_rows(rng, n, dim):
    return torch.from_numpy((rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(np.float32)).to(torch.bfloat16)


def _inputs(dim, n_docs, klass, seed):
    """64 queries of the class and ``n_docs`` documents: nnz 0 .. 11 as in test_lexical_gpu's ``_scan_inputs``, every seventh a
    tombstone that keeps its entries, one document each of nnz 65, 513 and 8192 and three exact duplicates (from 63 documents up;
    a store of one document holds the one of nnz 65), weights on a coarse grid.  Queries 0 .. 3 hold 0, 1, 33 and -- in the long
    class -- 512 ids."""
    rng = np.random.default_rng(seed)
    vocab, wide = np.arange(10, 10 + 400), np.arange(10, 10 + 20000)
    d_terms, d_nnz = [], []
    for d in range(n_docs):
        n = LONG_DOCS.get(d, int(rng.integers(0, 12))) if n_docs >= 63 else (65 if n_docs == 1 else int(rng.integers(0, 12)))
        d_terms.append(np.sort(rng.choice(wide if n > 11 else vocab, n, replace=False)).astype(np.int32))
        d_nnz.append(-1 if (d % 7 == 3 and n_docs > 1) else n)
    d_dense = _bf16_rows(rng, n_docs, dim)
    if n_docs >= 63:
        d_terms[DUPLICATES[0]] = np.sort(rng.choice(vocab, 9, replace=False)).astype(np.int32)
        d_nnz[DUPLICATES[0]] = 9
        for d in DUPLICATES[1:]:
            d_terms[d], d_nnz[d] = d_terms[DUPLICATES[0]], 9
            d_dense[d] = d_dense[DUPLICATES[0]]
    dt_, ds = _pack(d_terms, np.int32)
    dw = rng.integers(1, 3, len(dt_)).astype(np.float32) * 0.5
    if n_docs >= 63:
        a = ds[DUPLICATES[0]]
        for d in DUPLICATES[1:]:
            dw[ds[d]:ds[d] + 9] = dw[a:a + 9]
    head = [0, 1, 33] + ([512] if klass == "long" else [64])
    q_n = head + [int(rng.integers(1, 5)) for _ in range(64 - len(head))]
    q_terms = [np.sort(rng.choice(vocab if n <= 64 else wide[:1000], n, replace=False)).astype(np.int32) for n in q_n]
    qt, qs = _pack(q_terms, np.int32)
    qw = rng.integers(1, 4, len(qt)).astype(np.float32) * 0.5
    q_dense = _bf16_rows(rng, 64, dim)
    return dict(qt=qt, qw=qw, qs=qs.astype(np.int32), qn=np.asarray(q_n, dtype=np.int32), dt=dt_, dw=dw, ds=ds,
                dn=np.asarray(d_nnz, dtype=np.int32), dl=[len(p) for p in d_terms], qd=q_dense, dd=d_dense)


def _on(dev, x):
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return dict(x, qt=t(x["qt"]), qw=t(x["qw"]), dt=t(x["dt"]), dw=t(x["dw"]), qd=x["qd"].to(dev), dd=x["dd"].to(dev))


def _oracle(x, n_q=64):
    from tensor_truth_amd import lexical

    return lexical.lexical_score(x["qt"], x["qw"], x["qs"][:n_q], x["qn"][:n_q], x["dt"], x["dw"], x["ds"], x["dn"],
                                 q_dense=x["qd"][:n_q].contiguous(), d_dense=x["dd"], hybrid_weights=HW)[2].cpu().numpy()


def _scan(x, n_q, k, max_q_nnz=None, q_sel=None):
    """-> (scores, idx, the workspace's [n_q][n_docs] scores), as numpy arrays.  ``q_sel``: the queries to send, in that order."""
    from tensor_truth_amd import lexical

    sel = np.arange(n_q) if q_sel is None else np.asarray(q_sel)
    n_docs = len(x["dn"])
    stride = (n_docs + 31) // 32 * 32
    ws = torch.full((len(sel) * stride + 64,), 12345.0, dtype=torch.float32, device=x["qt"].device)      # (a sentinel no score equals)
    s, i = lexical.hybrid_scan_topk(x["qt"], x["qw"], x["qs"][sel], x["qn"][sel], x["dt"], x["dw"], x["ds"], x["dn"],
                                    x["qd"][torch.from_numpy(sel).to(x["qd"].device)].contiguous(), x["dd"], HW, k,
                                    workspace=ws.view(torch.uint8), max_q_nnz=max_q_nnz)
    return s.cpu().numpy(), i.cpu().numpy(), ws[:len(sel) * stride].view(len(sel), stride)[:, :n_docs].cpu().numpy()


def _sorted_topk(full, live, k):
    docs = np.flatnonzero(live)
    order = docs[np.argsort(-full[docs], kind="stable")][:k]                 # (score descending, document number ascending)
    want_i = np.full(k, -1, dtype=np.int32)
    want_s = np.full(k, -np.inf, dtype=np.float32)
    want_i[:len(order)] = order
    want_s[:len(order)] = full[order]
    return want_s, want_i


# ---- 1. bits and selection ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("klass", ["short", "long"])
@pytest.mark.parametrize("n_docs", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("dim", [128, 384, 1024])
def test_hybrid_scan_is_the_rerank_kernels_score_sorted(dev, built_lib, dim, n_docs, klass):
    x = _on(dev, _inputs(dim, n_docs, klass, 97 * dim + 31 * n_docs + len(klass)))
    full = _oracle(x)
    live = x["dn"] >= 0
    assert np.isneginf(full[:, ~live]).all() and np.isfinite(full[:, live]).all()
    if n_docs >= 63:
        assert {65, 513, 8192} <= set(x["dn"].tolist()) and (~live).sum() >= 9
        dup = full[:, list(DUPLICATES)]
        assert (dup == dup[:, :1]).all(), "the duplicates score equal"
    for n_q in N_Q[klass]:
        _, _, ws = _scan(x, n_q, 10, MAX_Q_NNZ[klass])
        assert ws[:, live].tobytes() == full[:n_q][:, live].tobytes(), f"n_q {n_q}: the workspace is not out_hybrid, byte for byte"
        assert np.isnan(ws[:, ~live]).all(), f"n_q {n_q}: a dead pair's slot is not NaN"
        for k in KS:
            scores, idx, _ = _scan(x, n_q, k, MAX_Q_NNZ[klass])
            want = [_sorted_topk(full[a], live, k) for a in range(n_q)]
            assert idx.tolist() == [w[1].tolist() for w in want], f"n_q {n_q} k {k}: indices"
            assert scores.tobytes() == np.stack([w[0] for w in want]).tobytes(), f"n_q {n_q} k {k}: scores"
            assert not np.isin(idx, np.flatnonzero(~live)).any(), "a tombstone was returned"
            for a in range(n_q if n_docs >= 63 else 0):
                row = idx[a].tolist()
                if all(d in row for d in DUPLICATES):
                    pos = [row.index(d) for d in DUPLICATES]
                    assert pos == list(range(pos[0], pos[0] + 3)), "equal scores come in ascending document number"
    print(f"\nhybrid scan dim {dim} n_docs {n_docs} {klass}: n_q {N_Q[klass]}, {int((~live).sum())} tombstones")


# ---- 2. independence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("klass", ["short", "long"])
@pytest.mark.parametrize("dim", [128, 1024])
def test_a_pair_scores_the_same_bits_in_every_arrangement(dev, built_lib, dim, klass):
    host = _inputs(dim, 131, klass, 7 + dim)
    x = _on(dev, host)
    full = _oracle(x)
    live = x["dn"] >= 0
    _, _, base = _scan(x, 64, 10, MAX_Q_NNZ[klass])
    assert base[:, live].tobytes() == full[:, live].tobytes()
    for q in (0, 1, 2, 3, 17, 63):
        others = [a for a in range(64) if a != q]
        for what, sel in (("alone", [q]), ("first of 64", [q] + others), ("last of 64", others + [q])):
            _, _, ws = _scan(x, len(sel), 10, MAX_Q_NNZ[klass], q_sel=sel)
            row = ws[sel.index(q)]
            assert row[live].tobytes() == base[q][live].tobytes(), f"query {q} {what}: other bits"
    # the store in reverse (document 0 <-> n_docs - 1), its entries behind filler rows of the arrays
    n = len(host["dn"])
    filler = 777
    parts_t = [host["dt"][host["ds"][d]:host["ds"][d] + host["dl"][d]] for d in range(n)]      # (a tombstone's too)
    parts_w = [host["dw"][host["ds"][d]:host["ds"][d] + host["dl"][d]] for d in range(n)]
    rt, rs = _pack([np.full(filler, 5, dtype=np.int32)] + parts_t[::-1], np.int32)
    rw, _ = _pack([np.full(filler, 9.0, dtype=np.float32)] + parts_w[::-1], np.float32)
    rev = _on(dev, dict(host, dt=rt, dw=rw, ds=rs[1:], dn=host["dn"][::-1].copy(), dd=host["dd"].flip(0).contiguous()))
    _, _, ws = _scan(rev, 64, 10, MAX_Q_NNZ[klass])
    assert ws[:, ::-1][:, live].tobytes() == base[:, live].tobytes(), "a document scores other bits at another number"


# ---- 3. refusals come before a launch ---------------------------------------------------------------------------------------------
def test_hybrid_scan_refusals_come_before_a_launch(dev, built_lib):
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    i = torch.zeros(8, dtype=torch.int32, device=dev)
    l = torch.zeros(8, dtype=torch.int64, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    b = torch.zeros(8, 128, dtype=torch.bfloat16, device=dev)
    out_s = torch.zeros(2048, dtype=torch.float32, device=dev)
    out_i = torch.zeros(2048, dtype=torch.int32, device=dev)

    def call(dim=128, n_q=1, k=2, max_q=4, wd=0.4, wl=0.2, qd=b.data_ptr(), ws_bytes=4096 * 4, n_docs=4):
        return lib.tt_hybrid_scan_topk(i.data_ptr(), f.data_ptr(), i.data_ptr(), i.data_ptr(), n_q, max_q, i.data_ptr(), f.data_ptr(),
                                       l.data_ptr(), i.data_ptr(), n_docs, qd, b.data_ptr(), dim, wd, wl, k, out_s.data_ptr(),
                                       out_i.data_ptr(), f.data_ptr(), ws_bytes, None)

    assert call(dim=192) == -2 and b"dim=192" in lib.tt_last_error()
    assert call(dim=2048) == -2 and b"dim=2048" in lib.tt_last_error()
    assert call(n_q=65) == -2
    assert call(k=1025) == -2
    assert call(max_q=513) == -2
    assert call(wd=0.0, wl=0.0) == -1 and call(wd=-1.0, wl=2.0) == -1
    assert call(qd=None) == -1
    assert call(ws_bytes=8) == -3
    torch.cuda.synchronize()
    assert (out_s == 0).all() and (out_i == 0).all(), "a refused call wrote its outputs"
    assert call(n_q=3, k=5, n_docs=0) == 0
    torch.cuda.synchronize()
    assert np.isneginf(out_s[:15].cpu().numpy()).all() and (out_i[:15] == -1).all(), "n_docs == 0 pads the outputs"
    assert (out_s[15:] == 0).all() and (out_i[15:] == 0).all() and (f == 0).all(), "n_docs == 0 writes the padding only"
    assert call() == 0                    # (the same arguments are accepted once nothing is wrong with them)
    torch.cuda.synchronize()


# ---- 4. the fixture --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(GOLDEN, "m3_l2_expected.npz"))


@pytest.fixture(scope="module")
def embedders(dev, built_lib):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = HipHuggingFaceEmbedding(model_name=M3, device="cuda:0", model_kwargs={"precision": precision})
        return cache[precision]

    return get


def _nodes(passages):
    from tensor_truth_amd.schema import NodeWithScore, TextNode

    return [NodeWithScore(node=TextNode(text=t, id_=f"p{i}"), score=0.0) for i, t in enumerate(passages)]


def _hits(retriever, q):
    return [(n.node.id_, n.score) for n in retriever.retrieve(q)]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fixture_hybrid_retriever(dev, built_lib, expected, embedders, precision):
    from tensor_truth_amd import lexical, splade

    z = expected
    n_q = int(z["n_queries"])
    texts = [str(t) for t in z["texts"]]
    queries, passages = texts[:n_q], texts[n_q:]
    assert len(queries) == 4 and len(passages) == 24
    emb = embedders(precision)
    hw = tuple(float(v) for v in z["hybrid_weights"])
    make = lambda weights, **kw: lexical.HipM3HybridRerank(model=M3, top_n=24, model_kwargs=dict(hybrid_weights=weights, embedder=emb, **kw))  # noqa: E731
    stored, sealed, lex_rr = make(hw), make(hw, postings=True), make((0, 1))
    for rr in (stored, sealed, lex_rr):
        assert rr.index_nodes(_nodes(passages)) == 24
    retr = lexical.HipM3HybridRetriever(stored, similarity_top_k=10)
    plain = {}
    for qi, q in enumerate(queries):
        want = [(n.node.id_, n.score) for n in stored.postprocess_nodes(_nodes(passages), query_str=q)]
        assert len(want) == 24 and all(isinstance(s, float) for _, s in want)
        plain[q] = _hits(retr, q)
        assert plain[q] == want[:10], f"query {qi}: not the rerank path's ids and scores"
        assert [i for i, _ in plain[q][:5]] == [f"p{i}" for i in np.argsort(-z["hybrid"][qi])[:5]], "the fp64 top-5 order"
    # (0, 1): the lexical retriever's result, zero scores dropped
    lex_h, lex_l = lexical.HipM3HybridRetriever(lex_rr, similarity_top_k=10), lexical.HipLexicalRetriever(lex_rr, similarity_top_k=10)
    for q in queries:
        got = _hits(lex_h, q)
        assert got == _hits(lex_l, q) and 0 < len(got) < 10
    # posting lists change nothing: the hybrid search is the full scan
    sealed.store.seal()
    assert sealed.store.index is not None
    retr_s = lexical.HipM3HybridRetriever(sealed, similarity_top_k=10)
    for q in queries:
        assert _hits(retr_s, q) == plain[q], "sealed posting lists changed the hybrid hits"
    best = plain[queries[0]][0][0]
    assert stored.remove_node(best)
    again = _hits(retr, queries[0])
    assert len(again) == 10 and best not in [i for i, _ in again], "a removed node was returned"
    assert again[:9] == plain[queries[0]][1:], "the other hits keep their scores and order"
    with pytest.raises(ValueError, match="no dense rows"):
        splade.SpladeStore(dev).search_hybrid(None, None, 10, hw)
