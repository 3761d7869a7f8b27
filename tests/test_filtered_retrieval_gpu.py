"""GPU: metadata-filtered retrieval through the public surface -- ``index.as_retriever(filters=...)``, ``HipIndexGroup`` /
``MultiIndexRetriever`` with one shared filter, concurrent callers with different filters, mutation, refusal on sharded indexes."""
import threading

import numpy as np
import pytest
import torch

import tensor_truth_amd  # noqa: F401
from tensor_truth_amd.metadata_filter import build_metadata_filters, row_matches
from tensor_truth_amd.retrievers import MultiIndexRetriever
from tensor_truth_amd.schema import QueryBundle, TextNode
from tensor_truth_amd.sharded_index import ShardedHipVectorIndex
from tensor_truth_amd.vector_index import HipIndexGroup, HipVectorIndex

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
D = 256
DOC_TYPES = ["library", "book", "paper", "blog"]


def _unit(x):
    x = torch.as_tensor(x, dtype=torch.float32)
    return x / x.norm(dim=-1, keepdim=True)


def _nodes(n, seed, prefix):
    rng = np.random.default_rng(seed)
    nodes = []
    for i in range(n):
        md = {"doc_type": DOC_TYPES[rng.integers(0, 4)], "version": float(rng.integers(0, 40)) / 10, "page": int(rng.integers(0, 300))}
        if rng.random() < 0.1:
            del md["doc_type"]                      # a missing key matches nothing
        if rng.random() < 0.3:
            md["tags"] = [str(t) for t in rng.choice(["cuda", "hip", "rocm", "torch"], size=2, replace=False)]
        nodes.append(TextNode(text=f"{prefix} {i}", id_=f"{prefix}-{i}", metadata=md))
    emb = _unit(torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)))
    return nodes, emb


def _matches(filters, md) -> bool:
    res = []
    for f in filters.filters:
        op = getattr(f.operator, "value", f.operator)
        res.append(row_matches(op, f.key in md, md.get(f.key), f.value))
    cond = getattr(filters.condition, "value", filters.condition)
    return any(res) if cond == "or" else all(res)


def _host_ranking(index, q, filters, k):
    """Brute force on the host: fp64 dot products of the bf16 rows of the matching leaves."""
    mat, ids = index.snapshot()
    m = mat.float().cpu().double()
    qq = _unit(q).to(torch.bfloat16).double()
    scores = (m @ qq).numpy()
    cand = [(-scores[r], r) for r, nid in enumerate(ids)
            if nid is not None and nid in index.docstore and _matches(filters, index.docstore[nid].metadata)]
    cand.sort()
    return [ids[r] for _, r in cand[:k]], [-s for s, _ in cand[:k]]


def _matching_only(index, filters):
    """A fresh index over the matching live leaves only, same rows in the same order."""
    mat, ids = index.snapshot()
    keep = [r for r, nid in enumerate(ids) if nid is not None and _matches(filters, index.docstore[nid].metadata)]
    sub = HipVectorIndex(D, DEV, score_mode="cosine")
    if keep:
        sub.add([index.docstore[ids[r]] for r in keep], embeddings=mat[torch.tensor(keep, device=DEV)].float())
    return sub


def _hits(nodes):
    return [(n.node.id_, n.score) for n in nodes]


SPECS = [
    {"doc_type": "library"},
    {"doc_type": ["book", "paper"], "version": {"$gte": 2.0}},
    {"tags": {"$contains": "hip"}},
    {"doc_type": {"$ne": "blog"}, "page": {"$lt": 40}},
    {"doc_type": {"$text_match": "oo"}},
]


def test_as_retriever_filters_return_only_matching_exact_hits():
    nodes, emb = _nodes(3000, 1, "a")
    index = HipVectorIndex(D, DEV, score_mode="cosine")
    index.add(nodes, embeddings=emb)
    rng = np.random.default_rng(2)
    for spec in SPECS:
        filters = build_metadata_filters(spec)
        ret = index.as_retriever(similarity_top_k=5, filters=filters)
        for _ in range(3):
            q = rng.standard_normal(D).astype(np.float32)
            got = ret.retrieve(QueryBundle(query_str="q", embedding=q.tolist()))
            assert got and all(_matches(filters, n.node.metadata) for n in got), spec
            want_ids, want_s = _host_ranking(index, torch.from_numpy(q), filters, 5)
            assert [n.node.id_ for n in got] == want_ids, spec
            assert np.allclose([n.score for n in got], want_s, rtol=1e-3, atol=1e-4)


def test_mutation_keeps_filtered_search_exact():
    nodes, emb = _nodes(4000, 3, "m")
    index = HipVectorIndex(D, DEV, score_mode="cosine")
    index.add(nodes[:2000], embeddings=emb[:2000])
    filters = build_metadata_filters({"doc_type": ["library", "paper"], "version": {"$lt": 3.0}})
    ret = index.as_retriever(similarity_top_k=8, filters=filters, coalesce=False)
    q = np.random.default_rng(4).standard_normal((4, D)).astype(np.float32)

    def check():
        sub = _matching_only(index, filters)
        ref = sub.as_retriever(similarity_top_k=8, coalesce=False)
        for qq in q:
            b = QueryBundle(query_str="q", embedding=qq.tolist())
            assert _hits(ret.retrieve(b)) == _hits(ref.retrieve(b))

    check()                                                     # columns built on first use
    index.add(nodes[2000:3000], embeddings=emb[2000:3000])      # appended codes (and a grown matrix)
    check()
    index.delete([n.id_ for n in nodes[0:1500:2]])              # tombstones
    check()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        index.persist(tmp)                                      # compaction: renumbered rows, columns replaced
        check()
        loaded = HipVectorIndex.load(tmp, DEV, score_mode="cosine")
        lret = loaded.as_retriever(similarity_top_k=8, filters=filters, coalesce=False)
        for qq in q:
            b = QueryBundle(query_str="q", embedding=qq.tolist())
            assert _hits(lret.retrieve(b)) == _hits(ret.retrieve(b))
    index.add(nodes[3000:], embeddings=emb[3000:])
    check()
    # an old snapshot keeps its own rows across a compaction
    snap = index.snapshot()
    index.delete([n.id_ for n in nodes[3000:3600]])
    index._compact()
    s_old, r_old = index.search(torch.from_numpy(q), 8, snapshot=snap, filters=filters)
    by_id = {n.id_: n for n in nodes}
    _, ids = snap
    for row in r_old.flatten().cpu().tolist():
        if row >= 0:
            assert ids[row] is not None and _matches(filters, by_id[ids[row]].metadata)


def test_group_and_multi_index_share_one_filter():
    idxs, rets = [], []
    for m in range(3):
        nodes, emb = _nodes(1500 + 500 * m, 10 + m, f"g{m}")
        ix = HipVectorIndex(D, DEV, score_mode="cosine")
        ix.add(nodes, embeddings=emb)
        idxs.append(ix)
    filters = build_metadata_filters({"doc_type": "book", "page": {"$gte": 100}})
    q = np.random.default_rng(5).standard_normal((3, D)).astype(np.float32)
    group = HipIndexGroup(idxs)
    s, r = group.search(torch.from_numpy(q), 6, filters=filters)
    hs, hr, ids = group.search_host(torch.from_numpy(q), 6, filters=filters)
    assert torch.equal(hr, r.cpu()) and torch.equal(hs.view(torch.int32), s.cpu().view(torch.int32))
    for m, ix in enumerate(idxs):
        ws, wr = ix.search(torch.from_numpy(q), 6, filters=filters)
        assert torch.equal(r[:, m], wr) and torch.equal(s[:, m].view(torch.int32), ws.view(torch.int32)), m
    # MultiIndexRetriever: single pass through the group, equal to the per-retriever path
    rets = [ix.as_retriever(similarity_top_k=6, filters=filters) for ix in idxs]
    mir = MultiIndexRetriever(rets, enable_cache=False, share_query_embedding=False)
    b = QueryBundle(query_str="q", embedding=q[0].tolist())
    single = mir._single_pass_retrieve(b)
    assert single is not None
    for m, ret in enumerate(rets):
        assert _hits(single[m]) == _hits(ret.retrieve(b))
        assert all(_matches(filters, n.node.metadata) for n in single[m])
    # different filters per retriever: no single pass (per-retriever calls)
    other = [idxs[0].as_retriever(similarity_top_k=6, filters=build_metadata_filters({"doc_type": "blog"}))] + rets[1:]
    assert MultiIndexRetriever(other, enable_cache=False)._single_pass_retrieve(b) is None


def test_concurrent_callers_with_different_filters():
    nodes, emb = _nodes(6000, 20, "c")
    index = HipVectorIndex(D, DEV, score_mode="cosine")
    index.add(nodes, embeddings=emb)
    fa = build_metadata_filters({"doc_type": "library"})
    fb = build_metadata_filters({"tags": {"$contains": "rocm"}, "version": {"$gt": 1.0}})
    ra = index.as_retriever(similarity_top_k=7, filters=fa)
    rb = index.as_retriever(similarity_top_k=7, filters=fb)
    qs = np.random.default_rng(21).standard_normal((8, D)).astype(np.float32)
    want = []
    for i, qq in enumerate(qs):
        f = fa if i % 2 == 0 else fb
        want.append(_host_ranking(index, torch.from_numpy(qq), f, 7)[0])
    got = [None] * 8
    barrier = threading.Barrier(8)

    def run(i):
        barrier.wait()
        r = ra if i % 2 == 0 else rb
        got[i] = [n.node.id_ for n in r.retrieve(QueryBundle(query_str=f"q{i}", embedding=qs[i].tolist()))]

    threads = [threading.Thread(target=run, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got == want


def test_sharded_index_refuses_filters():
    nodes, emb = _nodes(200, 30, "s")
    rows = emb.to(torch.bfloat16).to(DEV).contiguous()
    index = ShardedHipVectorIndex(D, rows, 0, 200, [n.id_ for n in nodes], {n.id_: n for n in nodes}, score_mode="cosine")
    filters = build_metadata_filters({"doc_type": "library"})
    with pytest.raises(NotImplementedError):
        index.as_retriever(similarity_top_k=5, filters=filters)
    with pytest.raises(NotImplementedError):
        index.search(emb[:1], 5, filters=filters)
