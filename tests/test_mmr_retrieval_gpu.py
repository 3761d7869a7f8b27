"""GPU: MMR through the public surface -- ``index.as_retriever(vector_store_query_mode="mmr", ...)``, ``search_mmr``, the
coalescer, filters, ``MultiIndexRetriever``, snapshots, and the refusal on a row-sharded index.  Precomputed embeddings, no model."""
import threading

import numpy as np
import pytest
import torch

import tensor_truth_amd  # noqa: F401
from tensor_truth_amd.metadata_filter import build_metadata_filters
from tensor_truth_amd.retrievers import MultiIndexRetriever
from tensor_truth_amd.schema import QueryBundle, TextNode
from tensor_truth_amd.sharded_index import ShardedHipVectorIndex
from tensor_truth_amd.vector_index import HipVectorIndex

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
D = 128
SIZES = [6, 3, 3, 3, 3]          # near-duplicate clusters around e0 .. e4: 18 rows, all within the 20 candidates of k = 5 x 4
AFFINITY = [1.0, 0.9, 0.8, 0.7, 0.6]


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _planted(seed, prefix, n_filler=300):
    """Clusters of near-identical rows (centre e_c plus a little noise in dims 5 .. 63) among filler that lives in dims 64 ..: the
    cosine is ~0.99 inside a cluster and ~0 across.  Every second member of a cluster and every third filler row is tagged
    kind=odd for the filter test."""
    g = torch.Generator().manual_seed(seed)
    rows, names, kinds = [], [], []
    for c, size in enumerate(SIZES):
        for j in range(size):
            v = torch.zeros(D)
            v[c] = 1.0
            v[5:64] = 0.012 * torch.randn(59, generator=g)
            rows.append(v)
            names.append(f"{prefix}-c{c}-{j}")
            kinds.append("odd" if j % 2 == 0 else "even")
    filler = torch.zeros(n_filler, D)
    filler[:, 64:] = torch.randn(n_filler, D - 64, generator=g)
    emb = _unit(torch.cat([torch.stack(rows), filler]))
    names += [f"{prefix}-f{i}" for i in range(n_filler)]
    kinds += ["odd" if i % 3 == 0 else "even" for i in range(n_filler)]
    order = torch.randperm(len(names), generator=g).tolist()           # clusters scattered over the rows
    nodes = [TextNode(text=names[i], id_=names[i], metadata={"kind": kinds[i]}) for i in order]
    return nodes, emb[order]


def _query(weights=AFFINITY):
    q = np.zeros(D, dtype=np.float32)
    q[: len(weights)] = weights
    return QueryBundle(query_str="q", embedding=q.tolist())


def _cluster(node_id):
    return node_id.split("-")[1]


def _hits(nodes):
    return [(n.node.id_, n.score) for n in nodes]


def _index(seed=1, prefix="a", **kw):
    nodes, emb = _planted(seed, prefix)
    index = HipVectorIndex(D, DEV, **kw)
    index.add(nodes, embeddings=emb)
    return index


MMR = dict(vector_store_query_mode="mmr", vector_store_kwargs={"mmr_threshold": 0.5})


def test_mmr_mode_returns_one_node_per_cluster():
    index = _index()
    plain = index.as_retriever(similarity_top_k=5).retrieve(_query())
    assert [_cluster(n.node.id_) for n in plain] == ["c0"] * 5
    got = index.as_retriever(similarity_top_k=5, **MMR).retrieve(_query())
    assert [_cluster(n.node.id_) for n in got] == ["c0", "c1", "c2", "c3", "c4"]          # selection order: by affinity
    assert got[0].node.id_ == plain[0].node.id_ and got[0].score == plain[0].score
    # the score is the node's relevance on the usual scale, node_score(cosine), not the MMR value
    mat, ids = index.snapshot()
    qq = _unit(torch.tensor(_query().embedding)).to(torch.bfloat16).double()
    for n in got:
        cos = float(mat[ids.index(n.node.id_)].double().cpu() @ qq)
        assert n.score == pytest.approx(index.node_score(cos), rel=1e-4)
    # "last" forgets all but the latest pick: after c0, c1 it goes back to a c0 duplicate
    last = index.as_retriever(similarity_top_k=3, vector_store_query_mode="mmr",
                              vector_store_kwargs={"mmr_threshold": 0.5, "mmr_penalty": "last"}).retrieve(_query())
    assert [_cluster(n.node.id_) for n in last] == ["c0", "c1", "c0"]


def test_threshold_one_is_the_default_mode():
    index = _index()
    for k in (1, 5, 12):
        plain = index.as_retriever(similarity_top_k=k, coalesce=False).retrieve(_query())
        one = index.as_retriever(similarity_top_k=k, coalesce=False, vector_store_query_mode="mmr",
                                 vector_store_kwargs={"mmr_threshold": 1}).retrieve(_query())
        assert _hits(one) == _hits(plain) and len(plain) == k
    for mode in (None, "default"):
        assert _hits(index.as_retriever(similarity_top_k=5, vector_store_query_mode=mode).retrieve(_query())) == \
            _hits(index.as_retriever(similarity_top_k=5).retrieve(_query()))


def test_results_do_not_depend_on_the_batch():
    index = _index()
    rng = np.random.default_rng(3)
    queries = [_query((rng.permutation(AFFINITY) + rng.uniform(0, 0.05, 5)).tolist()) for _ in range(32)]
    lone = index.as_retriever(similarity_top_k=5, coalesce=False, **MMR)
    want = [_hits(lone.retrieve(q)) for q in queries]
    assert all(len({_cluster(i) for i, _ in w}) == 5 for w in want)
    front = index.as_retriever(similarity_top_k=5, **MMR)
    assert _hits(front.retrieve(queries[0])) == want[0]                                   # a lone call through the coalescer
    got = [None] * len(queries)

    def work(i):
        got[i] = _hits(front.retrieve(queries[i]))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(queries))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert got == want
    # and the batched search itself: rows, cosines and MMR values, bit for bit
    qm = torch.tensor([q.embedding for q in queries])
    s_all, r_all, v_all = index.search_mmr_host(qm, 5)
    for i in range(0, 32, 7):
        s1, r1, v1 = index.search_mmr_host(qm[i:i + 1], 5)
        assert torch.equal(r1[0], r_all[i]) and torch.equal(s1[0].view(torch.int32), s_all[i].view(torch.int32))
        assert torch.equal(v1[0].view(torch.int32), v_all[i].view(torch.int32))
    d_s, d_r, d_v = index.search_mmr(qm, 5)
    assert torch.equal(d_r.cpu(), r_all) and torch.equal(d_s.cpu(), s_all) and torch.equal(d_v.cpu(), v_all)


def test_filters_apply_to_the_candidates():
    nodes, emb = _planted(1, "a")
    index = HipVectorIndex(D, DEV)
    index.add(nodes, embeddings=emb)
    filters = build_metadata_filters({"kind": "odd"})
    got = index.as_retriever(similarity_top_k=5, filters=filters, **MMR).retrieve(_query())
    assert got and all(n.node.metadata["kind"] == "odd" for n in got)
    plain = index.as_retriever(similarity_top_k=5, filters=filters).retrieve(_query())
    assert got[0].node.id_ == plain[0].node.id_
    assert [_cluster(n.node.id_) for n in plain] == ["c0", "c0", "c0", "c1", "c1"]
    assert [_cluster(n.node.id_) for n in got] == ["c0", "c1", "c2", "c3", "c4"]
    # against the unfiltered search over an index of the passing rows only: same picks, same scores
    keep = [r for r, n in enumerate(nodes) if n.metadata["kind"] == "odd"]
    sub = HipVectorIndex(D, DEV)
    sub.add([nodes[r] for r in keep], embeddings=emb[keep])
    assert _hits(sub.as_retriever(similarity_top_k=5, **MMR).retrieve(_query())) == _hits(got)


def test_multi_index_retriever_keeps_each_index_its_mmr_picks(monkeypatch):
    a, b = _index(1, "a"), _index(2, "b")
    ra, rb = a.as_retriever(similarity_top_k=4, **MMR), b.as_retriever(similarity_top_k=4, **MMR)
    multi = MultiIndexRetriever([ra, rb], enable_cache=False, balance_strategy="none")
    q = _query()
    want = {0: _hits(ra.retrieve(q)), 1: _hits(rb.retrieve(q))}

    def by_index(nodes):
        out = {0: [], 1: []}
        for n in nodes:
            out[n.node.metadata["_source_index"]].append((n.node.id_, n.score))
        return out

    # hand the precomputed embedding down in the bundle, as a shared embed model would
    import tensor_truth_amd.retrievers as rt
    monkeypatch.setattr(rt, "QueryBundle", lambda query_str: QueryBundle(query_str=query_str, embedding=q.embedding))
    got = by_index(multi.retrieve("q"))
    assert got == want
    assert [_cluster(i) for i, _ in got[0]] == ["c0", "c1", "c2", "c3"] == [_cluster(i) for i, _ in got[1]]
    balanced = MultiIndexRetriever([ra, rb], enable_cache=False, balance_strategy="top_k_per_index")
    both = balanced.retrieve("q")
    assert len(both) == 8 and [n.score for n in both] == sorted((n.score for n in both), reverse=True)
    assert {k: sorted(v) for k, v in by_index(both).items()} == {k: sorted(v) for k, v in want.items()}
    # with room for three per index, balancing keeps each index's first three: the MMR prefix
    three = MultiIndexRetriever([ra, b.as_retriever(similarity_top_k=3, **MMR)], enable_cache=False,
                                balance_strategy="top_k_per_index").retrieve("q")
    assert sorted(by_index(three)[0]) == sorted(want[0][:3]) and sorted(by_index(three)[1]) == sorted(want[1][:3])


def test_search_mmr_over_a_snapshot_taken_before_a_delete():
    index = _index(score_mode="cosine")
    q = torch.tensor([_query().embedding])
    snap = index.snapshot()
    s0, r0, v0 = index.search_mmr_host(q, 5, snapshot=snap)
    ids0 = [snap[1][r] for r in r0[0].tolist()]
    assert [_cluster(i) for i in ids0] == ["c0", "c1", "c2", "c3", "c4"]
    index.delete([ids0[1]])                                              # the c1 pick becomes a tombstone (NaN row)
    s1, r1, v1 = index.search_mmr_host(q, 5, snapshot=snap)              # still answers over the old snapshot
    assert r1.shape == (1, 5) and ids0[1] not in [snap[1][r] for r in r1[0].tolist() if r >= 0]
    now = index.as_retriever(similarity_top_k=5, coalesce=False, **MMR).retrieve(_query())
    assert ids0[1] not in [n.node.id_ for n in now]
    assert [_cluster(n.node.id_) for n in now] == ["c0", "c1", "c2", "c3", "c4"]        # another c1 row takes its place
    # k beyond the rows there are: padded like search
    tiny = HipVectorIndex(D, DEV, score_mode="cosine")
    nodes, emb = _planted(5, "t", n_filler=0)
    tiny.add(nodes[:3], embeddings=emb[:3])
    s, r, v = tiny.search_mmr_host(q, 5)
    assert (r[0, :3] >= 0).all() and r[0, 3:].tolist() == [-1, -1] and torch.isinf(s[0, 3:]).all()
    with pytest.raises(ValueError):
        index.search_mmr(q, 5, lam=1.5)
    with pytest.raises(ValueError):
        index.search_mmr(q, 5, prefetch_factor=0.5)
    with pytest.raises(ValueError):
        index.search_mmr(q, 5, penalty="mean")


def test_sharded_index_refuses_mmr():
    nodes, emb = _planted(7, "s", n_filler=50)
    rows = emb.to(torch.bfloat16).to(DEV).contiguous()
    index = ShardedHipVectorIndex(D, rows, 0, len(nodes), [n.id_ for n in nodes], {n.id_: n for n in nodes}, score_mode="cosine")
    with pytest.raises(NotImplementedError):
        index.as_retriever(similarity_top_k=5, vector_store_query_mode="mmr")
