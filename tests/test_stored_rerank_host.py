"""CPU: the rerank driver the stored-passage postprocessors share (tensor_truth_amd/_stored.py), through a stub subclass whose
encoders return the texts and whose scorers compute a value from (query text, passage text).  No device, no library.

Checked here: ``predict`` returns each pair's own value in input order over rows of uneven width and a repeated pair;
``postprocess_nodes`` splits its nodes into the stored and the encoded part, hands each scorer a table that holds -1 exactly where
a passage belongs to the other part, counts them in ``stats``, sorts, cuts and keeps the retrieval score only when asked; a
passage one of two stores does not hold is encoded; the ranking both ``rerank`` surfaces use is stable.
"""
import zlib

import numpy as np
import pytest

from tensor_truth_amd._stored import IdTable, _StoredRerank, descending, rerank_result
from tensor_truth_amd.schema import NodeWithScore, QueryBundle, TextNode


def value(query: str, passage: str) -> float:
    return float(zlib.crc32(f"{query}|{passage}".encode()) % 9973)


class Stub(_StoredRerank):
    """``held``: one {node id: document number} per store; a stored document's text is ``texts[document number]``."""

    def __init__(self, held=({},), texts=(), top_n=10, keep_retrieval_score=False):
        self.held, self.texts, self.top_n, self.keep_retrieval_score = [dict(h) for h in held], list(texts), top_n, keep_retrieval_score
        self.stats = {"queries": 0, "stored": 0, "encoded": 0}
        self.calls = []                      # ("stored", cands) / ("fresh", cand, texts), in call order

    def encode_queries(self, texts):
        self.calls.append(("queries", list(texts)))
        return list(texts)

    def encode_documents(self, texts):
        return list(texts)

    def add_documents(self, nodes, encoded):
        for n, t in zip(nodes, encoded):
            for h in self.held:
                h[n.id_] = len(self.texts)
            self.texts.append(t)

    def lookup(self, ids):
        rows = [np.asarray([h.get(i, -1) for i in ids], dtype=np.int32) for h in self.held]
        return rows[0] if len(rows) == 1 else np.stack(rows)

    def _table(self, q, cand, texts):
        out = np.full(cand.shape, np.nan, dtype=np.float32)          # (a slot of no passage must never be read)
        for (a, j), d in np.ndenumerate(cand):
            if d >= 0:
                out[a, j] = value(q[a], texts[d])
        return out

    def score_stored(self, q, cands):
        self.calls.append(("stored", [c.copy() for c in cands]))
        assert all(c.dtype == np.int32 and c.shape == cands[0].shape for c in cands)
        assert all(((c >= 0) == (cands[0] >= 0)).all() for c in cands), "every store's table names the same passages"
        return self._table(q, cands[0], self.texts)

    def score_fresh(self, q, d, cand):
        self.calls.append(("fresh", cand.copy(), list(d)))
        assert cand.dtype == np.int32
        return self._table(q, cand, d)


def nodes_of(texts, score=0.5):
    return [NodeWithScore(node=TextNode(text=t, id_=f"n{i}"), score=score + i) for i, t in enumerate(texts)]


def kinds(stub):
    return [c[0] for c in stub.calls]


def test_predict_over_uneven_widths_and_a_duplicate_pair():
    q, d = ["q0", "q1"], ["d0", "d1", "d2"]
    pairs = [(q[0], d[0]), (q[0], d[1]), (q[0], d[2]), (q[1], d[1]), (q[0], d[1])]
    rr = Stub()
    got = rr.predict(pairs)
    assert got == [value(a, b) for a, b in pairs] and all(type(s) is float for s in got)
    assert kinds(rr) == ["queries", "fresh"]
    cand, texts = rr.calls[1][1:]
    assert texts == d and cand.tolist() == [[0, 1, 2, 1], [1, -1, -1, -1]]
    assert rr.stats == {"queries": 2, "stored": 0, "encoded": 3}
    assert rr.predict([]) == [] and kinds(rr) == ["queries", "fresh"]


@pytest.mark.parametrize("keep", [False, True])
def test_postprocess_nodes_mixes_stored_and_fresh(keep):
    texts = [f"passage {i}" for i in range(5)]
    rr = Stub(held=({"n0": 2, "n2": 0, "n4": 1},), texts=[texts[2], texts[4], texts[0]], top_n=3, keep_retrieval_score=keep)
    nodes = nodes_of(texts)
    out = rr.postprocess_nodes(nodes, QueryBundle("the query"))
    assert kinds(rr) == ["queries", "stored", "fresh"], "queries first, then the stored part, then the fresh part; each once"
    assert [c.tolist() for c in rr.calls[1][1]] == [[[2, -1, 0, -1, 1]]]
    assert rr.calls[2][1].tolist() == [[-1, 0, -1, 1, -1]] and rr.calls[2][2] == [texts[1], texts[3]]
    assert rr.stats == {"queries": 1, "stored": 3, "encoded": 2}
    want = {f"n{i}": value("the query", t) for i, t in enumerate(texts)}
    assert all(n.score == want[n.node.id_] and type(n.score) is float for n in nodes)
    assert [n.node.id_ for n in out] == sorted(want, key=lambda i: -want[i])[:3]
    for i, n in enumerate(nodes):
        assert n.node.metadata.get("retrieval_score") == (0.5 + i if keep else None)
    # positional and query_str forms, and the alias llama-index calls
    again = rr._postprocess_nodes(nodes_of(texts), None, "the query")
    assert [n.node.id_ for n in again] == [n.node.id_ for n in out]


def test_all_stored_and_all_fresh_call_one_scorer_each():
    texts = ["a", "b", "c"]
    rr = Stub(top_n=2)
    assert rr.index_nodes(nodes_of(texts)[:1] + [n.node for n in nodes_of(texts)[1:]]) == 3      # (wrapped or bare)
    assert rr.index_nodes([]) == 0 and rr.texts == texts
    out = rr.postprocess_nodes(nodes_of(texts), query_str="q")
    assert kinds(rr) == ["queries", "stored"] and rr.stats == {"queries": 1, "stored": 3, "encoded": 0}
    assert len(out) == 2 and out[0].score >= out[1].score
    fresh = Stub()
    fresh.postprocess_nodes(nodes_of(texts), query_str="q")
    assert kinds(fresh) == ["queries", "fresh"] and fresh.stats == {"queries": 1, "stored": 0, "encoded": 3}
    assert fresh.calls[1][1].tolist() == [[0, 1, 2]]


def test_a_passage_one_of_two_stores_lacks_is_fresh():
    texts = ["a", "b", "c"]
    rr = Stub(held=({"n0": 0, "n1": 1, "n2": 2}, {"n0": 5, "n2": 7}), texts=texts)
    nodes = nodes_of(texts)
    rr.postprocess_nodes(nodes, query_str="q")
    assert kinds(rr) == ["queries", "stored", "fresh"]
    assert [c.tolist() for c in rr.calls[1][1]] == [[[0, -1, 2]], [[5, -1, 7]]]
    assert rr.calls[2][1].tolist() == [[-1, 0, -1]] and rr.calls[2][2] == ["b"]
    assert rr.stats == {"queries": 1, "stored": 2, "encoded": 1}
    assert [n.score for n in nodes] == [value("q", t) for t in texts]


def test_missing_query_and_empty_inputs():
    rr = Stub()
    with pytest.raises(ValueError, match=r"^Missing query bundle in extra info\.$"):
        rr.postprocess_nodes(nodes_of(["a"]))
    assert rr.postprocess_nodes([], query_str="q") == [] and rr.predict([]) == [] and rr.rerank("q", []) == []
    assert rr.calls == [] and rr.stats == {"queries": 0, "stored": 0, "encoded": 0}


def test_the_ranking_is_stable_and_shared():
    scores = [1.0, 3.0, 3.0, 0.5, 3.0]
    assert descending(scores) == [1, 2, 4, 0, 3] and descending(scores, 2) == [1, 2] and descending([], 3) == []
    assert rerank_result(scores, 3) == [{"index": i, "relevance_score": 3.0} for i in (1, 2, 4)]
    assert [r["index"] for r in rerank_result(scores)] == [1, 2, 4, 0, 3]
    # the driver's rerank and the cross-encoder's rerank are this helper over their own predict
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank

    docs = ["a", "b", "c", "d", "e"]
    table = dict(zip(docs, scores))
    ce = object.__new__(HipSentenceTransformerRerank)
    ce.predict = lambda pairs: [table[d] for _, d in pairs]
    rr = Stub()
    rr.predict = ce.predict
    assert ce.rerank("q", docs, top_n=4) == rr.rerank("q", docs, top_n=4) == rerank_result(scores, 4)
    # equal node scores keep input order too
    tied = Stub(top_n=3)
    tied.score_fresh = lambda q, d, cand: np.ones(cand.shape, dtype=np.float32)
    assert [n.node.id_ for n in tied.postprocess_nodes(nodes_of(docs), query_str="q")] == ["n0", "n1", "n2"]


def test_id_table():
    t = IdTable()
    assert t.assign(["a", "b"]) == [] and t.assign(["b", "c"]) == [1]
    assert len(t) == 3 and t.lookup(["a", "b", "c", "x"]).tolist() == [0, 2, 3, -1] and t.lookup([]).dtype == np.int32
    assert [t.node_id(d) for d in (-1, 0, 1, 2, 3, 4)] == [None, "a", None, "b", "c", None]
    assert t.pop("a") == 0 and t.pop("a") is None and t.node_id(0) is None and len(t) == 2
