"""What the rerank postprocessors over stored passages (``HipColbertRerank``, ``HipM3HybridRerank``, ``HipM3AllRerank``) and their
stores share: the table from node ids to document numbers, the ranking of a list of scores, the retrievers' hit loop, and ``_StoredRerank`` -- the
postprocessor surface with the bookkeeping that splits a call's passages into those a store holds and those encoded in the call.
Host code only: nothing here touches a device or the library."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np


class IdTable:
    """Node id -> document number and back, for a store that numbers its documents in the order they were added."""

    def __init__(self):
        self.doc_of: Dict[Any, int] = {}
        self.id_of: List[Any] = []           # document number -> node id (None once removed or replaced)

    def __len__(self) -> int:
        return len(self.doc_of)

    def assign(self, node_ids: Sequence[Any]) -> List[int]:
        """Give ``node_ids`` the next document numbers -> the numbers of the older copies of ids that were already there."""
        older = []
        for nid in node_ids:
            old = self.doc_of.get(nid)
            if old is not None:
                self.id_of[old] = None
                older.append(old)
            self.doc_of[nid] = len(self.id_of)
            self.id_of.append(nid)
        return older

    def pop(self, node_id: Any) -> Optional[int]:
        """Forget ``node_id`` -> its document number (None: it was not there)."""
        doc = self.doc_of.pop(node_id, None)
        if doc is not None:
            self.id_of[doc] = None
        return doc

    def lookup(self, node_ids: Sequence[Any]) -> np.ndarray:
        """-> document numbers (int32), -1 for an id that is not stored."""
        return np.fromiter((self.doc_of.get(n, -1) for n in node_ids), dtype=np.int32, count=len(node_ids))

    def node_id(self, doc: int) -> Any:
        """The node id of document number ``doc`` (None: removed, or no such document)."""
        return self.id_of[doc] if 0 <= doc < len(self.id_of) else None


def descending(scores: Sequence[float], top_n: Optional[int] = None) -> List[int]:
    """The positions of ``scores`` from the best down, equal scores in input order, cut to ``top_n`` (None: all)."""
    return sorted(range(len(scores)), key=lambda i: -scores[i])[:top_n]


def rerank_result(scores: Sequence[float], top_n: Optional[int] = None) -> List[Dict[str, Any]]:
    """What a ``rerank(query, documents, top_n)`` returns for the documents' ``scores``."""
    return [{"index": i, "relevance_score": float(scores[i])} for i in descending(scores, top_n)]


def top_nodes(store, query, k: int, nodes: Dict[Any, Any], node_type, positive_only: bool = True, search=None) -> list:
    """What a lexical, SPLADE or ColBERT retriever returns for ONE encoded query: ``store.search`` (through posting lists, built
    here if the store has them on and none yet) -> ``node_type(node=nodes[id], score=...)`` of the hits, best first.  Hits whose id
    is not in ``nodes`` are dropped, and -- ``positive_only``, the sparse retrievers -- hits with score <= 0: passages that share
    no weighted id with the query.  (A MaxSim sum has no such point: ``HipColbertRetriever`` keeps every hit.)  ``search``: a
    callable ``(query, k) -> (scores, idx)`` to run instead of ``store.search`` (``HipM3HybridRetriever``: the store's hybrid
    scan, which uses no posting lists -- none are built for it)."""
    if search is None:
        if getattr(store, "postings", False) and store.index is None:
            store.seal()
        search = store.search
    scores, idx = search(query, k)
    out = []
    for s, d in zip(scores[0].cpu().tolist(), idx[0].cpu().tolist()):
        if d < 0 or (positive_only and not s > 0):
            continue
        node = nodes.get(store.node_id(d))
        if node is not None:
            out.append(node_type(node=node, score=float(s)))
    return out


class _StoredRerank:
    """The postprocessor surface of ``HipSentenceTransformerRerank`` -- ``postprocess_nodes`` (keyword or positional), ``rerank``,
    ``predict`` -- plus ``index_nodes``, over passages that are either held by the instance's store(s) or encoded in the call.  A
    subclass sets ``top_n``, ``keep_retrieval_score`` and ``stats = {"queries": 0, "stored": 0, "encoded": 0}`` and supplies

        encode_queries(texts) -> q          encode_documents(texts) -> d          add_documents(nodes, d)
        lookup(ids)                         one row of document numbers per store (-1: not held)
        score_stored(q, cands)              ``cands``: one int32 [n_q][width] table of document numbers per store (-1 = none)
        score_fresh(q, d, cand)             ``cand``: int32 [n_q][width] positions in ``d`` (-1 = none)

    with both scorers returning a host fp32 [n_q][width] array.  A passage counts as stored only if every store holds it.  Within
    a call the queries are encoded first, then the stored passages are scored, then the others are encoded and scored."""

    top_n: int
    keep_retrieval_score: bool
    stats: Dict[str, int]

    # ---- ingest -----------------------------------------------------------------------------------------------------
    def index_nodes(self, nodes) -> int:
        """Encode the nodes' EMBED-mode content into the store(s) (a ``NodeWithScore`` or a bare node) -> how many were added."""
        from .schema import MetadataMode

        bare = [getattr(n, "node", n) for n in nodes]
        if not bare:
            return 0
        self.add_documents(bare, self.encode_documents([n.get_content(metadata_mode=MetadataMode.EMBED) for n in bare]))
        return len(bare)

    # ---- scoring ----------------------------------------------------------------------------------------------------
    def _score(self, queries: List[str], docs: List[Any], table: np.ndarray, stored=None) -> np.ndarray:
        """Scores fp32 [n_q][width] of ``table``, each query's row of document numbers (positions in ``docs``, -1 = none; what is
        returned there is not to be read).  ``stored``: ``lookup``'s rows for ``docs`` (None: nothing is stored); a document every
        store holds is scored from the stores, any other is ``docs[d]`` (text), encoded here."""
        q = self.encode_queries(queries)
        n_d = len(docs)
        rows = np.full((1, n_d), -1) if stored is None else np.atleast_2d(stored)
        held = (rows >= 0).all(0)
        n_held = int(held.sum())
        there = table >= 0
        from_store = there & held[table]
        out = np.zeros(table.shape, dtype=np.float32)
        if n_held:
            cands = [np.where(from_store, row[table], -1).astype(np.int32) for row in rows]
            out[from_store] = self.score_stored(q, cands)[from_store]
        if n_held < n_d:
            from_text = there & ~from_store
            slot = np.cumsum(~held) - 1                   # a fresh document's position among the fresh
            cand = np.where(from_text, slot[table], -1).astype(np.int32)
            d = self.encode_documents([docs[i] for i in np.flatnonzero(~held)])
            out[from_text] = self.score_fresh(q, d, cand)[from_text]
        st = self.stats
        st["queries"] += len(queries)
        st["stored"] += n_held
        st["encoded"] += n_d - n_held
        return out

    def predict(self, pairs: Sequence[Sequence[str]]) -> List[float]:
        """[(query, passage), ...] -> scores; every passage is encoded in the call."""
        q_no: Dict[str, int] = {}
        d_no: Dict[str, int] = {}
        rows: List[List[int]] = []           # per query, the document numbers of its pairs
        at = []                              # where each pair sits: (query number, place in the query's row)
        for q, d in pairs:
            qi = q_no.setdefault(q, len(q_no))
            if qi == len(rows):
                rows.append([])
            at.append((qi, len(rows[qi])))
            rows[qi].append(d_no.setdefault(d, len(d_no)))
        if not at:
            return []
        table = np.full((len(rows), max(map(len, rows))), -1, dtype=np.int64)
        for qi, row in enumerate(rows):
            table[qi, :len(row)] = row
        out = self._score(list(q_no), list(d_no), table)
        return [float(out[p]) for p in at]

    def postprocess_nodes(self, nodes, query_bundle=None, query_str: Optional[str] = None):
        from .schema import MetadataMode

        if query_bundle is None and query_str is None:
            raise ValueError("Missing query bundle in extra info.")
        q = query_str if query_bundle is None else query_bundle.query_str
        if len(nodes) == 0:
            return []
        stored = np.atleast_2d(self.lookup([n.node.id_ for n in nodes]))
        docs = [None if held else n.node.get_content(metadata_mode=MetadataMode.EMBED)
                for n, held in zip(nodes, (stored >= 0).all(0).tolist())]
        scores = self._score([q], docs, np.arange(len(nodes))[None], stored)[0].tolist()
        for n, s in zip(nodes, scores):
            if self.keep_retrieval_score:
                n.node.metadata["retrieval_score"] = n.score
            n.score = s
        return [nodes[i] for i in descending(scores, self.top_n)]

    _postprocess_nodes = postprocess_nodes

    def rerank(self, query: str, documents: Sequence[str], top_n: Optional[int] = None):
        return rerank_result(self.predict([(query, d) for d in documents]), top_n)
