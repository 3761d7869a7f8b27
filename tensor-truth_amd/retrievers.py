"""Host-side retriever logic around the GPU retriever: multi-index fan-out + balancing,
auto-merging, similarity cutoff.  Pure Python (lists of at most a few hundred nodes) -- these
restate the reference's control flow so the HIP retriever drops into the same pipeline.
"""
from __future__ import annotations

import threading
from collections import OrderedDict, defaultdict
from concurrent.futures import ThreadPoolExecutor, as_completed
from functools import lru_cache
from typing import Dict, List, Optional

from .schema import NodeWithScore, QueryBundle, as_query_bundle


def similarity_top_k_for(reranker_top_n: int) -> int:
    """Candidate-pool size per index (reference: rag_engine.py:592-593)."""
    return max(5, reranker_top_n * 2)


def _node_metadata(node):
    inner = getattr(node, "node", None)
    if inner is not None and isinstance(getattr(inner, "metadata", None), dict):
        return inner.metadata
    md = getattr(node, "metadata", None)
    return md if isinstance(md, dict) else None


class MultiIndexRetriever:
    """Queries several index retrievers concurrently and balances their contributions.

    Behaviour of the reference class (``src/tensortruth/rag_engine.py:368-527``): one task per
    retriever on a thread pool (``min(len, 8)`` workers), results concatenated in completion
    order, every node tagged ``metadata["_source_index"] = idx``; a failing retriever is
    reported and skipped; with more than one retriever and ``balance_strategy ==
    "top_k_per_index"`` each index keeps its first ``max(1, total // n_indexes)`` nodes and
    the union is re-sorted by score (missing score = 0.0) descending; an LRU cache keyed on
    the query string (default 128 entries) short-circuits repeated queries.
    """

    def __init__(self, retrievers: List, max_workers: Optional[int] = None, enable_cache: bool = True,
                 cache_size: int = 128, balance_strategy: str = "top_k_per_index",
                 share_query_embedding: bool = True, single_pass: bool = True) -> None:
        self.retrievers = retrievers
        self.max_workers = max_workers or min(len(retrievers), 8)
        self.enable_cache = enable_cache
        self.balance_strategy = balance_strategy
        # The reference embeds the query once PER INDEX (every VectorIndexRetriever calls the embed model itself,
        # SURVEY.md section 8 row a4).  When every retriever searches with the same embed-model object the embedding
        # is computed once here and handed down in the QueryBundle: same vectors, n_indexes x fewer encoder passes.
        self.share_query_embedding = share_query_embedding
        # When every retriever is a HipVectorRetriever (directly or under an AutoMergingRetriever) on one
        # device, the module matrices are packed into one (HipIndexGroup) and searched with ONE pass
        # (tt_scan_topk_segmented) instead of one search per worker thread; per-module results, auto-merging,
        # tagging and balancing are unchanged.  Anything unexpected falls back to the thread pool.
        self.single_pass = single_pass
        self._group = None
        self._group_lock = threading.Lock()
        # concurrent callers (the reference's request threads, rag_engine.py:392) share ONE pass over the packed matrix: a lone caller
        # runs at once, alone (per-module fp8-shadow passes); what queues up behind a running scan goes out as one batch
        from .coalesce import Coalescer

        self._scan_front = Coalescer(self._group_scan_many, max_batch=64)
        if enable_cache:
            self._retrieve_cached = lru_cache(maxsize=cache_size)(self._retrieve_impl)
        else:
            self._retrieve_cached = self._retrieve_impl

    def _shared_embed_model(self):
        models = []
        for r in self.retrievers:
            base = getattr(r, "_vector_retriever", r)            # AutoMergingRetriever wraps the index retriever
            em = getattr(getattr(base, "index", None), "embed_model", None)
            if em is None or not hasattr(em, "get_agg_embedding_from_queries"):
                return None
            models.append(em)
        return models[0] if models and all(m is models[0] for m in models) else None

    def _retrieve_impl(self, query_text: str):
        bundle = QueryBundle(query_str=query_text)
        if self.share_query_embedding and len(self.retrievers) > 1:
            em = self._shared_embed_model()
            if em is not None:
                try:
                    bundle.embedding = list(em.get_agg_embedding_from_queries(bundle.embedding_strs))
                except Exception:  # noqa: BLE001 - fall back to per-index embedding, as the reference does it
                    bundle.embedding = None
        combined = []
        per_index = None
        if self.single_pass and len(self.retrievers) > 1 and bundle.embedding is not None:
            try:
                per_index = self._single_pass_retrieve(bundle)
            except Exception as exc:  # noqa: BLE001 - the per-index path below degrades per retriever
                print(f"Single-pass retrieval unavailable ({exc}); using one search per index")
                per_index = None
        if per_index is not None:
            for i, nodes in enumerate(per_index):
                for n in nodes:
                    md = _node_metadata(n)
                    if md is not None:
                        md["_source_index"] = i
                combined.extend(nodes)
        else:
            with ThreadPoolExecutor(max_workers=max(1, self.max_workers)) as pool:
                futures = {pool.submit(r.retrieve, bundle): i for i, r in enumerate(self.retrievers)}
                for fut in as_completed(futures):
                    try:
                        nodes = fut.result()
                    except Exception as exc:  # noqa: BLE001 - degrade like the reference (rag_engine.py:453-455)
                        print(f"Retriever failed: {exc}")
                        continue
                    for n in nodes:
                        md = _node_metadata(n)
                        if md is not None:
                            md["_source_index"] = futures[fut]
                    combined.extend(nodes)
        if len(self.retrievers) > 1 and self.balance_strategy == "top_k_per_index":
            combined = self._balance_top_k_per_index(combined)
        return combined

    def _single_pass_retrieve(self, bundle):
        """One segmented scan for all modules -> per-retriever node lists, or None when the retrievers are not
        all HIP index retrievers on one device."""
        import torch

        from .vector_index import HipIndexGroup, HipVectorRetriever

        bases = [getattr(r, "_vector_retriever", r) for r in self.retrievers]
        if not all(isinstance(b, HipVectorRetriever) for b in bases) or len(bases) > 64:
            return None
        # the packed scan answers plain top-k only: a retriever in MMR mode runs its own search (the thread pool path)
        if any(getattr(b, "query_mode", "default") == "mmr" for b in bases):
            return None
        indexes = [b.index for b in bases]
        if len({(ix.dim, ix.device) for ix in indexes}) != 1 or len({id(ix) for ix in indexes}) != len(indexes):
            return None
        # one pass applies ONE metadata filter to every module: only when all retrievers carry the same one
        fkeys = {getattr(b, "filter_key", None) for b in bases}
        if len(fkeys) != 1:
            return None
        fkey = fkeys.pop()
        filters = bases[0].filters if fkey is not None else None
        with self._group_lock:   # retrieve() is called from several threads (rag_engine.py:392,420)
            if self._group is None or [id(ix) for ix in self._group.indexes] != [id(ix) for ix in indexes]:
                self._group = HipIndexGroup(indexes)
            group = self._group
        k = max(min(b.similarity_top_k, ix.num_live) for b, ix in zip(bases, indexes))
        if k < 1:
            return [[] for _ in bases]
        scores, rows, snap_ids = self._scan_front.submit((group, bundle.embedding, k, fkey, filters))
        out = []
        for i, (r, b) in enumerate(zip(self.retrievers, bases)):
            kk = min(b.similarity_top_k, indexes[i].num_live)
            nodes = b.nodes_from_hits(scores[i][:kk], rows[i][:kk], snap_ids[i])
            out.append(r.merge(nodes) if r is not b and hasattr(r, "merge") else nodes)
        return out

    @staticmethod
    def _group_scan_many(items):
        """[(group, query embedding, k[, filter key, filters])] -> [(scores [S][k'], rows [S][k'], id lists)]: one
        ``HipIndexGroup.search_host`` per (group, filter key) with k' = the largest k asked for -- an exact top-k list is a prefix of
        every longer one (score descending, row ascending among equals), and every caller slices its own k per module."""
        import torch

        out = [None] * len(items)
        by_group = {}
        for i, it in enumerate(items):
            fkey = it[3] if len(it) > 3 else None
            by_group.setdefault((id(it[0]), fkey), (it[0], it[4] if len(it) > 4 else None, []))[2].append(i)
        for group, filters, members in by_group.values():
            k = max(items[i][2] for i in members)
            q = torch.tensor([items[i][1] for i in members], dtype=torch.float32)
            scores, rows, ids = group.search_host(q, k) if filters is None else group.search_host(q, k, filters=filters)
            scores, rows = scores.tolist(), rows.tolist()
            for j, i in enumerate(members):
                out[i] = (scores[j], rows[j], ids)
        return out

    def _balance_top_k_per_index(self, nodes: List[NodeWithScore]) -> List[NodeWithScore]:
        groups: Dict[int, list] = defaultdict(list)
        for n in nodes:
            md = _node_metadata(n)
            groups[md.get("_source_index", 0) if md else 0].append(n)
        if not groups:
            return []
        limit = max(1, len(nodes) // len(groups))
        kept = []
        for members in groups.values():
            kept.extend(members[:limit])
        kept.sort(key=lambda n: n.score if n.score else 0.0, reverse=True)
        return kept

    def retrieve(self, query) -> List[NodeWithScore]:
        return self._retrieve(as_query_bundle(query))

    def _retrieve(self, query_bundle) -> List[NodeWithScore]:
        return self._retrieve_cached(query_bundle.query_str)

    def clear_cache(self) -> None:
        if self.enable_cache and hasattr(self._retrieve_cached, "cache_clear"):
            self._retrieve_cached.cache_clear()


class AutoMergingRetriever:
    """Merges retrieved leaves into their parent when most of the parent's children were hit.

    Restates llama-index ``AutoMergingRetriever`` as the reference builds it
    (``rag_engine.py:641-643``): ``simple_ratio_thresh = 0.5``; loop
    {fill in single gaps between retrieved neighbours (score = mean of the two), replace
    children by their parent when ``hits / len(parent.children) > ratio`` (score = mean of the
    children)} until nothing changes; final sort by score descending.  ``docstore`` maps node id
    -> node with ``parent_id / child_ids / prev_id / next_id`` links.
    """

    def __init__(self, vector_retriever, docstore, simple_ratio_thresh: float = 0.5, verbose: bool = False):
        self._vector_retriever = vector_retriever
        self._docstore = docstore.docstore if hasattr(docstore, "docstore") and isinstance(
            getattr(docstore, "docstore"), dict) else docstore
        self._ratio = simple_ratio_thresh
        self._verbose = verbose

    def _get(self, node_id):
        ds = self._docstore
        return ds.get(node_id) if hasattr(ds, "get") else ds[node_id]

    def _merge_parents(self, nodes: List[NodeWithScore]):
        by_parent: Dict[str, List[NodeWithScore]] = OrderedDict()
        for n in nodes:
            pid = getattr(n.node, "parent_id", None)
            if pid is not None:
                by_parent.setdefault(pid, []).append(n)
        drop, add, changed = set(), [], False
        for pid, hits in by_parent.items():
            parent = self._get(pid)
            if parent is None:
                continue
            children = list(getattr(parent, "child_ids", []) or [])
            if not children:
                continue
            if len(hits) / len(children) > self._ratio:
                drop.update(h.node.id_ for h in hits)
                score = sum((h.score or 0.0) for h in hits) / len(hits)
                add.append(NodeWithScore(node=parent, score=score))
                changed = True
        out = [n for n in nodes if n.node.id_ not in drop]
        present = {n.node.id_ for n in out}
        for a in add:
            if a.node.id_ not in present:
                out.append(a)
                present.add(a.node.id_)
        return out, changed

    def _fill_in(self, nodes: List[NodeWithScore]):
        out, changed = [], False
        present = {n.node.id_ for n in nodes}
        for i, cur in enumerate(nodes):
            out.append(cur)
            if i + 1 >= len(nodes):
                continue
            nxt = nodes[i + 1]
            gap = getattr(cur.node, "next_id", None)
            if gap is not None and gap == getattr(nxt.node, "prev_id", None) and gap not in present:
                mid = self._get(gap)
                if mid is not None:
                    out.append(NodeWithScore(node=mid, score=((cur.score or 0.0) + (nxt.score or 0.0)) / 2))
                    present.add(gap)
                    changed = True
        return out, changed

    def _try_merging(self, nodes):
        nodes, c1 = self._fill_in(nodes)
        nodes, c2 = self._merge_parents(nodes)
        return nodes, (c1 or c2)

    def retrieve(self, query) -> List[NodeWithScore]:
        return self.merge(self._vector_retriever.retrieve(as_query_bundle(query)))

    def merge(self, nodes: List[NodeWithScore]) -> List[NodeWithScore]:
        """Fill-in + parent merging to a fixpoint over already-retrieved leaves."""
        nodes, changed = self._try_merging(nodes)
        while changed:
            nodes, changed = self._try_merging(nodes)
        nodes.sort(key=lambda n: n.score if n.score is not None else 0.0, reverse=True)
        return nodes

    _retrieve = retrieve


class SimilarityPostprocessor:
    """Drops nodes scoring below ``similarity_cutoff`` (reference wiring: rag_engine.py:717-726)."""

    def __init__(self, similarity_cutoff: Optional[float] = None):
        self.similarity_cutoff = similarity_cutoff

    def postprocess_nodes(self, nodes, query_bundle=None, query_str=None):
        if self.similarity_cutoff is None:
            return list(nodes)
        return [n for n in nodes if n.score is not None and n.score >= self.similarity_cutoff]

    _postprocess_nodes = postprocess_nodes
