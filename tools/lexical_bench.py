"""Hybrid (dense + lexical) retrieval timing, for the record: BAAI/bge-m3's geometry (XLM-R large: 24 layers,
1024) with seeded weights, a seeded lexical head and the hashing tokenizer, one MI355X, HIP events, warm-up, median of ``--repeat``.

    python tools/lexical_bench.py [--repeat 20] [--dtype bfloat16] [--scan-docs 1000000] [--out profiles/lexical_bench.jsonl]
    python tools/lexical_bench.py --postings-only [--out profiles/lexical_postings_bench.jsonl]
    python tools/lexical_bench.py --hybrid [--out profiles/hybrid_scan_bench.log]

One JSON line per leg, appended to ``--out``:
  lone_caller_stored   one query against 50 candidates that sit in the ``LexicalStore``: query encode + ``tt_lexical_score`` (lexical,
                       dense and hybrid) between one event pair, and the wall time of ``postprocess_nodes`` (tokenise, encode,
                       score, read back, sort)
  cross_encoder        the cross-encoder reranker of the same box for the same job: BAAI/bge-reranker-v2-m3's geometry, one caller,
                       50 pairs, wall time of ``predict`` -- the number the leg above stands beside (tools/colbert_bench.py's leg)
  lexical_scan         ``tt_lexical_scan_topk`` (k = 50, one query of 8 ids) over ``--scan-docs`` documents of about 150 ids each, and
                       its scoring kernel alone (``tt_lexical_score``, every document): bytes = n_docs * 12 + nnz * 8 against the
                       8 TB/s of the part
  dense_scan           the dense exact-order scan of the same box over ``--scan-docs`` x 1024 bf16 rows, k = 50, one query
  ingest               ``M3Encoder.encode`` against ``embed_token_batches`` on the same 256 passages: the lexical ingest runs the full
                       last layer and the head, CLS pooling runs the last layer for the CLS rows only
  lexical_postings     the same ``--scan-docs`` arrays through both paths of a store in one process: the full
                       scan (``tt_lexical_scan_topk``) and the posting-list path (``postings.search``: host planning, readbacks
                       and all), for one query of 8 ids and for a batch of 64, k = 50, and the one-off ``tt_postings_build``; with
                       the share of the documents that were scored.  The ids are NOT uniform: a document's ids are 3 + the
                       running sum of 100 .. 200 gaps drawn from 1 .. 1249 (mean 625), so every document starts at the low ids and
                       ends between about 62 000 and 125 000 -- lists are about n_docs / 625 long below 62 000, taper to nothing
                       by about 147 000 and are EMPTY above, 45 % of the id range in all; the query ids alone are uniform in 4 ..
                       250 001, so about half of a query's 8 ids have no list; a second pair of lines draws them below 60 000,
                       where every id has a list.  The leg records the profile it met (list length
                       by decile of the id range, the share of ids without a list, the query ids that had one).  Real
                       vocabularies have stopword-like ids whose lists are far longer than any here
  hybrid_scan          (``--hybrid`` only) ``tt_hybrid_scan_topk`` (k = 50) over the same ``--scan-docs`` arrays
                       plus one unit bf16 row of 1024 per document, for 1, 4, 16 and 64 queries of 8 ids, against
                       ``tt_lexical_score`` over the whole store with the dense arguments followed by ``torch.topk``: median, minimum
                       and maximum of ``--repeat`` event pairs each, bytes per sweep (n_docs * (12 + 2048) + nnz * 8) over the
                       scan's time against 8 TB/s, and whether the two top-50 are equal
with the shader clock sampled (amdsmi, read only) while the windows ran.  ``--postings-only`` runs the last leg alone (no model is
built) and writes to ``profiles/lexical_postings_bench.jsonl`` unless ``--out`` says otherwise; ``--hybrid`` likewise runs the
hybrid leg alone and writes to ``profiles/hybrid_scan_bench.log``.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=50)
    ap.add_argument("--passage-words", type=int, default=177)
    ap.add_argument("--scan-docs", type=int, default=1_000_000)
    ap.add_argument("--dtype", default="bfloat16", choices=("bfloat16", "float16"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--postings-only", action="store_true")
    ap.add_argument("--hybrid", action="store_true")
    args = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)

    import numpy as np
    import torch
    from modernbert_bench import _clock_sampler

    from tensor_truth_amd import _lib, lexical
    from tensor_truth_amd import scan as tscan
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank
    from tensor_truth_amd.schema import NodeWithScore, TextNode

    out_path = args.out or os.path.join(os.path.dirname(here), "profiles",
                                        "hybrid_scan_bench.log" if args.hybrid else
                                        "lexical_postings_bench.jsonl" if args.postings_only else "lexical_bench.jsonl")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    words = [f"w{i}" for i in range(5000)]

    def text(n):
        return " ".join(words[i] for i in rng.integers(0, len(words), n))

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")

    def timed(fn):
        """-> (median device ms between an event pair, median wall ms) of ``fn`` over --repeat runs."""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
        return statistics.median(ev), statistics.median(wall)

    def scan_corpus(n_docs, gd):
        """--scan-docs documents of 100 .. 200 ascending ids: 3 + the cumulative sums of gaps drawn from 1 .. 1249, so ids run from 4
        to at most 249 803 and crowd at the low end (every document starts there); weights in 0.01 .. 2.01."""
        nnz = torch.randint(100, 201, (n_docs,), generator=gd, device=dev, dtype=torch.int32)
        d_start = torch.zeros(n_docs, dtype=torch.int64, device=dev)
        d_start[1:] = torch.cumsum(nnz[:-1].to(torch.int64), 0)
        total = int(nnz.sum())
        gaps = torch.randint(1, 1250, (total,), generator=gd, device=dev, dtype=torch.int64)
        run = torch.cumsum(gaps, 0)
        first = torch.repeat_interleave(run[d_start] - gaps[d_start], nnz.to(torch.int64))
        d_terms = (run - first + 3).to(torch.int32)                    # (ascending inside a document: ids 4 .. 249 803)
        del gaps, run, first
        d_weights = torch.rand(total, generator=gd, device=dev) * 2 + 0.01
        return d_terms, d_weights, d_start, nnz, total

    def postings_leg():
        from types import SimpleNamespace

        from tensor_truth_amd import postings

        n_docs, vocab, k = args.scan_docs, 250002, 50
        gd = torch.Generator(device=dev).manual_seed(3)
        d_terms, d_weights, d_start, nnz, total = scan_corpus(n_docs, gd)
        clock = _clock_sampler()
        built = []

        def build():
            built[:] = [postings.postings_build(d_terms, d_weights, d_start, nnz, n_docs, vocab, total)]

        build_ms, _ = timed(build)
        ix = built[0]
        lens = np.diff(ix.off_host)
        deciles = np.array_split(lens, 10)
        profile = dict(list_len_mean_by_id_decile=[round(float(d.mean()), 1) for d in deciles], list_len_max=int(lens.max()),
                       ids_without_list_share=round(float((lens == 0).mean()), 4),
                       highest_id_with_list=int(np.flatnonzero(lens)[-1]) if lens.any() else -1)
        store = SimpleNamespace(terms=d_terms, weights=d_weights, d_start=d_start, d_nnz=nnz, n_docs=n_docs, index=ix, _pws=None, _ws=None,
                                _check_query=lexical.LexicalStore._check_query, stats={})
        # query ids over the whole id range (section 4.17's query: about half of its ids have no list), then below 60 000, where
        # every id has a list of about n_docs / 625
        for n_q, q_hi in ((1, 250002), (64, 250002), (1, 60000), (64, 60000)):
            q_terms = torch.sort(torch.randint(4, q_hi, (n_q, 8), generator=gd, device=dev, dtype=torch.int32), dim=1).values.reshape(-1)
            q_weights = torch.rand(n_q * 8, generator=gd, device=dev) + 0.5
            lw = lexical.LexicalWeights(q_terms.contiguous(), q_weights, np.arange(n_q, dtype=np.int64) * 8, np.full(n_q, 8, dtype=np.int32))
            ws = torch.empty(int(_lib.load_library().tt_lexical_scan_workspace_bytes(n_docs, n_q)), dtype=torch.uint8, device=dev)
            qs = lw.starts.astype(np.int32)
            scan = lambda: lexical.lexical_scan_topk(lw.terms, lw.weights, qs, lw.nnz, d_terms, d_weights, d_start, nnz, k, workspace=ws)  # noqa: E731
            want, got = scan(), postings.search(store, lw, k)
            same = bool(torch.equal(want[1], got[1]) and torch.equal(want[0].view(torch.int32), got[0].view(torch.int32)))
            scan_ms, scan_wall = timed(scan)
            post_ms, post_wall = timed(lambda: postings.search(store, lw, k))
            st = dict(store.stats)
            q_lens = lens[q_terms.cpu().numpy().astype(np.int64)].reshape(n_q, 8)
            emit(leg="lexical_postings", n_docs=n_docs, nnz=total, vocab=vocab,
                 ids="document ids: 3 + cumulative sums of 100..200 gaps uniform in 1..1249 (crowded below 62k, thinning out to none by ~147k); "
                     f"query ids: uniform in 4..{q_hi - 1}", query_id_below=q_hi, k=k, queries=n_q, query_ids=8,
                 scan_topk_ms=round(scan_ms, 4), scan_topk_wall_ms=round(scan_wall, 4), postings_ms=round(post_ms, 4),
                 postings_wall_ms=round(post_wall, 4), build_ms=round(build_ms, 3), index_bytes=ix.nbytes, prunable=ix.prunable,
                 same_bits_as_scan=same, candidates=st["candidates"], passes=st["passes"], fallbacks=st["fallbacks"],
                 query_ids_with_list_mean=round(float((q_lens > 0).sum(1).mean()), 3),
                 query_list_len_sum_mean=round(float(q_lens.sum(1).mean()), 1),
                 query_list_lens=q_lens[0].tolist() if n_q == 1 else None, **profile,
                 candidate_share=round(st["candidates"] / (n_q * n_docs), 6), sclk_mhz=clock(), repeat=args.repeat,
                 warmup=args.warmup)
            del ws

    def hybrid_leg():
        """the hybrid scan against what the library could do before it -- ``tt_lexical_score`` over the whole
        store with the dense arguments, then ``torch.topk`` -- on the corpus above plus one unit bf16 row of 1024 per document."""
        n_docs, dim, k, hw = args.scan_docs, 1024, 50, (0.4, 0.2)
        gd = torch.Generator(device=dev).manual_seed(3)
        d_terms, d_weights, d_start, nnz, total = scan_corpus(n_docs, gd)
        d_dense = torch.empty((n_docs, dim), dtype=torch.bfloat16, device=dev)
        for lo in range(0, n_docs, 1 << 17):      # (in pieces: the fp32 image of the whole corpus is never held)
            n = min(1 << 17, n_docs - lo)
            d_dense[lo:lo + n] = torch.nn.functional.normalize(torch.randn(n, dim, generator=gd, device=dev), dim=-1).to(torch.bfloat16)
        nbytes = n_docs * (12 + 2 * dim) + total * 8

        def spread(fn):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ev = []
            for _ in range(args.repeat):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ev.append(a.elapsed_time(b))
            return statistics.median(ev), min(ev), max(ev)

        for n_q in (1, 4, 16, 64):
            q_terms = torch.sort(torch.randint(4, 250002, (n_q, 8), generator=gd, device=dev, dtype=torch.int32), dim=1).values.reshape(-1)
            q_terms = q_terms.contiguous()
            q_weights = torch.rand(n_q * 8, generator=gd, device=dev) + 0.5
            q_dense = torch.nn.functional.normalize(torch.randn(n_q, dim, generator=gd, device=dev), dim=-1).to(torch.bfloat16)
            qs, qn = np.arange(n_q, dtype=np.int32) * 8, np.full(n_q, 8, dtype=np.int32)
            qs_t, qn_t = torch.from_numpy(qs).to(dev), torch.from_numpy(qn).to(dev)
            ws = torch.empty(int(_lib.load_library().tt_hybrid_scan_workspace_bytes(n_docs, n_q)), dtype=torch.uint8, device=dev)
            scan = lambda: lexical.hybrid_scan_topk(q_terms, q_weights, qs_t, qn_t, d_terms, d_weights, d_start, nnz, q_dense, d_dense,  # noqa: E731
                                                    hw, k, workspace=ws, max_q_nnz=8)
            base = lambda: torch.topk(lexical.lexical_score(q_terms, q_weights, qs_t, qn_t, d_terms, d_weights, d_start, nnz,  # noqa: E731
                                                            q_dense=q_dense, d_dense=d_dense, hybrid_weights=hw)[2], k, dim=1)
            got, want = scan(), base()
            same_scores = bool(torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)))
            same_docs = bool(torch.equal(got[1].to(torch.int64), want[1]))
            clock = _clock_sampler()
            s_med, s_min, s_max = spread(scan)
            b_med, b_min, b_max = spread(base)
            # what the selection costs at this size: the lexical scan of the same queries (scoring + the same selection) less its
            # scoring kernel alone -- an estimate by subtraction, not a timing of the selection itself
            lws = torch.empty(int(_lib.load_library().tt_lexical_scan_workspace_bytes(n_docs, n_q)), dtype=torch.uint8, device=dev)
            ls_med, _, _ = spread(lambda: lexical.lexical_scan_topk(q_terms, q_weights, qs_t, qn_t, d_terms, d_weights, d_start, nnz, k,
                                                                    workspace=lws))
            lk_med, _, _ = spread(lambda: lexical.lexical_score(q_terms, q_weights, qs_t, qn_t, d_terms, d_weights, d_start, nnz))
            del lws
            emit(leg="hybrid_scan", selection_ms_by_subtraction=round(ls_med - lk_med, 4),
                 scoring_ms_by_subtraction=round(s_med - (ls_med - lk_med), 4), n_docs=n_docs, nnz=total, dim=dim, k=k, queries=n_q, query_ids=8, bytes_per_sweep=nbytes,
                 scan_ms=round(s_med, 4), scan_min_ms=round(s_min, 4), scan_max_ms=round(s_max, 4),
                 baseline_ms=round(b_med, 4), baseline_min_ms=round(b_min, 4), baseline_max_ms=round(b_max, 4),
                 sweep_fraction_of_8_tb_per_s=round(nbytes / s_med / 1e9 / 8.0, 4), baseline_over_scan=round(b_med / s_med, 3),
                 same_top_k_scores=same_scores, same_top_k_documents=same_docs, sclk_mhz=clock(), repeat=args.repeat,
                 warmup=args.warmup)
            del ws

    if args.hybrid:
        hybrid_leg()
        return
    if args.postings_only:
        postings_leg()
        return

    emb = HipHuggingFaceEmbedding(model_name="BAAI/bge-m3", device="cuda:0", model_kwargs=dict(synthetic_seed=3, torch_dtype=args.dtype))
    H = emb.config.hidden
    g = torch.Generator().manual_seed(11)
    head = (torch.randn(H, generator=g) * 0.05, -0.2)
    rr = lexical.HipM3HybridRerank(model="BAAI/bge-m3", top_n=10, model_kwargs=dict(hybrid_weights=(0.4, 0.2), embedder=emb,
                                                                                     sparse_head=head))
    query = text(9)
    passages = [text(args.passage_words) for _ in range(args.candidates)]

    def nodes(prefix):
        return [NodeWithScore(node=TextNode(text=t, id_=f"{prefix}{i}"), score=0.0) for i, t in enumerate(passages)]

    rr.index_nodes(nodes("s"))
    stored = rr.store.lookup([f"s{i}" for i in range(args.candidates)])[None]
    base = dict(dtype=args.dtype, layers=emb.config.layers, hidden=H, candidates=args.candidates,
                ids_per_passage=int(rr.store.n_terms / args.candidates), repeat=args.repeat)

    def encode_and_score():
        q_dense, q_lw = rr.encoder.encode([query], is_query=True)
        return rr.store.score(q_lw, stored, dense=q_dense, hybrid_weights=rr.hybrid_weights)

    clock = _clock_sampler()
    dev_ms, _ = timed(encode_and_score)
    _, wall_ms = timed(lambda: rr.postprocess_nodes(nodes("s"), query_str=query))
    emit(leg="lone_caller_stored", encode_plus_score_ms=round(dev_ms, 3), postprocess_nodes_wall_ms=round(wall_ms, 3),
         store_bytes=rr.store.nbytes, sclk_mhz=clock(), **base)

    # ingest: the same 256 passages through the lexical encoder and through the embedder's own CLS path
    batch = emb._tokenize([text(args.passage_words) for _ in range(256)], "")
    clock = _clock_sampler()
    m3_ms, _ = timed(lambda: rr.encoder.encode(batch, is_query=False))
    cls_ms, _ = timed(lambda: emb.embed_token_batches(batch))
    emit(leg="ingest", passages=len(batch), tokens=int(sum(len(s) for s in batch)), m3_encode_ms=round(m3_ms, 3),
         embed_token_batches_ms=round(cls_ms, 3), ratio=round(m3_ms / cls_ms, 3), sclk_mhz=clock(), dtype=args.dtype, repeat=args.repeat)

    # the cross-encoder of the same box for the same job (one caller, the coalescing front off: nobody to share a batch with)
    ce = HipSentenceTransformerRerank(model="BAAI/bge-reranker-v2-m3", top_n=10, device="cuda:0", coalesce=False,
                                      model_kwargs=dict(synthetic_seed=1, torch_dtype=args.dtype))
    ce_pairs = [(query, text(280)) for _ in range(args.candidates)]
    clock = _clock_sampler()
    dev_ms, wall_ms = timed(lambda: ce.predict(ce_pairs))
    emit(leg="cross_encoder", model="BAAI/bge-reranker-v2-m3 geometry (24 layers, 1024)", predict_event_ms=round(dev_ms, 3),
         predict_wall_ms=round(wall_ms, 3), pairs=args.candidates, tokens_per_pair=int(ce.stats["tokens"] / max(ce.stats["pairs"], 1)),
         sclk_mhz=clock(), dtype=args.dtype, repeat=args.repeat)
    del ce, rr, emb
    torch.cuda.empty_cache()

    # the full lexical scan
    n_docs = args.scan_docs
    gd = torch.Generator(device=dev).manual_seed(3)
    d_terms, d_weights, d_start, nnz, total = scan_corpus(n_docs, gd)
    q_terms = torch.sort(torch.randint(4, 250002, (8,), generator=gd, device=dev, dtype=torch.int32)).values
    q_weights = torch.rand(8, generator=gd, device=dev) + 0.5
    q_start, q_nnz = np.zeros(1, dtype=np.int32), np.full(1, 8, dtype=np.int32)
    ws = torch.empty(int(_lib.load_library().tt_lexical_scan_workspace_bytes(n_docs, 1)), dtype=torch.uint8, device=dev)
    qs_t, qn_t = torch.from_numpy(q_start).to(dev), torch.from_numpy(q_nnz).to(dev)
    nbytes = n_docs * 12 + total * 8
    clock = _clock_sampler()
    scan_ms, _ = timed(lambda: lexical.lexical_scan_topk(q_terms, q_weights, qs_t, qn_t, d_terms, d_weights, d_start, nnz, 50, workspace=ws))
    score_ms, _ = timed(lambda: lexical.lexical_score(q_terms, q_weights, qs_t, qn_t, d_terms, d_weights, d_start, nnz))
    emit(leg="lexical_scan", n_docs=n_docs, nnz=total, k=50, query_ids=8, bytes=nbytes, scan_topk_ms=round(scan_ms, 4),
         score_kernel_ms=round(score_ms, 4), scan_tb_per_s=round(nbytes / scan_ms / 1e9, 3),
         scan_fraction_of_8_tb_per_s=round(nbytes / scan_ms / 1e9 / 8.0, 4), score_tb_per_s=round(nbytes / score_ms / 1e9, 3),
         score_fraction_of_8_tb_per_s=round(nbytes / score_ms / 1e9 / 8.0, 4), sclk_mhz=clock(), repeat=args.repeat)
    del d_terms, d_weights, d_start, nnz, ws
    torch.cuda.empty_cache()

    # the dense scan of the same box: --scan-docs x 1024 bf16 rows, one query, k = 50
    corpus = torch.nn.functional.normalize(torch.randn(n_docs, 1024, generator=gd, device=dev), dim=-1).to(torch.bfloat16)
    qv = torch.nn.functional.normalize(torch.randn(1, 1024, generator=gd, device=dev), dim=-1).to(torch.bfloat16)
    clock = _clock_sampler()
    dense_ms, _ = timed(lambda: tscan.scan_topk(corpus, qv, 50))
    dbytes = corpus.numel() * 2
    emit(leg="dense_scan", n_docs=n_docs, dim=1024, k=50, bytes=dbytes, scan_topk_ms=round(dense_ms, 4),
         tb_per_s=round(dbytes / dense_ms / 1e9, 3), fraction_of_8_tb_per_s=round(dbytes / dense_ms / 1e9 / 8.0, 4), sclk_mhz=clock(),
         repeat=args.repeat)
    del corpus, qv
    torch.cuda.empty_cache()
    postings_leg()


if __name__ == "__main__":
    main()
