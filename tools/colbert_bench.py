"""Late-interaction rerank timing, for the record: colbert-ir/colbertv2.0's geometry (BERT-base, 12 layers,
768 -> 128, 32-token queries, 180-token passages) with seeded weights and the hashing tokenizer, one MI355X, HIP events, warm-up,
median of ``--repeat``.

    python tools/colbert_bench.py [--repeat 20] [--dtype bfloat16] [--out profiles/colbert_bench.jsonl]

One JSON line per leg, appended to ``--out``:
  lone_caller_stored     one query against 50 candidates whose token vectors are in the store: query encode + MaxSim between one
                         event pair, and the wall time of ``postprocess_nodes`` (tokenise, encode, score, read back, sort)
  lone_caller_in_call    the same 50 passages encoded in the call (nothing stored)
  maxsim_256x50          ``tt_maxsim`` alone: 256 queries x 50 candidates each, every (query, candidate) a different passage of a
                         12 800-passage store, so the bytes are HBM bytes: achieved bytes/s against the 8 TB/s of the part
  cross_encoder          the cross-encoder reranker of the same box for the same job: BAAI/bge-reranker-v2-m3's geometry (24 layers,
                         1024), one caller, 50 pairs, wall time of ``predict`` -- the number the legs above stand beside
with the shader clock sampled (amdsmi, read only) while the windows ran.

    python tools/colbert_bench.py --scan [--scan-docs 92000] [--scan-log profiles/maxsim_scan_bench.log]

runs only the exact-retrieval leg (``scan_leg`` below): ``tt_maxsim_scan_topk`` against ``tt_maxsim`` with
``cand == NULL`` + ``torch.topk`` over a store of at least 4 GB, n_q in {1, 4, 8, 16}, k = 50, and rewrites ``--scan-log``.
"""
import argparse
import json
import os
import statistics
import sys
import time


HBM_PEAK_TB_S = 8.0      # the part's HBM3E peak, the denominator of every "fraction of the roof" here


def scan_leg(args, log_path):
    """Exact retrieval over a store that does not fit the 256 MiB Infinity Cache: ``--scan-docs`` passages of 180 unit vectors at dim
    128 (>= 4 GB), 32-token queries, k = 50, n_q in {1, 4, 8, 16}.  At every point two things are timed with the same procedure
    (warm-up, one HIP event pair per repetition, median and min .. max over ``--repeat``):
      scan      ``colbert.maxsim_scan_topk``: one sweep of the store per 8 queries, then the library's selection
      baseline  what the library could do before: ``colbert.maxsim`` with ``cand == NULL`` over the whole store (one workgroup per
                (document, query): the store is read once per query), then ``torch.topk``
    Per sweep: the store's vector bytes / time against the HBM peak, and the MFMA flops / time.  The log states, per point, whether
    the expectation holds: at n_q = 1 the scan takes no longer than the baseline within the measured spread; from n_q = 4 up it is
    faster by more than that spread."""
    import numpy as np
    import torch
    from modernbert_bench import _clock_sampler

    from tensor_truth_amd import _lib, colbert

    dev = torch.device("cuda", 0)
    dt = getattr(torch, args.dtype)
    n_docs, d_len, q_len, dim, k = args.scan_docs, 180, 32, 128, 50
    g = torch.Generator(device=dev).manual_seed(3)
    d = torch.empty(n_docs * d_len, dim, dtype=dt, device=dev)
    step = 1 << 21
    for lo in range(0, d.shape[0], step):      # (in slices: the fp32 draw of the whole store would double the footprint)
        n = min(step, d.shape[0] - lo)
        d[lo:lo + n] = torch.nn.functional.normalize(torch.randn(n, dim, generator=g, device=dev), dim=-1).to(dt)
    to = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=t)  # noqa: E731
    ds, dl = to(np.arange(n_docs, dtype=np.int64) * d_len, torch.int64), to(np.full(n_docs, d_len), torch.int32)
    store_bytes = d.numel() * 2
    ws = torch.empty(int(_lib.load_library().tt_maxsim_scan_workspace_bytes(n_docs, 16)), dtype=torch.uint8, device=dev)

    def timed(fn):
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

    lines = [f"# tools/colbert_bench.py --scan: {n_docs} passages x {d_len} tokens x dim {dim} {args.dtype} = {store_bytes / 1e9:.3f} GB of "
             f"vectors (Infinity Cache: 0.268 GB), {q_len}-token queries, k = {k}; warm-up {args.warmup}, {args.repeat} repetitions, one "
             "HIP event pair each; ms are median [min .. max]; spread = the larger (max - min) of the two sides",
             f"# HBM fraction = vector bytes read / time / {HBM_PEAK_TB_S} TB/s (scan: one sweep per 8 queries; baseline: one read per "
             "query); TFLOP/s = 2 * dim * q_len * tokens * n_q / time"]
    for n_q in (1, 4, 8, 16):
        q = torch.nn.functional.normalize(torch.randn(n_q * q_len, dim, generator=g, device=dev), dim=-1).to(dt)
        qs, ql = to(np.arange(n_q) * q_len, torch.int32), to(np.full(n_q, q_len), torch.int32)

        def scan():
            return colbert.maxsim_scan_topk(q, qs, ql, d, ds, dl, k, workspace=ws)

        def baseline():
            return torch.topk(colbert.maxsim(q, qs, ql, d, ds, dl), k, dim=1)

        got, want = scan()[0], baseline()[0]
        same = bool(torch.equal(got, want))
        clock = _clock_sampler()
        s_med, s_min, s_max = timed(scan)
        s_clk = clock()
        clock = _clock_sampler()
        b_med, b_min, b_max = timed(baseline)
        b_clk = clock()
        sweeps = (n_q + 7) // 8
        flops = 2.0 * dim * q_len * n_docs * d_len * n_q
        spread = max(s_max - s_min, b_max - b_min)
        if n_q == 1:
            verdict = "confirmed" if s_med <= b_med + spread else "REFUTED"
            claim = "scan no slower than the baseline within the spread"
        else:
            verdict = "confirmed" if b_med - s_med > spread else "REFUTED"
            claim = "scan faster than the baseline by more than the spread"
        rec = dict(leg="maxsim_scan", n_q=n_q, k=k, n_docs=n_docs, tokens_per_passage=d_len, dim=dim, dtype=args.dtype,
                   store_gb=round(store_bytes / 1e9, 3), sweeps=sweeps, repeat=args.repeat, scores_equal=same,
                   scan_ms=round(s_med, 3), scan_min_ms=round(s_min, 3), scan_max_ms=round(s_max, 3),
                   scan_hbm_fraction=round(sweeps * store_bytes / s_med / 1e9 / HBM_PEAK_TB_S, 3), scan_tflops=round(flops / s_med / 1e9, 1),
                   scan_sclk_mhz=s_clk, baseline_ms=round(b_med, 3), baseline_min_ms=round(b_min, 3), baseline_max_ms=round(b_max, 3),
                   baseline_hbm_fraction=round(n_q * store_bytes / b_med / 1e9 / HBM_PEAK_TB_S, 3),
                   baseline_tflops=round(flops / b_med / 1e9, 1), baseline_sclk_mhz=b_clk, spread_ms=round(spread, 3),
                   baseline_over_scan=round(b_med / s_med, 2), expectation=f"{claim}: {verdict}")
        lines.append(f"n_q {n_q:2d}: scan {s_med:8.3f} ms [{s_min:.3f} .. {s_max:.3f}] {rec['scan_hbm_fraction']:.3f} of HBM peak per sweep "
                     f"({sweeps} sweep{'s' if sweeps > 1 else ''}) {rec['scan_tflops']:.1f} TFLOP/s sclk {s_clk} | baseline {b_med:8.3f} ms "
                     f"[{b_min:.3f} .. {b_max:.3f}] {rec['baseline_hbm_fraction']:.3f} of HBM peak x {n_q} reads {rec['baseline_tflops']:.1f} "
                     f"TFLOP/s sclk {b_clk} | spread {spread:.3f} ms | baseline / scan {rec['baseline_over_scan']:.2f} | top-{k} scores equal: "
                     f"{same} | {claim}: {verdict}")
        lines.append(json.dumps(rec))
        print(lines[-2], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
    with open(log_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=50)
    ap.add_argument("--passage-words", type=int, default=177)
    ap.add_argument("--dtype", default="bfloat16", choices=("bfloat16", "float16"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--scan", action="store_true", help="only the exact-retrieval leg (tt_maxsim_scan_topk against tt_maxsim + torch.topk)")
    ap.add_argument("--scan-docs", type=int, default=92_000, help="180-token passages at dim 128: 46 080 bytes each (92 000: 4.24 GB)")
    ap.add_argument("--scan-log", default=None)
    args = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)

    import numpy as np
    import torch
    from modernbert_bench import _clock_sampler

    from tensor_truth_amd import colbert
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank
    from tensor_truth_amd.schema import NodeWithScore, TextNode

    out_path = args.out or os.path.join(os.path.dirname(here), "profiles", "colbert_bench.jsonl")
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

    if args.scan:
        scan_leg(args, os.path.join(os.path.dirname(here), "profiles", "maxsim_scan_bench.log") if args.scan_log is None else args.scan_log)
        return

    settings = dict(synthetic_seed=9, encoder_config=colbert.COLBERT_V2, dim=128, query_length=32, document_length=180,
                    attend_to_expansion_tokens=False, mask_punctuation=False, similarity="cosine", torch_dtype=args.dtype)
    rr = colbert.HipColbertRerank(model="colbert-ir/colbertv2.0", top_n=10, device="cuda:0", model_kwargs=settings)
    query = text(9)
    passages = [text(args.passage_words) for _ in range(args.candidates)]

    def nodes(prefix):
        return [NodeWithScore(node=TextNode(text=t, id_=f"{prefix}{i}"), score=0.0) for i, t in enumerate(passages)]

    rr.index_nodes(nodes("s"))
    stored = rr.store.lookup([f"s{i}" for i in range(args.candidates)])[None]
    base = dict(dtype=args.dtype, layers=12, hidden=768, dim=128, query_length=32, candidates=args.candidates,
                tokens_per_passage=int(rr.store.n_tokens / args.candidates), repeat=args.repeat)

    clock = _clock_sampler()
    dev_ms, _ = timed(lambda: rr.store.score(rr.encoder.encode_queries([query]), stored))
    _, wall_ms = timed(lambda: rr.postprocess_nodes(nodes("s"), query_str=query))
    emit(leg="lone_caller_stored", encode_plus_maxsim_ms=round(dev_ms, 3), postprocess_nodes_wall_ms=round(wall_ms, 3),
         store_bytes=rr.store.nbytes, sclk_mhz=clock(), **base)

    clock = _clock_sampler()
    dev_ms, wall_ms = timed(lambda: rr.postprocess_nodes(nodes("fresh"), query_str=query))
    emit(leg="lone_caller_in_call", postprocess_nodes_event_ms=round(dev_ms, 3), postprocess_nodes_wall_ms=round(wall_ms, 3),
         sclk_mhz=clock(), **base)

    # MaxSim alone over HBM-resident vectors: 256 x 50 different passages
    n_q, n_c, d_len, dim = 256, args.candidates, 180, 128
    dt = getattr(torch, args.dtype)
    g = torch.Generator(device=dev).manual_seed(3)
    d = torch.nn.functional.normalize(torch.randn(n_q * n_c * d_len, dim, generator=g, device=dev), dim=-1).to(dt)
    q = torch.nn.functional.normalize(torch.randn(n_q * 32, dim, generator=g, device=dev), dim=-1).to(dt)
    to = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=t)  # noqa: E731
    ds, dl = to(np.arange(n_q * n_c, dtype=np.int64) * d_len, torch.int64), to(np.full(n_q * n_c, d_len), torch.int32)
    qs, ql = to(np.arange(n_q) * 32, torch.int32), to(np.full(n_q, 32), torch.int32)
    cand = to(rng.permutation(n_q * n_c).reshape(n_q, n_c), torch.int32)
    clock = _clock_sampler()
    dev_ms, _ = timed(lambda: colbert.maxsim(q, qs, ql, d, ds, dl, cand=cand))
    nbytes = d.numel() * 2 + q.numel() * 2
    emit(leg="maxsim_256x50", maxsim_ms=round(dev_ms, 4), bytes=nbytes, achieved_tb_per_s=round(nbytes / dev_ms / 1e9, 3),
         fraction_of_8_tb_per_s=round(nbytes / dev_ms / 1e9 / 8.0, 3), sclk_mhz=clock(), dtype=args.dtype, queries=n_q, candidates=n_c,
         tokens_per_passage=d_len, dim=dim, repeat=args.repeat)
    del d, q

    # the cross-encoder of the same box for the same job (one caller, the coalescing front off: nobody to share a batch with)
    ce = HipSentenceTransformerRerank(model="BAAI/bge-reranker-v2-m3", top_n=10, device="cuda:0", coalesce=False,
                                      model_kwargs=dict(synthetic_seed=1, torch_dtype=args.dtype))
    ce_pairs = [(query, text(280)) for _ in range(args.candidates)]
    clock = _clock_sampler()
    dev_ms, wall_ms = timed(lambda: ce.predict(ce_pairs))
    emit(leg="cross_encoder", model="BAAI/bge-reranker-v2-m3 geometry (24 layers, 1024)", predict_event_ms=round(dev_ms, 3),
         predict_wall_ms=round(wall_ms, 3), pairs=args.candidates, tokens_per_pair=int(ce.stats["tokens"] / max(ce.stats["pairs"], 1)),
         sclk_mhz=clock(), dtype=args.dtype, repeat=args.repeat)


if __name__ == "__main__":
    main()
