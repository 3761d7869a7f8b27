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
    ap.add_argument("--dtype", default="bfloat16", choices=("bfloat16", "float16"))
    ap.add_argument("--out", default=None)
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
