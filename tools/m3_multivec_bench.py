"""Rerank with all three heads of BGE-M3: timing, for the record: BAAI/bge-m3's geometry (XLM-R large: 24
layers, 1024) with seeded weights, seeded lexical and multi-vector heads (1024 -> 1024, with a bias) and the hashing tokenizer, one
MI355X, HIP events, warm-up, median of ``--repeat``.  No gate.

    python tools/m3_multivec_bench.py [--repeat 20] [--dtype bfloat16] [--out profiles/m3_multivec_bench.jsonl]

One JSON line per leg, appended to ``--out``:
  lone_caller_stored   one query against 50 candidates of about 180 tokens that sit in the two stores: query encode + projection +
                       ``tt_lexical_score`` + ``tt_maxsim_wide`` + ``tt_m3_mix`` between one event pair, and the wall time of
                       ``postprocess_nodes`` (tokenise, encode, score, read back, sort)
  maxsim_wide_256x50   ``tt_maxsim_wide`` alone: 256 queries of 32 vectors x 50 candidates each of 180 vectors at dim 1024, every (query,
                       candidate) a different passage of a 12 800-passage store, so the bytes are HBM bytes: achieved bytes/s
                       against the 8 TB/s of the part -- beside ``tt_maxsim`` at dim 128 on the same shape (tools/colbert_bench.py's
                       leg, run here on the same box)
  ingest               ``M3MultiVectorEncoder.encode`` against ``M3Encoder.encode`` on the same 256 passages: the projection of every
                       token row is what the third head adds
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

    from tensor_truth_amd import colbert, lexical, multivec
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding
    from tensor_truth_amd.schema import NodeWithScore, TextNode

    out_path = args.out or os.path.join(os.path.dirname(here), "profiles", "m3_multivec_bench.jsonl")
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

    emb = HipHuggingFaceEmbedding(model_name="BAAI/bge-m3", device="cuda:0", model_kwargs=dict(synthetic_seed=3, torch_dtype=args.dtype))
    H = emb.config.hidden
    g = torch.Generator().manual_seed(11)
    sparse = (torch.randn(H, generator=g) * 0.05, -0.2)
    wide = (torch.randn(H, H, generator=g) * 0.03, torch.randn(H, generator=g) * 0.3)
    rr = multivec.HipM3AllRerank(model="BAAI/bge-m3", top_n=10, model_kwargs=dict(m3_weights=(0.4, 0.2, 0.4), embedder=emb,
                                                                                   m3_heads=(sparse, wide)))
    query = text(9)
    passages = [text(args.passage_words) for _ in range(args.candidates)]

    def nodes(prefix):
        return [NodeWithScore(node=TextNode(text=t, id_=f"{prefix}{i}"), score=0.0) for i, t in enumerate(passages)]

    rr.index_nodes(nodes("s"))
    ids = [f"s{i}" for i in range(args.candidates)]
    stored, stored_mv = rr.store.lookup(ids)[None], rr.vectors.lookup(ids)[None]
    base = dict(dtype=args.dtype, layers=emb.config.layers, hidden=H, dim=rr.encoder.dim, candidates=args.candidates,
                tokens_per_passage=int(rr.vectors.n_tokens / args.candidates), repeat=args.repeat)

    def encode_and_score():
        q_dense, q_lw, q_tv = rr.encoder.encode([query], is_query=True)
        lex, dense, _ = rr.store.score(q_lw, stored, dense=q_dense, hybrid_weights=(1.0, 1.0))
        return multivec.m3_mix(dense, lex, rr.vectors.score(q_tv, stored_mv, mean=True), rr.m3_weights)

    clock = _clock_sampler()
    dev_ms, _ = timed(encode_and_score)
    _, wall_ms = timed(lambda: rr.postprocess_nodes(nodes("s"), query_str=query))
    emit(leg="lone_caller_stored", encode_plus_three_scores_ms=round(dev_ms, 3), postprocess_nodes_wall_ms=round(wall_ms, 3),
         vector_store_bytes=rr.vectors.nbytes, lexical_store_bytes=rr.store.nbytes, sclk_mhz=clock(), **base)

    # ingest: the same 256 passages through the three-head encoder and through the two-head one
    batch = emb._tokenize([text(args.passage_words) for _ in range(256)], "")
    two = lexical.M3Encoder(emb, head=sparse)
    clock = _clock_sampler()
    all_ms, _ = timed(lambda: rr.encoder.encode(batch, is_query=False))
    two_ms, _ = timed(lambda: two.encode(batch, is_query=False))
    emit(leg="ingest", passages=len(batch), tokens=int(sum(len(s) for s in batch)), m3_multivector_encode_ms=round(all_ms, 3),
         m3_encode_ms=round(two_ms, 3), ratio=round(all_ms / two_ms, 3), sclk_mhz=clock(), dtype=args.dtype, repeat=args.repeat)
    del rr, emb, two
    torch.cuda.empty_cache()

    # MaxSim alone over HBM-resident vectors: 256 x 50 different passages, at dim 1024 (the wide kernel) and at dim 128 (tt_maxsim)
    n_q, n_c, d_len, q_len = 256, args.candidates, 180, 32
    dt = getattr(torch, args.dtype)
    to = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=t)  # noqa: E731
    ds, dl = to(np.arange(n_q * n_c, dtype=np.int64) * d_len, torch.int64), to(np.full(n_q * n_c, d_len), torch.int32)
    qs, ql = to(np.arange(n_q) * q_len, torch.int32), to(np.full(n_q, q_len), torch.int32)
    cand = to(rng.permutation(n_q * n_c).reshape(n_q, n_c), torch.int32)
    for dim, name, fn in ((1024, "maxsim_wide_256x50", lambda q, d: multivec.maxsim_wide(q, qs, ql, d, ds, dl, cand=cand, mean=True)),
                          (128, "maxsim_wide_256x50_dim128", lambda q, d: multivec.maxsim_wide(q, qs, ql, d, ds, dl, cand=cand, mean=True)),
                          (128, "maxsim_256x50_dim128", lambda q, d: colbert.maxsim(q, qs, ql, d, ds, dl, cand=cand))):
        gd = torch.Generator(device=dev).manual_seed(3)
        d = torch.empty(n_q * n_c * d_len, dim, dtype=dt, device=dev)
        for lo in range(0, d.shape[0], 1 << 18):            # (normalised in pieces: the fp32 image of 4.7 GB is not needed at once)
            part = torch.randn(min(1 << 18, d.shape[0] - lo), dim, generator=gd, device=dev)
            d[lo:lo + part.shape[0]] = torch.nn.functional.normalize(part, dim=-1).to(dt)
        q = torch.nn.functional.normalize(torch.randn(n_q * q_len, dim, generator=gd, device=dev), dim=-1).to(dt)
        clock = _clock_sampler()
        dev_ms, _ = timed(lambda: fn(q, d))
        nbytes = d.numel() * 2 + q.numel() * 2
        emit(leg=name, maxsim_ms=round(dev_ms, 4), bytes=nbytes, achieved_tb_per_s=round(nbytes / dev_ms / 1e9, 3),
             fraction_of_8_tb_per_s=round(nbytes / dev_ms / 1e9 / 8.0, 3), sclk_mhz=clock(), dtype=args.dtype, queries=n_q, candidates=n_c,
             tokens_per_passage=d_len, query_vectors=q_len, dim=dim, repeat=args.repeat)
        del d, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
