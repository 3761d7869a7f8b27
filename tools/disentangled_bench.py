"""GPU: what DeBERTa's disentangled attention costs.  Two measurements, per element type:

  attention   ``tt_attention_disentangled`` (the launch that writes the two fp32 position score tables + the tile that reads them)
              against ``tt_attention_window`` (no window: the same tile with the bias policy off) on the same operands;
  rerank      pairs per second of a 12-layer base-geometry synthetic DeBERTa cross-encoder (mixedbread-ai/mxbai-rerank-base-v1's
              shape) next to the XLM-R base reranker's (BAAI/bge-reranker-base's shape), both on token pairs of one length.

    python tools/disentangled_bench.py [--seqs 50] [--len 292] [--heads 12] [--iters 50] [--rounds 7] [--skip-rerank]

Each round times ``iters`` back-to-back calls of one side, then of the other, between device events (alternating, so that clock
drift and other tenants hit both); the report is the median round per side, the spread of the rounds and the ratio.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(calls, iters, rounds, warm=5):
    """calls: name -> f().  -> name -> list of microseconds per call, one per round."""
    for f in calls.values():                            # warm-up: code objects loaded, clocks up
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in calls}
    for _ in range(rounds):
        for n, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / iters)
    return times


def attention(a, lib, _lib, dev):
    from tensor_truth_amd.deberta import build_dist_index

    st = torch.cuda.current_stream(dev).cuda_stream
    stride = (a.len + 7) // 8 * 8
    H, T = a.heads * 64, (a.seqs * stride + 255) // 256 * 256
    n_pos, max_pos = 512, 512
    g = torch.Generator(device=dev).manual_seed(1)
    starts = torch.arange(a.seqs, dtype=torch.int32, device=dev) * stride
    lens = torch.full((a.seqs,), a.len, dtype=torch.int32, device=dev)
    dist = build_dist_index(256, max_pos).to(dev)
    tb = (T * a.heads * n_pos * 4 + 255) // 256 * 256
    ws = torch.empty(2 * tb + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    for name, dt, sfx in (("bf16", torch.bfloat16, ""), ("fp16", torch.float16, "_f16")):
        q, k, v = (torch.randn(T, H, generator=g, device=dev).to(dt) for _ in range(3))
        pk, pq = (torch.randn(n_pos, H, generator=g, device=dev).to(dt).contiguous() for _ in range(2))
        qkv = torch.cat([q, k, v], 1).contiguous()
        vt = v.reshape(T // 8, 8, H).permute(0, 2, 1).contiguous()
        out = torch.zeros(T, H, dtype=dt, device=dev)
        head = (qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, starts.data_ptr(), lens.data_ptr(), a.seqs, T,
                a.heads, 64, a.len)
        calls = {"window": lambda: _lib.check(getattr(lib, "tt_attention_window" + sfx)(*head, T, st), "window"),
                 "disentangled": lambda: _lib.check(getattr(lib, "tt_attention_disentangled" + sfx)(
                     *head, pk.data_ptr(), pq.data_ptr(), n_pos, dist.data_ptr(), max_pos, base, 2 * tb, st), "disentangled")}
        t = timed(calls, a.iters, a.rounds)
        med = {n: statistics.median(x) for n, x in t.items()}
        print(json.dumps({"what": "attention", "dtype": name, "seqs": a.seqs, "len": a.len, "heads": a.heads, "rows": T,
                          "table_bytes": 2 * tb, "iters": a.iters, "rounds": a.rounds, "window_us": round(med["window"], 1),
                          "disentangled_us": round(med["disentangled"], 1), "ratio": round(med["disentangled"] / med["window"], 3),
                          "window_us_min_max": [round(min(t["window"]), 1), round(max(t["window"]), 1)],
                          "disentangled_us_min_max": [round(min(t["disentangled"]), 1), round(max(t["disentangled"]), 1)]}),
              flush=True)


def rerank(a, dev):
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank

    g = np.random.default_rng(3)
    for name, dtype in (("bf16", "bfloat16"), ("fp16", "float16")):
        sides = {}
        for label, model, first, last in (("deberta", "mixedbread-ai/mxbai-rerank-base-v1", 1, 2), ("xlmr", "BAAI/bge-reranker-base", 0, 2)):
            rr = HipSentenceTransformerRerank(model, top_n=5, device="cuda", coalesce=False,
                                              model_kwargs={"synthetic_seed": 1, "torch_dtype": dtype})
            ids = g.integers(4, 30000, (a.seqs, a.len)).astype(np.int32)
            ids[:, 0], ids[:, -1], ids[:, a.len // 4] = first, last, last
            pairs = [row for row in ids]
            sides[label] = (rr, lambda rr=rr, pairs=pairs: rr.score_token_pairs(pairs))
        t = timed({n: f for n, (_, f) in sides.items()}, max(2, a.iters // 10), a.rounds, warm=2)
        med = {n: statistics.median(x) for n, x in t.items()}
        print(json.dumps({"what": "rerank", "dtype": name, "pairs": a.seqs, "len": a.len, "layers": 12, "rounds": a.rounds,
                          "deberta_ms": round(med["deberta"] / 1e3, 2), "xlmr_ms": round(med["xlmr"] / 1e3, 2),
                          "deberta_pairs_per_s": round(a.seqs / med["deberta"] * 1e6, 1),
                          "xlmr_pairs_per_s": round(a.seqs / med["xlmr"] * 1e6, 1), "ratio": round(med["deberta"] / med["xlmr"], 3),
                          "deberta_ms_min_max": [round(min(t["deberta"]) / 1e3, 2), round(max(t["deberta"]) / 1e3, 2)],
                          "xlmr_ms_min_max": [round(min(t["xlmr"]) / 1e3, 2), round(max(t["xlmr"]) / 1e3, 2)]}), flush=True)
        del sides
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=50)
    ap.add_argument("--len", type=int, default=292)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--skip-rerank", action="store_true")
    a = ap.parse_args()
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    dev = torch.device("cuda:0")
    attention(a, lib, _lib, dev)
    if not a.skip_rerank:
        rerank(a, dev)


if __name__ == "__main__":
    main()
