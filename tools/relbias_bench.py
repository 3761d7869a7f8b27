"""GPU: what the relative-position bias costs the attention tile.  Times ``tt_attention_relbias`` against ``tt_attention_window``
(no window: w = n_rows) of the same library -- the same tile with the bias policy off -- on the same operands, per element type:

    python tools/relbias_bench.py [--seqs 64] [--len 384] [--heads 12] [--iters 200] [--rounds 7]

Each round times ``iters`` back-to-back launches of one kernel, then of the other, between device events (alternating, so that
clock drift and other tenants hit both); the report is the median round per kernel, the spread of the rounds and the ratio.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=64)
    ap.add_argument("--len", type=int, default=384)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    H, T = a.heads * 64, a.seqs * a.len
    assert a.len % 8 == 0 and T % 128 == 0
    g = torch.Generator(device=dev).manual_seed(1)
    starts = torch.arange(a.seqs, dtype=torch.int32, device=dev) * a.len
    lens = torch.full((a.seqs,), a.len, dtype=torch.int32, device=dev)
    table = (torch.randn(a.heads, 257, generator=g, device=dev) * 1.4426950408889634).contiguous()
    for name, dt, sfx in (("bf16", torch.bfloat16, ""), ("fp16", torch.float16, "_f16")):
        q, k, v = (torch.randn(T, H, generator=g, device=dev).to(dt) for _ in range(3))
        qkv = torch.cat([q, k, v], 1).contiguous()
        vt = v.reshape(T // 8, 8, H).permute(0, 2, 1).contiguous()
        out = torch.zeros(T, H, dtype=dt, device=dev)
        head = (qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, starts.data_ptr(), lens.data_ptr(), a.seqs, T,
                a.heads, 64, a.len)
        calls = {"window": lambda: getattr(lib, "tt_attention_window" + sfx)(*head, T, st),
                 "relbias": lambda: getattr(lib, "tt_attention_relbias" + sfx)(*head, table.data_ptr(), st)}
        times = {n: [] for n in calls}
        for n, f in calls.items():                       # warm-up: code objects loaded, clocks up
            for _ in range(20):
                _lib.check(f(), n)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for n, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f()
                e1.record()
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e3 / a.iters)     # microseconds per launch
        med = {n: statistics.median(t) for n, t in times.items()}
        print(json.dumps({"dtype": name, "seqs": a.seqs, "len": a.len, "heads": a.heads, "iters": a.iters, "rounds": a.rounds,
                          "window_us": round(med["window"], 2), "relbias_us": round(med["relbias"], 2),
                          "ratio": round(med["relbias"] / med["window"], 4),
                          "window_us_min_max": [round(min(times["window"]), 2), round(max(times["window"]), 2)],
                          "relbias_us_min_max": [round(min(times["relbias"]), 2), round(max(times["relbias"]), 2)]}))


if __name__ == "__main__":
    main()
