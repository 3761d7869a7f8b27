"""Metadata-filtered exact search at 10 M x 1024 bf16: tt_filter_rows + tt_scan_topk_rows against the unfiltered tt_scan_topk.

For a lone caller (1 query) and a batch (64 queries) at pass rates 0.1 % .. 100 %: the filter pass and the row-list scan timed
with device events (median of the repetitions), the listed rows' bytes over the scan time as a fraction of the 8 TB/s peak,
and the unfiltered scan beside it.  One JSON line per case, then a summary table.

    python tools/filtered_scan_bench.py [--rows 10000000] [--dim 1024] [--k 10] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensor_truth_amd  # noqa: E402,F401
from tensor_truth_amd import metadata_filter as mf  # noqa: E402
from tensor_truth_amd import scan as tscan  # noqa: E402

PEAK = 8.0e12
N_CODES = 100_000


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, d, k = args.rows, args.dim, args.k
    g = torch.Generator(device=dev).manual_seed(1)
    mat = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, 1 << 20):                       # (fp32 scratch a slice at a time)
        x = torch.randn((min(1 << 20, n - lo), d), generator=g, device=dev)
        mat[lo:lo + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
    codes = torch.randint(1, N_CODES + 1, (n,), generator=g, device=dev, dtype=torch.int32)
    results = []
    for nq in (1, 64):
        x = torch.randn((nq, d), generator=g, device=dev)
        q = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()
        for _ in range(3):
            tscan.scan_topk(mat, q, k)
        t_dense = timed(lambda: tscan.scan_topk(mat, q, k, check_overflow=False), args.reps)
        for rate in (0.001, 0.01, 0.1, 0.5, 1.0):
            allowed = np.zeros(N_CODES + 1, dtype=bool)
            allowed[1: 1 + int(round(rate * N_CODES))] = True
            bits = torch.from_numpy(mf.pack_bits(allowed).view(np.int32)).to(dev)
            comp = mf.CompiledFilter([codes], [bits], [len(allowed)], False, n)
            rows, offs = tscan.filter_rows(comp, n, dev)
            count = int(offs[-1])
            comp.bound = count
            for _ in range(3):
                tscan.scan_topk_rows(mat, q, k, rows, offs, count)
            t_filter = timed(lambda: tscan.filter_rows(comp, n, dev), args.reps)
            t_scan = timed(lambda: tscan.scan_topk_rows(mat, q, k, rows, offs, count, check_overflow=False), args.reps)
            s, i, flag = tscan.scan_topk_rows(mat, q, k, rows, offs, count, return_flag=True)
            row_bytes = count * d * 2
            r = {"queries": nq, "pass_rate": rate, "listed_rows": count, "k": k, "filter_ms": round(t_filter, 4),
                 "scan_ms": round(t_scan, 4), "total_ms": round(t_filter + t_scan, 4), "unfiltered_ms": round(t_dense, 4),
                 "listed_bytes_tb_s": round(row_bytes / (t_scan * 1e-3) / 1e12, 3),
                 "frac_of_peak": round(row_bytes / (t_scan * 1e-3) / PEAK, 3),
                 "scan_vs_unfiltered": round(t_scan / t_dense, 3), "overflow_flag": flag}
            print(json.dumps(r), flush=True)
            results.append(r)
    print(f"\n{n} x {d} bf16, k = {k}, median of {args.reps}")
    print(f"{'Q':>3} {'pass':>6} {'rows':>9} {'filter ms':>10} {'scan ms':>8} {'total ms':>9} {'TB/s':>6} {'of peak':>8} {'unfilt ms':>10}")
    for r in results:
        print(f"{r['queries']:>3} {r['pass_rate']:>6.3f} {r['listed_rows']:>9} {r['filter_ms']:>10.4f} {r['scan_ms']:>8.4f} "
              f"{r['total_ms']:>9.4f} {r['listed_bytes_tb_s']:>6.2f} {r['frac_of_peak']:>8.3f} {r['unfiltered_ms']:>10.4f}")


if __name__ == "__main__":
    main()
