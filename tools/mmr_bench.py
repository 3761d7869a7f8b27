"""MMR timing, for the record: the scan's candidates diversified by ``tt_mmr_select`` against what the library
could do before for the same question, one MI355X, 1 M x 1024 bf16 rows (2 GB: HBM bytes, not Infinity Cache bytes).

    python tools/mmr_bench.py [--rows 1000000] [--repeat 20] [--warmup 3] [--log profiles/mmr_bench.log]

At every point (n_q, P, k) three things are timed with the same procedure (warm-up, one HIP event pair per repetition, median and
min .. max over ``--repeat``), alternating, with the shader clock sampled (amdsmi, read only) while the windows ran:
  scan      ``scan.scan_topk`` for the P best rows per query (no overflow read-back: the flag stays on the device on every side)
  mmr       that scan, then ``scan.mmr_select`` on the same stream: the Gram tiles and the greedy selection, lambda 0.5, "max"
  baseline  that scan, then a ``torch`` gather of the candidates' rows, ``C @ C.T`` (bf16 ``bmm``), and the greedy loop as k
            iterations of ``torch`` calls on the device
The log states per point whether the expectation holds: mmr is faster than the baseline by more than the larger spread of the
two, and at (1, 40, 10) the selection adds less than the scan itself takes.
"""
import argparse
import json
import os
import statistics
import sys

POINTS = [(1, 40, 10), (1, 200, 50), (64, 200, 50), (8, 1024, 256)]
LAMBDA = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)

    import torch
    from modernbert_bench import _clock_sampler

    from tensor_truth_amd import scan as tscan

    log_path = args.log or os.path.join(os.path.dirname(here), "profiles", "mmr_bench.log")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(11)
    corpus = torch.empty(args.rows, args.dim, dtype=torch.bfloat16, device=dev)
    step = 1 << 18
    for lo in range(0, args.rows, step):       # (in slices: the fp32 draw of the whole matrix would triple the footprint)
        n = min(step, args.rows - lo)
        corpus[lo:lo + n] = torch.nn.functional.normalize(torch.randn(n, args.dim, generator=g, device=dev), dim=-1).to(torch.bfloat16)

    def timed(fns):
        """The legs alternate inside every repetition -> per leg (median, min, max) ms."""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ev = [[] for _ in fns]
        for _ in range(args.repeat):
            for j, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ev[j].append(a.elapsed_time(b))
        return [(statistics.median(e), min(e), max(e)) for e in ev]

    lines = [f"# tools/mmr_bench.py: {args.rows} x {args.dim} bf16 rows = {corpus.numel() * 2 / 1e9:.3f} GB; lambda {LAMBDA}, penalty max; "
             f"warm-up {args.warmup}, {args.repeat} repetitions, one HIP event pair each, the three legs alternating; ms are median "
             "[min .. max]; spread = the larger (max - min) of mmr and baseline",
             "# scan = scan_topk(P); mmr = scan + tt_mmr_select; baseline = scan + torch gather + bf16 bmm + k-step torch greedy loop; "
             "GFLOP = 2 * dim * P * P * n_q of the full similarity matrix"]
    for n_q, p, k in POINTS:
        q = torch.nn.functional.normalize(torch.randn(n_q, args.dim, generator=g, device=dev), dim=-1).to(torch.bfloat16).contiguous()
        ar = torch.arange(n_q, device=dev)

        def scan():
            return tscan.scan_topk(corpus, q, p, check_overflow=False)

        def mmr():
            s, i = scan()
            return tscan.mmr_select(corpus, i, s, k, LAMBDA)

        def baseline():
            s, i = scan()
            c = corpus[i.long().clamp_min(0)]                               # [n_q, P, dim]
            gm = torch.bmm(c, c.transpose(1, 2)).float()
            lr = LAMBDA * s
            pen = torch.zeros_like(s)
            taken = torch.zeros_like(s, dtype=torch.bool)
            picks = []
            for t in range(k):
                v = (lr - (1.0 - LAMBDA) * pen) if t else lr
                pick = v.masked_fill(taken, float("-inf")).argmax(dim=1)
                picks.append(pick)
                taken[ar, pick] = True
                row = gm[ar, pick]
                pen = row if t == 0 else torch.maximum(pen, row)
            return torch.stack(picks, 1)

        same = float((mmr()[3].long() == baseline()).float().mean())        # (the baseline's G is rounded to bf16: information only)
        clock = _clock_sampler()
        (s_med, s_min, s_max), (m_med, m_min, m_max), (b_med, b_min, b_max) = timed([scan, mmr, baseline])
        sclk = clock()
        spread = max(m_max - m_min, b_max - b_min)
        faster = b_med - m_med > spread
        verdict = f"mmr faster than the baseline by more than the spread: {'confirmed' if faster else 'REFUTED'}"
        added = m_med - s_med
        if (n_q, p, k) == POINTS[0]:
            verdict += f"; the selection adds less than the scan takes ({added:.3f} < {s_med:.3f} ms): {'confirmed' if added < s_med else 'REFUTED'}"
        gflop = 2.0 * args.dim * p * p * n_q / 1e9
        rec = dict(n_q=n_q, P=p, k=k, rows=args.rows, dim=args.dim, repeat=args.repeat, scan_ms=round(s_med, 3), scan_min_ms=round(s_min, 3),
                   scan_max_ms=round(s_max, 3), mmr_ms=round(m_med, 3), mmr_min_ms=round(m_min, 3), mmr_max_ms=round(m_max, 3),
                   baseline_ms=round(b_med, 3), baseline_min_ms=round(b_min, 3), baseline_max_ms=round(b_max, 3),
                   select_added_ms=round(added, 3), spread_ms=round(spread, 3), baseline_over_mmr=round(b_med / m_med, 2),
                   gram_gflop=round(gflop, 3), picks_equal_fraction=round(same, 3), sclk_mhz=sclk, expectation=verdict)
        lines.append(f"n_q {n_q:2d} P {p:4d} k {k:3d}: scan {s_med:7.3f} ms [{s_min:.3f} .. {s_max:.3f}] | mmr {m_med:7.3f} ms [{m_min:.3f} .. "
                     f"{m_max:.3f}] (+{added:.3f} ms for {gflop:.2f} GFLOP and {k} steps) | baseline {b_med:8.3f} ms [{b_min:.3f} .. {b_max:.3f}] | "
                     f"spread {spread:.3f} ms | baseline / mmr {rec['baseline_over_mmr']:.2f} | picks equal {same:.3f} | sclk {sclk} | {verdict}")
        lines.append(json.dumps(rec))
        print(lines[-2], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(log_path)), exist_ok=True)
    with open(log_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
