"""T5 encoder path timing: gtr-t5-base's geometry with seeded weights beside MPNet-base -- the same GEMM
shapes and the same attention kernel -- in one process, HIP events, warm-up, median of repeats.

    python tools/t5_bench.py [--model t5 mpnet] [--sequences 64 256] [--length 512] [--repeat 9]
        tokens/s of the full forward + the pooling tail (each timed window is ``--inner`` forwards between one event pair), and the
        GEMM / attention / row-op split of one more instrumented forward (tt_prof_*).  bf16.

One JSON line per measurement, with the shader clock sampled (amdsmi, read only) while it ran.
"""
import argparse
import ctypes
import dataclasses
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", nargs="+", default=["t5", "mpnet"], choices=("t5", "mpnet"))
    ap.add_argument("--sequences", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)

    import numpy as np
    import torch
    from modernbert_bench import _timed

    from tensor_truth_amd import mpnet, t5
    from tensor_truth_amd.encoder import Encoder, pack_token_matrix

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    for model in args.model:
        # the published depth and widths; the vocabulary cut to 1000 rows (a gather reads the rows it is asked for, whatever the table's height)
        if model == "t5":
            cfg = dataclasses.replace(t5.T5_BASE, vocab_size=1000)
            enc = Encoder(t5.T5Weights(cfg, t5.synthetic_state(cfg, 606), dev))
            first = 3
        else:
            cfg = dataclasses.replace(mpnet.MPNET_BASE, vocab_size=1000)
            enc = Encoder(mpnet.MpnetWeights(cfg, mpnet.synthetic_state(cfg, 606), dev))
            first = 4
        lib = enc.lib
        for n in args.sequences:
            length = min(args.length, cfg.max_seq_len)
            batch = pack_token_matrix(rng.integers(first, cfg.vocab_size, (n, length)), cfg)

            def run():
                for _ in range(args.inner):
                    enc.embed_packed(batch, pooling="mean")

            med, lo, hi, clk = _timed(run, args.warmup, args.repeat)
            med, lo, hi = med / args.inner, lo / args.inner, hi / args.inner
            lib.tt_prof_enable(1)
            enc.embed_packed(batch, pooling="mean")
            torch.cuda.synchronize()
            split = {}
            for name, kid in (("gemm", 4), ("attention", 5), ("rowops", 6)):
                ms, cnt = ctypes.c_double(0), ctypes.c_int(0)
                lib.tt_prof_read(kid, ctypes.byref(ms), ctypes.byref(cnt))
                split[name + "_ms"], split[name + "_launches"] = round(ms.value, 3), cnt.value
            lib.tt_prof_enable(0)
            print(json.dumps(dict(model=model, dtype="bfloat16", layers=cfg.layers, hidden=cfg.hidden, sequences=n, length=length,
                                  tokens=batch.n_tokens, forward_ms_median=round(med, 3), forward_ms_min=round(lo, 3),
                                  forward_ms_max=round(hi, 3), tokens_per_s=round(batch.n_tokens / med * 1e3), sclk_mhz=clk, **split)),
                  flush=True)
        del enc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
