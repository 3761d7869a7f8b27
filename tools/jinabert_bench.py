"""JinaBERT path timing: jina-embeddings-v2-base-en's geometry (12 layers, 768 / 12 / 3072, GEGLU) with
seeded weights beside the nearest existing path, NomicBERT-base on ``tt_ropebert_forward`` (``mlp_kind`` 1: the same hidden size,
heads, FFN width and GEMM shapes) -- both encoders in one process, on the same packed batch, their timed windows ALTERNATING, HIP
events, warm-up, median of repeats.

    python tools/jinabert_bench.py [--sequences 64] [--length 512] [--repeat 9] [--dtype bfloat16]
        tokens/s of the full forward + mean pooling (each timed window is ``--inner`` forwards between one event pair), the GEMM /
        attention / row-op split of one more instrumented forward per encoder (tt_prof_*), and the ratio of the two medians.

One JSON line per encoder and one for the ratio, with the shader clock sampled (amdsmi, read only) while the windows ran.
"""
import argparse
import ctypes
import dataclasses
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[64])
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--dtype", default="bfloat16", choices=("bfloat16", "float16"))
    args = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)

    import numpy as np
    import torch
    from modernbert_bench import _clock_sampler

    from tensor_truth_amd import jinabert as jb
    from tensor_truth_amd import ropebert as rb
    from tensor_truth_amd.encoder import Encoder, pack_token_matrix

    dev = torch.device("cuda", 0)
    dt = getattr(torch, args.dtype)
    rng = np.random.default_rng(1)
    # the published depth and widths; the vocabulary cut to 1000 rows (a gather reads the rows it is asked for, whatever the table's height)
    jcfg = dataclasses.replace(jb.JINA_V2_BASE, vocab_size=1000)
    rcfg = dataclasses.replace(rb.NOMIC_BASE, vocab_size=1000)
    assert (jcfg.hidden, jcfg.heads, jcfg.ffn, jcfg.layers) == (rcfg.hidden, rcfg.heads, rcfg.ffn, rcfg.layers) and rcfg.mlp == "swiglu"
    encs = {"jinabert": Encoder(jb.JinaBertWeights(jcfg, jb.synthetic_state(jcfg, 606), dev, dtype=dt)),
            "ropebert": Encoder(rb.RopeBertWeights(rcfg, rb.synthetic_state(rcfg, 606), dev, dtype=dt))}
    cfgs = {"jinabert": jcfg, "ropebert": rcfg}
    for n in args.sequences:
        ids = rng.integers(4, 1000, (n, args.length))
        batches = {k: pack_token_matrix(ids, cfgs[k]) for k in encs}
        assert batches["jinabert"].n_rows == batches["ropebert"].n_rows

        def run(k):
            for _ in range(args.inner):
                encs[k].embed_packed(batches[k], pooling="mean")

        for _ in range(args.warmup):
            for k in encs:
                run(k)
        torch.cuda.synchronize()
        clock = _clock_sampler()
        ms = {k: [] for k in encs}
        for _ in range(args.repeat):
            for k in encs:                                   # alternate: both see the same clock and the same neighbours
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(k)
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b) / args.inner)
        clk = clock()
        med = {}
        for k, enc in encs.items():
            lib = enc.lib
            lib.tt_prof_enable(1)
            enc.embed_packed(batches[k], pooling="mean")
            torch.cuda.synchronize()
            split = {}
            for name, kid in (("gemm", 4), ("attention", 5), ("rowops", 6)):
                t, cnt = ctypes.c_double(0), ctypes.c_int(0)
                lib.tt_prof_read(kid, ctypes.byref(t), ctypes.byref(cnt))
                split[name + "_ms"], split[name + "_launches"] = round(t.value, 3), cnt.value
            lib.tt_prof_enable(0)
            med[k] = statistics.median(ms[k])
            tokens = batches[k].n_tokens
            print(json.dumps(dict(model=k, dtype=args.dtype, layers=cfgs[k].layers, hidden=cfgs[k].hidden, sequences=n, length=args.length,
                                  tokens=tokens, forward_ms_median=round(med[k], 3), forward_ms_min=round(min(ms[k]), 3),
                                  forward_ms_max=round(max(ms[k]), 3), tokens_per_s=round(tokens / med[k] * 1e3), sclk_mhz=clk, **split)),
                  flush=True)
        print(json.dumps(dict(sequences=n, length=args.length, dtype=args.dtype,
                              jinabert_over_ropebert=round(med["jinabert"] / med["ropebert"], 4))), flush=True)


if __name__ == "__main__":
    main()
