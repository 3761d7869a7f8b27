"""SPLADE timing, for the record: one MI355X, HIP events, warm-up, median of ``--repeat``, the shader clock
sampled (amdsmi, read only) while the windows ran.

    python tools/splade_bench.py [--repeat 7] [--sequences 1600] [--length 292] [--out profiles/splade_pool_bench.log]

One JSON line per leg, appended to ``--out``:
  pool_ingest / pool_query   ``tt_splade_pool`` (bf16, activation 1) on random operands at bert-base's head geometry (H 768, Vp 30592):
                             ``--sequences`` x ``--length`` tokens -- the benchmark's packed batch, 1600 x 292 = 467 200 -- and one
                             32-token sequence; 2 rows H Vp flops against the 2.5 PF bf16 MFMA peak
  unfused_ingest / _query    the unfused form on the same operands: ``torch.matmul`` into a bf16 logits buffer, the bias, ``amax`` per
                             sequence, relu and log1p -- in chunks of ``--chunk`` sequences so that the logits fit (the fused kernel
                             never writes them); ``ratio`` = unfused / fused time
  encode                     ``SpladeEncoder.encode`` on synthetic bert-base weights (``--passages`` passages of ``--length`` tokens, ids
                             in) in passages/s, beside the dense embedder's ``embed_token_batches`` rate on the same ids in the same run
"""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sequences", type=int, default=1600)
    ap.add_argument("--length", type=int, default=292)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--passages", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)

    import numpy as np
    import torch
    from modernbert_bench import _clock_sampler

    from tensor_truth_amd import splade
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    out_path = args.out or os.path.join(os.path.dirname(here), "profiles", "splade_pool_bench.log")
    dev = torch.device("cuda", 0)
    PEAK = 2.5e15
    H, V = 768, 30522
    Vp = (V + 127) // 128 * 128

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        clock = _clock_sampler()
        ms = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms), clock()

    gen = torch.Generator(device="cpu").manual_seed(11)
    E = (torch.randn(Vp, H, generator=gen) * 0.05).to(torch.bfloat16).to(dev)
    bias = (torch.randn(Vp, generator=gen) - 3.0).to(dev)
    for leg, n_seq, length in (("ingest", args.sequences, args.length), ("query", 1, 32)):
        rows = n_seq * length
        t = torch.randn(rows, H, generator=gen).to(torch.bfloat16).to(dev)
        starts = torch.arange(n_seq, dtype=torch.int32, device=dev) * length
        lens = torch.full((n_seq,), length, dtype=torch.int32, device=dev)
        out = torch.empty((n_seq, Vp), dtype=torch.float32, device=dev)
        flops = 2.0 * rows * H * Vp

        def fused():
            splade.splade_pool(t, E, bias, starts, lens, max_len=length, activation=1, out=out)

        chunk = min(args.chunk, n_seq)
        logits = torch.empty((chunk * length, Vp), dtype=torch.bfloat16, device=dev)
        ref = torch.empty_like(out)

        def unfused():
            for lo in range(0, n_seq, chunk):
                hi = min(lo + chunk, n_seq)
                lg = logits[: (hi - lo) * length]
                torch.matmul(t[lo * length:hi * length], E.T, out=lg)
                m = lg.view(hi - lo, length, Vp).amax(1).float() + bias
                ref[lo:hi] = torch.log1p(torch.relu(m))

        f_med, f_min, f_max, f_clk = timed(fused)
        u_med, u_min, u_max, u_clk = timed(unfused)
        # (the unfused form rounds every logit to bf16 before the maximum and adds the bias after: it differs by bf16's half ulp)
        diff = float((out - ref).abs().max())
        emit(leg=f"pool_{leg}", sequences=n_seq, length=length, H=H, Vp=Vp, ms_median=f_med, ms_min=f_min, ms_max=f_max,
             tflops=flops / f_med / 1e9, of_bf16_peak=flops / (f_med * 1e-3) / PEAK, sclk_mhz=f_clk, repeat=args.repeat)
        emit(leg=f"unfused_{leg}", sequences=n_seq, length=length, chunk_sequences=chunk, logits_bytes_per_chunk=logits.numel() * 2,
             ms_median=u_med, ms_min=u_min, ms_max=u_max, tflops=flops / u_med / 1e9, of_bf16_peak=flops / (u_med * 1e-3) / PEAK,
             ratio_unfused_over_fused=u_med / f_med, max_abs_difference=diff, sclk_mhz=u_clk, repeat=args.repeat)
        del t, out, ref, logits

    # passages per second: SpladeEncoder.encode beside the dense embedder, synthetic bert-base weights, the same token ids
    cfg = splade.SPLADE_BERT_BASE
    retr = splade.HipSpladeRetriever(model="synthetic/splade-bert-base", model_kwargs={"encoder_config": cfg, "synthetic_seed": 3})
    emb = HipHuggingFaceEmbedding(model_name="synthetic/bert-base", model_kwargs={"encoder_config": cfg, "synthetic_seed": 3,
                                                                                  "torch_dtype": "bfloat16"})
    rng = np.random.default_rng(9)
    seqs = [[101] + rng.integers(1000, cfg.vocab_size, args.length - 2).tolist() + [102] for _ in range(args.passages)]
    nnz = []

    def encode():
        nnz.append(retr.encoder.encode(seqs).nnz)

    s_med, s_min, s_max, s_clk = timed(encode)
    d_med, d_min, d_max, d_clk = timed(lambda: emb.embed_token_batches(seqs))
    emit(leg="encode", passages=args.passages, length=args.length, splade_ms_median=s_med, splade_passages_per_s=args.passages / s_med * 1e3,
         dense_ms_median=d_med, dense_passages_per_s=args.passages / d_med * 1e3, splade_over_dense_time=s_med / d_med,
         mean_terms_per_passage=float(np.mean(nnz[-1])), sclk_mhz=[s_clk, d_clk], repeat=args.repeat)


if __name__ == "__main__":
    main()
