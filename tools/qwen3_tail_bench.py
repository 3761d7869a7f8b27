"""Decoder path timing: the 0.6B geometry with seeded weights, HIP events, warm-up, median of repeats.

    python tools/qwen3_tail_bench.py embed  [--root DIR] [--chunk 256 512] [--tokens 131072] [--repeat 7]
        tokens/s of ``Encoder.embed_packed(pooling="last")``.  ``--root``: the checkout whose package is measured (default: this
        one) -- run it on two checkouts alternately, in separate processes, to compare two commits on one box.
    python tools/qwen3_tail_bench.py rerank [--pairs 50 1024] [--length 292] [--repeat 7]
        pairs/s of ``Encoder.rerank_packed`` (the one-row-per-sequence tail + score head) against the full forward followed by the
        same score head over the gathered rows.

One JSON line per measurement, with the shader clock sampled (amdsmi, read only) while it ran.
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time


def _clock_sampler():
    samples, stop = [], threading.Event()
    try:
        import amdsmi

        amdsmi.amdsmi_init()
        h = amdsmi.amdsmi_get_processor_handles()[0]
    except Exception:  # noqa: BLE001
        return lambda: None

    def loop():
        while not stop.is_set():
            try:
                samples.append(amdsmi.amdsmi_get_clock_info(h, amdsmi.AmdSmiClkType.GFX).get("clk"))
            except Exception:  # noqa: BLE001
                return
            time.sleep(0.05)

    t = threading.Thread(target=loop, daemon=True)
    t.start()

    def finish():
        stop.set()
        t.join(timeout=2.0)
        c = sorted(x for x in samples if isinstance(x, (int, float)))
        return c[len(c) // 2] if c else None

    return finish


def _timed(fn, warmup, repeat):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    clock = _clock_sampler()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), clock()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("embed", "rerank"))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    ap.add_argument("--chunk", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--tokens", type=int, default=131072)
    ap.add_argument("--pairs", type=int, nargs="+", default=[50, 1024])
    ap.add_argument("--length", type=int, default=292)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--dtype", default="bfloat16", choices=("bfloat16", "float16"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import dataclasses

    import numpy as np
    import torch

    from tensor_truth_amd.decoder import QWEN3_EMBEDDING_0_6B, DecoderWeights
    from tensor_truth_amd.encoder import Encoder, pack_token_matrix

    dev = torch.device("cuda", 0)
    dt = getattr(torch, args.dtype)
    cfg = dataclasses.replace(QWEN3_EMBEDDING_0_6B, layers=args.layers, num_labels=1 if args.mode == "rerank" else 0)
    g = torch.Generator(device=dev).manual_seed(606)

    def rnd(*shape, std=0.02, mean=0.0):
        return mean + torch.randn(*shape, generator=g, device=dev) * std

    H, D, nq, nkv, F = cfg.hidden, cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.ffn
    sd = {"embed_tokens.weight": rnd(cfg.vocab_size, H), "norm.weight": rnd(H, std=0.1, mean=1.0)}
    for i in range(cfg.layers):
        p = f"layers.{i}."
        for n, shape in (("self_attn.q_proj", (nq * D, H)), ("self_attn.k_proj", (nkv * D, H)), ("self_attn.v_proj", (nkv * D, H)),
                         ("self_attn.o_proj", (H, nq * D)), ("mlp.gate_proj", (F, H)), ("mlp.up_proj", (F, H)), ("mlp.down_proj", (H, F))):
            sd[p + n + ".weight"] = rnd(*shape)
        for n, m in (("self_attn.q_norm", D), ("self_attn.k_norm", D), ("input_layernorm", H), ("post_attention_layernorm", H)):
            sd[p + n + ".weight"] = rnd(m, std=0.1, mean=1.0)
    if cfg.num_labels:
        sd["score.weight"] = rnd(1, H, std=0.15)
    enc = Encoder(DecoderWeights(cfg, sd, dev, dtype=dt))
    rng = np.random.default_rng(1)
    base = dict(mode=args.mode, label=args.label or os.path.basename(os.path.abspath(args.root)), dtype=args.dtype, layers=cfg.layers)
    if args.mode == "embed":
        for L in args.chunk:
            batch = pack_token_matrix(rng.integers(0, cfg.vocab_size, (args.tokens // L, L)), cfg)
            med, lo, hi, clk = _timed(lambda: enc.embed_packed(batch, pooling="last"), args.warmup, args.repeat)
            print(json.dumps(dict(base, chunk=L, tokens=batch.n_tokens, ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                  tokens_per_s=round(batch.n_tokens / med * 1e3), sclk_mhz=clk)), flush=True)
        return
    from tensor_truth_amd.encoder import pooled_rows

    lib = enc.lib
    for n in args.pairs:
        batch = pack_token_matrix(rng.integers(0, cfg.vocab_size, (n, args.length)), cfg)
        rows = torch.from_numpy(pooled_rows(batch).astype(np.int64)).to(dev)
        scores = torch.empty(n, dtype=torch.float32, device=dev)

        def full():
            hidden, _ = enc.forward_packed(batch)
            picked = hidden.index_select(0, rows)
            rc = getattr(lib, enc.path.score)(picked.data_ptr(), H, enc.w.score_w.data_ptr(), n, H, scores.data_ptr(), None,
                                              torch.cuda.current_stream(dev).cuda_stream)
            assert rc == 0
            return scores

        tail = enc.rerank_packed(batch)
        assert torch.equal(tail, full().clone()), "the tail and the full forward disagree"
        for what, fn in (("rows_forward+score", lambda: enc.rerank_packed(batch)), ("full_forward+score", full)):
            med, lo, hi, clk = _timed(fn, args.warmup, args.repeat)
            print(json.dumps(dict(base, what=what, pairs=n, length=args.length, ms_median=round(med, 3), ms_min=round(lo, 3),
                                  ms_max=round(hi, 3), pairs_per_s=round(n / med * 1e3), sclk_mhz=clk)), flush=True)


if __name__ == "__main__":
    main()
