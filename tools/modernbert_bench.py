"""ModernBERT path timing: the base / large geometry with seeded weights, HIP events, warm-up, median of
repeats.

    python tools/modernbert_bench.py embed  [--geometry base large] [--chunk 256 512 8192] [--tokens 131072] [--repeat 7]
        tokens/s of the full forward + CLS pooling, the GEMM / attention / row-op split of one more instrumented forward
        (tt_prof_*), and the windowed kernel alone (``tt_attention_window`` on the forward's shapes) in TFLOP/s against its own
        flop count 4 D sum_q |window(q)| per (sequence, head).
    python tools/modernbert_bench.py rerank [--geometry base] [--pairs 50 1024] [--length 292] [--repeat 7]
        pairs/s of ``Encoder.rerank_packed`` (full forward + pooling head).

One JSON line per measurement, with the shader clock sampled (amdsmi, read only) while it ran.
"""
import argparse
import ctypes
import dataclasses
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


def window_flops(L, w, heads, n_seq, D=64):
    """4 D sum_q |window(q)| per (sequence, head): two products of D MACs per live (query, key) pair."""
    live = sum(min(L - 1, q + w) - max(0, q - w) + 1 for q in range(L))
    return 4.0 * D * live * heads * n_seq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("embed", "rerank"))
    ap.add_argument("--geometry", nargs="+", default=["base", "large"], choices=("base", "large"))
    ap.add_argument("--chunk", type=int, nargs="+", default=[256, 512, 8192])
    ap.add_argument("--tokens", type=int, default=131072)
    ap.add_argument("--pairs", type=int, nargs="+", default=[50, 1024])
    ap.add_argument("--length", type=int, default=292)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--dtype", default="bfloat16", choices=("bfloat16", "float16"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    import numpy as np
    import torch

    from tensor_truth_amd import modernbert as mb
    from tensor_truth_amd.encoder import Encoder, pack_token_matrix

    dev = torch.device("cuda", 0)
    dt = getattr(torch, args.dtype)
    rng = np.random.default_rng(1)
    for geo in args.geometry:
        cfg = dataclasses.replace(mb.MODERNBERT_BASE if geo == "base" else mb.MODERNBERT_LARGE, num_labels=1)
        g = torch.Generator(device=dev).manual_seed(606)

        def rnd(*shape, std=0.02, mean=0.0):
            return mean + torch.randn(*shape, generator=g, device=dev) * std

        # the tensors of modernbert.synthetic_state, generated on the device
        sd = {n: rnd(*s, std=0.1, mean=1.0) if n.endswith("norm.weight") else rnd(*s) for n, s in _shapes(cfg, mb).items()}
        enc = Encoder(mb.ModernBertWeights(cfg, sd, dev, dtype=dt))
        lib, H, nh, w = enc.lib, cfg.hidden, cfg.heads, cfg.local_attention // 2
        base = dict(mode=args.mode, geometry=geo, dtype=args.dtype, layers=cfg.layers,
                    sliding_layers=sum(t == "sliding_attention" for t in cfg.layer_types))
        if args.mode == "rerank":
            for n in args.pairs:
                batch = pack_token_matrix(rng.integers(0, cfg.vocab_size, (n, args.length)), cfg)
                med, lo, hi, clk = _timed(lambda: enc.rerank_packed(batch), args.warmup, args.repeat)
                print(json.dumps(dict(base, pairs=n, length=args.length, ms_median=round(med, 3), ms_min=round(lo, 3),
                                      ms_max=round(hi, 3), pairs_per_s=round(n / med * 1e3), sclk_mhz=clk)), flush=True)
            continue
        for L in args.chunk:
            batch = pack_token_matrix(rng.integers(0, cfg.vocab_size, (args.tokens // L, L)), cfg)
            med, lo, hi, clk = _timed(lambda: enc.embed_packed(batch, pooling="cls"), args.warmup, args.repeat)
            lib.tt_prof_enable(1)
            enc.embed_packed(batch, pooling="cls")
            torch.cuda.synchronize()
            split = {}
            for name, kid in (("gemm", 4), ("attention", 5), ("rowops", 6)):
                ms, cnt = ctypes.c_double(0), ctypes.c_int(0)
                lib.tt_prof_read(kid, ctypes.byref(ms), ctypes.byref(cnt))
                split[name + "_ms"], split[name + "_launches"] = round(ms.value, 3), cnt.value
            lib.tt_prof_enable(0)
            # the windowed kernel alone, on the forward's shapes
            T, n_seq = batch.n_rows, len(batch.seq_len)
            qkv = (torch.randn(T, 3 * H, generator=g, device=dev)).to(dt)
            vt = torch.randn(T // 8, H, 8, generator=g, device=dev).to(dt)
            out = torch.zeros(T, H, dtype=dt, device=dev)
            ss = torch.from_numpy(batch.seq_start).to(dev)
            sl = torch.from_numpy(batch.seq_len).to(dev)
            fn = getattr(lib, "tt_attention_window" + ("_f16" if dt == torch.float16 else ""))

            def window():
                rc = fn(qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, ss.data_ptr(), sl.data_ptr(), n_seq, T, nh,
                        64, L, w, torch.cuda.current_stream(dev).cuda_stream)
                assert rc == 0

            wmed, _, _, _ = _timed(window, args.warmup, args.repeat)
            print(json.dumps(dict(base, chunk=L, tokens=batch.n_tokens, ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                  tokens_per_s=round(batch.n_tokens / med * 1e3), sclk_mhz=clk, **split,
                                  window_ms=round(wmed, 4), window_tflops=round(window_flops(L, w, nh, n_seq) / wmed * 1e-9, 2))),
                  flush=True)
        del enc, sd
        torch.cuda.empty_cache()


def _shapes(cfg, mb):
    H, F = cfg.hidden, cfg.ffn
    per = {"attn.Wqkv.weight": (3 * H, H), "attn.Wo.weight": (H, H), "mlp.Wi.weight": (2 * F, H), "mlp.Wo.weight": (H, F),
           "attn_norm.weight": (H,), "mlp_norm.weight": (H,)}
    head = {"head.dense.weight": (H, H), "head.norm.weight": (H,), "classifier.weight": (1, H), "classifier.bias": (1,),
            "embeddings.tok_embeddings.weight": (cfg.vocab_size, H), "embeddings.norm.weight": (H,), "final_norm.weight": (H,)}
    out = {}
    for n in mb.state_names(cfg):
        out[n] = head[n] if n in head else per[n.split(".", 2)[2]]
    return out


if __name__ == "__main__":
    main()
