"""NomicBERT / Jina-v3 path timing: the published geometry with seeded weights, HIP events, warm-up, median
of repeats.

    python tools/ropebert_bench.py [--geometry nomic jina] [--sequences 64 256] [--length 512] [--repeat 9] [--dtype bfloat16]
        tokens/s of the full forward + mean pooling (each timed window is ``--inner`` forwards between one event pair), and the
        GEMM / attention / row-op split of one more instrumented forward (tt_prof_*).

One JSON line per measurement, with the shader clock sampled (amdsmi, read only) while it ran.
"""
import argparse
import ctypes
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", nargs="+", default=["nomic"], choices=("nomic", "jina"))
    ap.add_argument("--sequences", type=int, nargs="+", default=[64, 256])
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
    from modernbert_bench import _timed

    from tensor_truth_amd import ropebert as rb
    from tensor_truth_amd.encoder import Encoder, pack_token_matrix

    dev = torch.device("cuda", 0)
    dt = getattr(torch, args.dtype)
    rng = np.random.default_rng(1)
    for geo in args.geometry:
        cfg = rb.NOMIC_BASE if geo == "nomic" else rb.JINA_V3
        g = torch.Generator(device=dev).manual_seed(606)
        # the tensors of ropebert.synthetic_state, generated on the device
        shapes = {k: tuple(v.shape) for k, v in rb.synthetic_state(_one_layer_tiny_vocab(cfg), 0).items()}
        sd = {}
        for i in range(cfg.layers):
            for k, s in shapes.items():
                if k.startswith("layers.0."):
                    norm = "layernorm.weight" in k
                    sd[k.replace("layers.0.", f"layers.{i}.")] = (1.0 if norm else 0.0) + torch.randn(*s, generator=g, device=dev) * (0.1 if norm else 0.02)
        H = cfg.hidden
        sd.update({"embeddings.word_embeddings.weight": torch.randn(cfg.vocab_size, H, generator=g, device=dev) * 0.02,
                   "embeddings.token_type_embeddings.weight": torch.randn(cfg.type_vocab, H, generator=g, device=dev) * 0.02,
                   "embeddings.LayerNorm.weight": 1 + torch.randn(H, generator=g, device=dev) * 0.1,
                   "embeddings.LayerNorm.bias": torch.randn(H, generator=g, device=dev) * 0.05})
        enc = Encoder(rb.RopeBertWeights(cfg, sd, dev, dtype=dt))
        lib = enc.lib
        for n in args.sequences:
            batch = pack_token_matrix(rng.integers(0, cfg.vocab_size, (n, args.length)), cfg)

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
            print(json.dumps(dict(geometry=geo, dtype=args.dtype, layers=cfg.layers, sequences=n, length=args.length,
                                  tokens=batch.n_tokens, forward_ms_median=round(med, 3), forward_ms_min=round(lo, 3),
                                  forward_ms_max=round(hi, 3), tokens_per_s=round(batch.n_tokens / med * 1e3), sclk_mhz=clk, **split)),
                  flush=True)
        del enc, sd
        torch.cuda.empty_cache()


def _one_layer_tiny_vocab(cfg):
    import dataclasses

    return dataclasses.replace(cfg, vocab_size=8, layers=1)


if __name__ == "__main__":
    main()
