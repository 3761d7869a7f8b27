"""EmbeddingGemma path timing: the 300m geometry with seeded weights in bf16, HIP events, warm-up, median
of repeats, and the split of one forward's kernel time between GEMMs, attention and row ops from the library's own per-kernel
events (tt_prof_*), taken in a run of its own after the timed ones.

    python tools/gemma_bench.py [--chunk 256 512] [--tokens 131072] [--repeat 7] [--warmup 2] [--layers 24]

One JSON line per chunk length, with the shader clock sampled (amdsmi, read only) while it ran.  attention_tflops counts the live
(query, key) pairs of every layer's mask: 4 * head_dim flops per pair and query head; attention_of_peak is that over the 2.5 PF
bf16 matrix peak.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from qwen3_tail_bench import _timed  # noqa: E402

PEAK_BF16 = 2.5e15
KERNELS = {"gemm": 4, "attention": 5, "rowops": 6}


def live_pairs(length: int, w: int) -> int:
    """(query, key) pairs with |q - k| <= w inside one sequence of ``length`` tokens"""
    return sum(min(length - 1, q + w) - max(0, q - w) + 1 for q in range(length))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--chunk", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--tokens", type=int, default=131072)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import dataclasses

    import numpy as np
    import torch

    from tensor_truth_amd.encoder import Encoder, pack_token_matrix
    from tensor_truth_amd.gemma import DENSE_NAMES, EMBEDDINGGEMMA_300M, GemmaWeights, default_layer_types, state_names

    dev = torch.device("cuda", 0)
    cfg = dataclasses.replace(EMBEDDINGGEMMA_300M, layers=args.layers, layer_types=default_layer_types(args.layers), vocab_size=32768)
    g = torch.Generator(device=dev).manual_seed(300)
    H, D, nq, nkv, F = cfg.hidden, cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.ffn
    shapes = {"embed_tokens": (cfg.vocab_size, H), "q_proj": (nq * D, H), "k_proj": (nkv * D, H), "v_proj": (nkv * D, H),
              "o_proj": (H, nq * D), "gate_proj": (F, H), "up_proj": (F, H), "down_proj": (H, F), "q_norm": (D,), "k_norm": (D,)}
    sd = {}
    for name in state_names(cfg):
        shape = shapes.get(name.split(".")[-2], (H,))
        sd[name] = torch.randn(*shape, generator=g, device=dev) * (0.02 if len(shape) == 2 else 0.1)
    sd[DENSE_NAMES[0]] = torch.randn(4 * H, H, generator=g, device=dev) * 0.02
    sd[DENSE_NAMES[1]] = torch.randn(H, 4 * H, generator=g, device=dev) * 0.02
    enc = Encoder(GemmaWeights(cfg, sd, dev))
    lib = enc.lib
    rng = np.random.default_rng(1)
    for L in args.chunk:
        batch = pack_token_matrix(rng.integers(0, cfg.vocab_size, (args.tokens // L, L)), cfg)
        med, lo, hi, clk = _timed(lambda: enc.embed_packed(batch, pooling="mean"), args.warmup, args.repeat)
        lib.tt_prof_enable(1)
        enc.embed_packed(batch, pooling="mean")
        torch.cuda.synchronize()
        split = {}
        for name, which in KERNELS.items():
            ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
            lib.tt_prof_read(which, ctypes.byref(ms), ctypes.byref(n))
            split[name] = (ms.value, n.value)
        lib.tt_prof_enable(0)
        n_seq = args.tokens // L
        pairs = sum(live_pairs(L, cfg.window if t == "sliding_attention" else L) for t in cfg.layer_types) * n_seq
        att_flops = 4.0 * D * nq * pairs
        att_ms = split["attention"][0]
        total = sum(v[0] for v in split.values())
        print(json.dumps(dict(
            model="embeddinggemma-300m geometry", dtype="bfloat16", layers=cfg.layers, chunk=L, tokens=batch.n_tokens,
            ms_median=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), tokens_per_s=round(batch.n_tokens / med * 1e3),
            sclk_mhz=clk, kernel_ms={k: round(v[0], 3) for k, v in split.items()}, launches={k: v[1] for k, v in split.items()},
            kernel_share={k: round(v[0] / total, 3) for k, v in split.items()} if total else None,
            attention_tflops=round(att_flops / att_ms / 1e9, 1) if att_ms else None,
            attention_of_peak=round(att_flops / (att_ms * 1e-3) / PEAK_BF16, 4) if att_ms else None)), flush=True)


if __name__ == "__main__":
    main()
