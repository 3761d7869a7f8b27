"""What the pre-norm families' shared prologue owns (csrc/prenorm.h: Qwen3, ModernBERT, T5, EmbeddingGemma): the workspace plan,
the two memsets and the carve.  A forward must not depend on what the scratch buffer held before it: every case runs once over a
buffer of 0xFF bytes (a NaN in bf16, fp16 and fp32) and once over zeros, on the same stream, and the two outputs must be the
same bits and finite -- on every row, the gap rows between the sequences and the unused tail rows included.  That is what zeros
sized for the wrong family, a lost ``ctx`` memset, a gate buffer carved where there is none or a buffer carved too narrow would
break; the fixture tests run on whatever the allocator hands out and would not see it.  Smallest geometry the kernels take: 128
wide, 2 layers, vocab 300; Qwen3 with 2 heads / 1 KV head of 64 and FFN 64 (its one-row-per-sequence tail too), ModernBERT with 2
heads, FFN 64, one full and one sliding layer, T5 with 2 heads, d_ff 128 and either MLP, EmbeddingGemma with 1 head / 1 KV head of
256, FFN 64 and one sliding layer."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
# (family, dtype): T5 and EmbeddingGemma compute in bf16 only
CASES = [(f, d) for f in ("qwen3", "modernbert") for d in DTYPES] + [(f, "bfloat16") for f in ("t5_relu", "t5_gated", "gemma")]
# 256 rows with gap rows between the sequences and a tail of unused rows; 64 rows: the skinny-GEMM route, buffers padded to 256 rows
BATCHES = {256: (1, 9, 130, 37), 64: (40, 3)}


def _model(family, dev, dt):
    from tensor_truth_amd import decoder, gemma, modernbert, t5

    small = dict(vocab_size=300, hidden=128, layers=2)
    kinds = ("full_attention", "sliding_attention")
    if family == "qwen3":
        cfg = dataclasses.replace(decoder.QWEN3_EMBEDDING_0_6B, **small, heads=2, kv_heads=1, head_dim=64, ffn=64)
        return cfg, decoder.DecoderWeights(cfg, decoder.synthetic_state(cfg, seed=11), dev, dtype=dt)
    if family == "modernbert":     # a window of +-8 tokens: narrower than the 130- and 37-token sequences
        cfg = dataclasses.replace(modernbert.MODERNBERT_BASE, **small, heads=2, ffn=64, pad_id=0, layer_types=kinds, local_attention=16)
        return cfg, modernbert.ModernBertWeights(cfg, modernbert.synthetic_state(cfg, seed=11), dev, dtype=dt)
    if family == "gemma":
        cfg = dataclasses.replace(gemma.EMBEDDINGGEMMA_300M, **small, heads=1, kv_heads=1, head_dim=256, ffn=64, layer_types=kinds,
                                  window=8)
        return cfg, gemma.GemmaWeights(cfg, gemma.synthetic_state(cfg, seed=11), dev, dtype=dt)
    cfg = dataclasses.replace(t5.T5_BASE, **small, heads=2, ffn=128, mlp_kind=1 if family == "t5_gated" else 0)
    return cfg, t5.T5Weights(cfg, t5.synthetic_state(cfg, seed=11, dense=0), dev, dtype=dt)


@pytest.mark.parametrize("n_rows", list(BATCHES))
@pytest.mark.parametrize("family,dtype", CASES)
def test_forward_does_not_depend_on_what_the_scratch_held(dev, built_lib, family, dtype, n_rows):
    from tensor_truth_amd import encoder
    from tensor_truth_amd.encoder import Encoder, pack_tokens, pooled_rows

    cfg, weights = _model(family, dev, DTYPES[dtype])
    enc = Encoder(weights)
    rng = np.random.default_rng(3)
    batch = pack_tokens([rng.integers(4, cfg.vocab_size, n).tolist() for n in BATCHES[n_rows]], cfg)
    assert batch.n_rows == n_rows
    w, n_seq = ctypes.byref(weights.struct), len(BATCHES[n_rows])
    need = getattr(enc.lib, enc.path.workspace)(w, batch.n_rows)
    assert need > 0
    runs = [(need, lambda: enc.forward_packed(batch)[0], (n_rows, cfg.hidden))]
    if family == "qwen3":          # the last layer for one row per sequence, on compact buffers carved from the same plan
        need_rows = getattr(enc.lib, enc.path.rows_workspace)(w, batch.n_rows, n_seq)
        assert need_rows == need
        runs.append((need_rows, lambda: enc.rows_hidden_packed(batch, pooled_rows(batch)), (64, cfg.hidden)))
    for nbytes, run, shape in runs:
        outs = []
        with torch.cuda.device(dev):
            for fill in (0xFF, 0x00):
                buf, _ = encoder._scratch.get(enc.path.scratch, dev, nbytes)     # the buffer the forward below gets: same key, same stream
                buf[: nbytes + 256].fill_(fill)
                outs.append(run().clone())
            torch.cuda.synchronize()
        assert outs[0].shape == shape
        assert torch.isfinite(outs[0].float()).all() and torch.isfinite(outs[1].float()).all()
        assert torch.equal(outs[0], outs[1])
