"""What the post-LN families' shared prologue owns (csrc/postln.h: MPNet, DeBERTa, JinaBERT, RoPE-BERT): the workspace plan, the
two memsets and the carve.  A forward must not depend on what the scratch buffer held before it: every case runs once over a
buffer of 0xFF bytes (a NaN in bf16, fp16 and fp32) and once over zeros, on the same stream, and the two outputs must be the
same bits and finite -- on every row, the gap rows between the sequences and the unused tail rows included.  That is what zeros
sized for the wrong family, a lost ``ctx`` memset or a buffer carved too narrow would break; the fixture tests run on whatever the
allocator hands out and would not see it.  Smallest geometry the kernels take: 128 wide, 2 heads, 2 layers, FFN 128 (64 for SwiGLU,
that family's own multiple)."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
FAMILIES = ["mpnet", "deberta", "jinabert", "ropebert_swiglu", "ropebert_gelu"]
# 256 rows with gap rows between the sequences and a tail of unused rows; 64 rows: the skinny-GEMM route, buffers padded to 256 rows
BATCHES = {256: (1, 9, 130, 37), 64: (40, 3)}


def _model(family, dev, dt):
    from tensor_truth_amd import deberta, jinabert, mpnet, ropebert

    small = dict(vocab_size=300, hidden=128, heads=2, layers=2, ffn=128)
    if family == "mpnet":
        mod, cls, cfg = mpnet, mpnet.MpnetWeights, dataclasses.replace(mpnet.MPNET_BASE, **small)
    elif family == "deberta":
        mod, cls, cfg = deberta, deberta.DebertaWeights, dataclasses.replace(deberta.MXBAI_RERANK_BASE, **small)
    elif family == "jinabert":
        mod, cls, cfg = jinabert, jinabert.JinaBertWeights, dataclasses.replace(jinabert.JINA_V2_SMALL, **small)
    elif family == "ropebert_swiglu":
        mod, cls, cfg = ropebert, ropebert.RopeBertWeights, dataclasses.replace(ropebert.NOMIC_BASE, **dict(small, ffn=64))
        assert cfg.mlp == "swiglu" and not cfg.biases
    else:
        mod, cls, cfg = ropebert, ropebert.RopeBertWeights, dataclasses.replace(ropebert.JINA_V3, **small)
        assert cfg.mlp == "gelu" and cfg.biases
    return cfg, cls(cfg, mod.synthetic_state(cfg, seed=11), dev, dtype=dt)


@pytest.mark.parametrize("n_rows", list(BATCHES))
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_does_not_depend_on_what_the_scratch_held(dev, built_lib, family, dtype, n_rows):
    from tensor_truth_amd import encoder
    from tensor_truth_amd.encoder import Encoder, pack_tokens

    cfg, weights = _model(family, dev, DTYPES[dtype])
    enc = Encoder(weights)
    rng = np.random.default_rng(3)
    batch = pack_tokens([rng.integers(4, cfg.vocab_size, n).tolist() for n in BATCHES[n_rows]], cfg)
    assert batch.n_rows == n_rows
    need = getattr(enc.lib, enc.path.workspace)(ctypes.byref(weights.struct), batch.n_rows)
    assert need > 0
    outs = []
    with torch.cuda.device(dev):
        for fill in (0xFF, 0x00):
            buf, _ = encoder._scratch.get(enc.path.scratch, dev, need)     # the buffer the forward below gets: same key, same stream
            buf[: need + 256].fill_(fill)
            hidden, _ = enc.forward_packed(batch)
            outs.append(hidden.clone())
        torch.cuda.synchronize()
    assert outs[0].shape == (n_rows, cfg.hidden)
    assert torch.isfinite(outs[0].float()).all() and torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])
