"""GPU: the JinaBERT path (csrc/jinabert.hip, tensor_truth_amd/jinabert.py).

* ``tt_attention_alibi[_f16]`` against an fp64 softmax attention that adds -slope_h |query - key| to the scaled scores, on the
  element-rounded operands, in the three packings of tests/test_modernbert_gpu.py (``_pack``).  The bound per output element is
  ``test_modernbert_gpu._window_reference``'s derivation (its module docstring) with the bias' own two roundings -- the product
  slope * distance and its subtraction from the scaled score, 2 u (|s| + |bias|) -- added to the score term.  Lengths around every
  tile and key-block edge, six heads (the non-power-of-two slope rule), one 1100-token sequence (distances beyond 1024: nothing is
  clamped).  The defects ``signed`` (key - query without the absolute value) and ``nobias`` must lie outside the bound, on the fp64
  references themselves and for the kernel.  Rows of no sequence stay zero, and a sequence's rows are the same bits in all three
  packings (the policy counts its key blocks from the sequence's first row).
* The fixture checkpoint (tests/golden/make_jinabert_golden.py) through ``HipHuggingFaceEmbedding`` in bf16 and fp16: hidden
  states within 2 e_<type> of the fp64 states for every length (1 ... 700 tokens), e_<type> the reference torch model's own error in
  that type on the CPU, read from the fixture (the factor 2 is DESIGN.md 4.8's for a second 16-bit implementation); every defect
  reference outside that bound; pooled embeddings with cos >= 0.999 against fp64.
* Packing independence of the forward (``torch.equal``): alone, in a tight batch, in an aligned batch.
* The published small geometry with one 8192-token and one 3-token sequence in the same batch.
* Arguments refused before a launch.
Every figure is printed before it is asserted.
"""
import ctypes
import dataclasses
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "jinabert_l2")
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
KEY = {"bfloat16": "bf16", "float16": "fp16"}
LENGTHS = [1, 9, 17, 92, 130, 300, 700]
FACTOR = 2.0
HEADS = 6
ATT_LENS = [1, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 129, 257, 300, 1100]
LOG2E = math.log2(math.e)


# ---- tt_attention_alibi against fp64 ------------------------------------------------------------------------------------------------
def _alibi_reference(q, k, v, lens, heads, slopes, eps=None, defect=None):
    """fp64 attention of (q, k, v) [sum(lens)][H], the sequences' rows in order, per sequence and head:
    softmax(q.k / 8 - slope_h |i - j|) v -> (O, bound); bound None without eps.  ``defect`` "signed": slope_h (j - i) without the
    absolute value; "nobias": no bias."""
    from test_modernbert_gpu import LAM, U

    dh, scale = 64, 0.125
    outs, bounds, s0 = [], [], 0
    sl = torch.tensor(slopes, dtype=torch.float64, device=q.device)[:, None, None]
    for n in lens:
        Q, K, V = (x[s0:s0 + n].double().view(n, heads, dh).transpose(0, 1) for x in (q, k, v))
        s0 += n
        i = torch.arange(n, device=q.device, dtype=torch.float64)
        dist = i[None, :] - i[:, None]                                  # key - query
        B = -sl * (dist if defect == "signed" else dist.abs())[None]
        if defect == "nobias":
            B = torch.zeros_like(B)
        S0 = (Q @ K.transpose(1, 2)) * scale
        S = S0 + B
        P = torch.softmax(S, dim=-1)
        O = P @ V
        outs.append(O.transpose(0, 1).reshape(n, heads * dh))
        if eps is None:
            continue
        Sa = S.abs()
        dS = (LAM * U * math.sqrt(dh) * (Q.abs() @ K.abs().transpose(1, 2)) * scale + 2 * U * (Sa + Sa.amax(-1, keepdim=True))
              + 2 * U * (S0.abs() + B.abs()))                           # the bias' product and its subtraction
        dS = dS * (1.0 + dS.amax())                                     # (second order)
        PW, Oa, Vabs = P * dS, O.abs(), V.abs()
        PV = P @ Vabs
        V2 = V.pow(2).sum(1, keepdim=True).sqrt()                       # sqrt(sum_j v_jd^2): every key of the sequence is live
        l_inv = torch.exp(S.amax(-1, keepdim=True) - torch.logsumexp(S, -1, keepdim=True))
        b = (PW @ Vabs + Oa * PW.sum(-1, keepdim=True) + eps["p"] * (PV + Oa) + LAM * eps["p_abs"] * V2 * l_inv
             + LAM * U * math.sqrt(n) * (PV + Oa) + eps["out"] * Oa + eps["out_abs"])
        bounds.append(b.transpose(0, 1).reshape(n, heads * dh))
    return torch.cat(outs), (torch.cat(bounds) if eps is not None else None)


@functools.lru_cache(maxsize=None)
def _attention_case(dt):
    """The operands (rows of the sequences in order, rounded to ``dt``), the fp64 reference, its bound and the two defect
    references: computed once per element type, shared by the three packings."""
    from test_modernbert_gpu import EPS

    from tensor_truth_amd.jinabert import alibi_slopes

    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(23)
    n, H = sum(ATT_LENS), HEADS * 64
    q, k, v = (torch.randn(n, H, generator=g, device=dev) * s for s in (1.5, 1.5, 1.0))
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    slopes = alibi_slopes(HEADS)
    want, bound = _alibi_reference(q, k, v, ATT_LENS, HEADS, slopes, EPS[dt])
    others = {d: _alibi_reference(q, k, v, ATT_LENS, HEADS, slopes, defect=d)[0] for d in ("signed", "nobias")}
    return q, k, v, slopes, want, bound, others


def _run_alibi(dev, dt, q, k, v, slopes, mode):
    from test_modernbert_gpu import _lib_and_stream, _pack, _sfx, _v8

    _lib, lib, st = _lib_and_stream(dev)
    H = HEADS * 64
    starts, T = _pack(ATT_LENS, mode)
    live = torch.zeros(T, dtype=torch.bool, device=dev)
    for s, n in zip(starts, ATT_LENS):
        live[s:s + n] = True
    # rows of no sequence hold other finite values: masked keys, never read into a result
    g = torch.Generator(device=dev).manual_seed(5)
    qkv = (torch.randn(T, 3 * H, generator=g, device=dev) * 1.5).to(dt)
    qkv[live] = torch.cat([q, k, v], dim=1)
    vt = _v8(qkv[:, 2 * H:].contiguous())
    out = torch.zeros(T, H, dtype=dt, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(ATT_LENS, dtype=torch.int32, device=dev)
    s2 = torch.tensor([s * LOG2E for s in slopes], dtype=torch.float64).to(torch.float32).to(dev)
    rc = getattr(lib, "tt_attention_alibi" + _sfx(dt))(qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, ss.data_ptr(),
                                                     sl.data_ptr(), len(ATT_LENS), T, HEADS, 64, max(ATT_LENS), s2.data_ptr(), st)
    _lib.check(rc, "tt_attention_alibi")
    torch.cuda.synchronize()
    assert (out[~live].view(torch.int16) == 0).all()          # rows of no sequence are not written
    return out[live], starts


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_alibi_attention_matches_fp64(dev, built_lib, dt):
    from test_modernbert_gpu import _ratio

    q, k, v, slopes, want, bound, others = _attention_case(dt)
    assert max(ATT_LENS) - 1 > 1024 and len(slopes) == HEADS and slopes[4] == 0.5      # not a geometric series in head order
    # teeth, on the fp64 references themselves: the defects are more than two bounds away
    for name, other in others.items():
        gap = _ratio((other - want).abs(), bound)
        print(f"\n{dt}: fp64 reference '{name}' lies {gap:.3g} bounds from the ALiBi reference")
        assert gap > 2.0
    got = {}
    for mode in ("alt", "tight", "aligned"):
        rows, starts = _run_alibi(dev, dt, q, k, v, slopes, mode)
        assert torch.isfinite(rows.float()).all()
        err = (rows.double() - want).abs()
        ratio = _ratio(err, bound)
        print(f"alibi {mode} {dt}: max error / bound = {ratio:.3f} (max abs error {err.max().item():.3g}); starts mod 8 "
              f"{sorted({s % 8 for s in starts})}")
        assert ratio <= 1.0, f"alibi {mode} {dt}: error {ratio:.3g} x its bound"
        for name, other in others.items():
            assert _ratio((rows.double() - other).abs(), bound) > 1.0, name
        got[mode] = rows
    # the key blocks are counted from the sequence's first row: the same bits on and off the 8-row grid
    assert torch.equal(got["tight"], got["aligned"]) and torch.equal(got["alt"], got["aligned"])


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_zero_slopes_give_the_unwindowed_tile(dev, built_lib, dt):
    """All-zero slopes subtract 0.0f * distance: on the 8-row grid (where both tiles walk the same key blocks) the bits of
    ``tt_attention_window`` without a window."""
    from test_modernbert_gpu import _lib_and_stream, _pack, _sfx, _v8

    q, k, v, _, _, _, _ = _attention_case(dt)
    rows, starts = _run_alibi(dev, dt, q, k, v, [0.0] * HEADS, "aligned")
    _lib, lib, st = _lib_and_stream(dev)
    H = HEADS * 64
    _, T = _pack(ATT_LENS, "aligned")
    qkv = torch.zeros(T, 3 * H, dtype=dt, device=dev)
    live = torch.zeros(T, dtype=torch.bool, device=dev)
    for s, n in zip(starts, ATT_LENS):
        live[s:s + n] = True
    qkv[live] = torch.cat([q, k, v], dim=1)
    vt = _v8(qkv[:, 2 * H:].contiguous())
    out = torch.zeros(T, H, dtype=dt, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(ATT_LENS, dtype=torch.int32, device=dev)
    rc = getattr(lib, "tt_attention_window" + _sfx(dt))(qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, ss.data_ptr(),
                                                      sl.data_ptr(), len(ATT_LENS), T, HEADS, 64, max(ATT_LENS), -1, st)
    _lib.check(rc, "tt_attention_window")
    torch.cuda.synchronize()
    assert torch.equal(out[live], rows)


# ---- the fixture checkpoint -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    name = "jinabert_l2"
    z = np.load(os.path.join(GOLDEN, f"{name}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seqs = [z["ids"][f:f + n].tolist() for f, n in zip(first, lens)]
    hidden = {}
    for fn in (f"{name}_hidden.npz", f"{name}_hidden_700.npz"):
        zh = np.load(os.path.join(GOLDEN, fn))
        hidden.update({int(k.split("_")[1]): zh[k].astype(np.float64) for k in zh.files})
    assert sorted(hidden) == list(range(len(seqs))) and all(hidden[i].shape == (n, 384) for i, n in enumerate(lens))
    defects = {}
    for dn in z["defects"].tolist():
        zd = np.load(os.path.join(GOLDEN, f"{name}_defect_{dn}.npz"))
        defects[dn] = [zd[f"{dn}_{k}"].astype(np.float64) for k in range(len(z["defect_idx"]))]
    return seqs, {k: z[k] for k in z.files}, hidden, defects


def _embedder(dtype, **kw):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    return HipHuggingFaceEmbedding(FIXTURE, device="cuda", model_kwargs={"torch_dtype": dtype}, **kw)


def _hidden_of(enc, batch):
    hidden, _ = enc.forward_packed(batch)
    torch.cuda.synchronize()
    return hidden


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_fixture_through_the_embedder(dev, built_lib, dtype):
    from tensor_truth_amd.encoder import pack_tokens
    from tensor_truth_amd.jinabert import JinaBertWeights

    seqs, z, want, defects = _fixture()
    assert [len(s) for s in seqs] == LENGTHS
    e_ref = float(z[f"e_{KEY[dtype]}"])
    assert 1e-4 < e_ref < 0.5
    bound = FACTOR * e_ref
    emb = _embedder(dtype)
    assert emb.config.arch == "jina_bert" and emb.pooling == "mean" and isinstance(emb._model, JinaBertWeights)
    assert emb.max_length == 8192 and (emb.query_instruction, emb.text_instruction) == ("", "")
    batch = pack_tokens(seqs, emb.config)
    assert int(batch.pos[0]) == 0 and batch.max_len == 700 and batch.types is None
    hidden = _hidden_of(emb._encoder, batch).double().cpu().numpy()
    got = [hidden[s:s + n] for s, n in zip(batch.seq_start, batch.seq_len)]
    assert all(np.isfinite(g).all() for g in got)
    errs = [float(np.abs(g - want[i]).max()) for i, g in enumerate(got)]
    print(f"\njinabert_l2 {dtype}: hidden states max |hip - fp64| per length {dict(zip(LENGTHS, np.round(errs, 5)))}, "
          f"e_ref = {e_ref:.5f}, ratio = {max(errs) / e_ref:.3f}, bound = {bound:.5f}")
    assert max(errs) <= bound, f"jinabert_l2 {dtype}: {max(errs):.5f} > {FACTOR} x e_ref = {bound:.5f}"
    # the embedder surface: mean pooling + L2 normalisation
    vec = emb.embed_token_batches(seqs).double().cpu().numpy()
    cos = (vec * z["emb"]).sum(1) / np.linalg.norm(vec, axis=1)
    print(f"jinabert_l2 {dtype}: min cos to the fp64 pooled embeddings = {cos.min():.6f}")
    assert np.abs(np.linalg.norm(vec, axis=1) - 1).max() < 1e-3 and cos.min() >= 0.999
    # every defect reference used for this type lies outside the bound
    used = [d for d in z["defects"].tolist() if dtype == "float16" or d not in z["defects_fp16_only"].tolist()]
    assert set(z["defects"].tolist()) == {"nobias", "signed", "prescale", "pow2slopes", "headrev", "swapglu", "notype", "prenorm", "nobias_qkv"}
    assert set(used) == set(z["defects"].tolist())             # (the generator lists none as fp16-only)
    for defect in used:
        gap = max(float(np.abs(got[i] - defects[defect][k]).max()) for k, i in enumerate(z["defect_idx"].tolist()))
        print(f"jinabert_l2 {dtype}: defect {defect}: max |hip - defect| = {gap:.5f}")
        assert gap > bound, f"the defect reference '{defect}' lands inside the bound"
    # strings go through the checkpoint's tokenizer: [CLS] text [SEP]
    words = " ".join(f"w{t - 4}" for t in seqs[2][1:-1])
    assert emb._tokenizer.encode(words, None) == seqs[2]
    v = np.asarray(emb.get_text_embedding(words))
    assert v.shape == (384,) and np.isfinite(v).all() and abs(np.linalg.norm(v) - 1) < 1e-3
    assert np.abs(v - vec[2]).max() < 1e-6


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_rows_do_not_depend_on_packing(dev, built_lib, dtype):
    """Each sequence's rows: alone, in a tight batch (every sequence right behind its neighbour: starts off the 8-row grid) and in
    an aligned batch (what ``pack_tokens`` gives) -- the same bits."""
    from tensor_truth_amd.encoder import PackedBatch, _round_rows, pack_tokens

    seqs, _, _, _ = _fixture()
    emb = _embedder(dtype)
    enc, cfg = emb._encoder, emb.config
    aligned = pack_tokens(seqs, cfg)
    h_aligned = _hidden_of(enc, aligned)
    lens = np.asarray(LENGTHS, dtype=np.int32)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    assert sorted({int(s) % 8 for s in starts}) == [0, 1, 2, 3, 5, 7]
    n_rows = _round_rows(int(lens.sum()))
    ids, pos = np.full(n_rows, cfg.pad_id, dtype=np.int32), np.zeros(n_rows, dtype=np.int32)
    for s, seq in zip(starts, seqs):
        ids[s:s + len(seq)] = seq
        pos[s:s + len(seq)] = np.arange(len(seq))
    tight = PackedBatch(ids, pos, None, starts, lens, n_rows, int(lens.max()), int(lens.sum()))
    h_tight = _hidden_of(enc, tight)
    for i, seq in enumerate(seqs):
        n = len(seq)
        alone = _hidden_of(enc, pack_tokens([seq], cfg))[:n].clone()
        assert torch.isfinite(alone.float()).all()
        a0, t0 = int(aligned.seq_start[i]), int(starts[i])
        assert torch.equal(alone, h_aligned[a0:a0 + n]), (n, "alone / aligned differ")
        assert torch.equal(alone, h_tight[t0:t0 + n]), (n, "alone / tight differ")


@pytest.mark.default_precision
def test_a_dtype_must_be_named(dev, built_lib):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    with pytest.raises(NotImplementedError, match="JinaBERT.*bfloat16.*float16"):
        HipHuggingFaceEmbedding(FIXTURE, device="cuda")


def test_the_reranker_refuses_this_type(dev, built_lib):
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank

    with pytest.raises(ValueError, match="jina_bert checkpoints are served as embedders only"):
        HipSentenceTransformerRerank(model=FIXTURE, device="cuda", model_kwargs={"torch_dtype": "bfloat16"})


# ---- the published geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_small_geometry_runs_an_8192_token_sequence(dev, built_lib, dt):
    """jina-embeddings-v2-small-en's layers (512, 8 heads, 2048; two of its four) with seeded weights and a small vocabulary: one
    8192-token and one 3-token sequence in the same batch."""
    from tensor_truth_amd.encoder import Encoder, pack_tokens
    from tensor_truth_amd.jinabert import JINA_V2_SMALL, JinaBertWeights, synthetic_state

    cfg = dataclasses.replace(JINA_V2_SMALL, vocab_size=1000, layers=2)
    assert (cfg.hidden, cfg.heads, cfg.ffn, cfg.max_seq_len) == (512, 8, 2048, 8192)
    enc = Encoder(JinaBertWeights(cfg, synthetic_state(cfg, seed=5), dev, dtype=dt))
    g = np.random.default_rng(3)
    seqs = [g.integers(4, cfg.vocab_size, n).tolist() for n in (8192, 3)]
    batch = pack_tokens(seqs, cfg)
    assert batch.max_len == 8192 and batch.seq_start.tolist() == [0, 8192]
    hidden = _hidden_of(enc, batch)
    long_rows, short_rows = hidden[:8192], hidden[8192:8195]
    assert torch.isfinite(long_rows.float()).all() and torch.isfinite(short_rows.float()).all()
    assert long_rows.float().abs().mean() > 0.1
    alone = _hidden_of(enc, pack_tokens([seqs[1]], cfg))[:3]
    assert torch.equal(short_rows, alone)
    emb, _ = enc.embed_packed(batch, pooling="mean")
    assert torch.isfinite(emb).all() and torch.allclose(emb.norm(dim=1), torch.ones(2, device=dev), atol=1e-3)


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["", "_f16"])
def test_bad_arguments_refused_before_a_launch(dev, built_lib, sfx):
    from tensor_truth_amd import _lib
    from tensor_truth_amd.jinabert import _JbLayerW, _JbW

    lib, st = _lib.load_library(), torch.cuda.current_stream(dev).cuda_stream
    fwd, wsb, att = (getattr(lib, n + sfx) for n in ("tt_jinabert_forward", "tt_jinabert_workspace_bytes", "tt_attention_alibi"))
    layers = (_JbLayerW * 1)()

    def weights(**kw):
        a = dict(hidden=512, layers=1, heads=8, ffn=2048, vocab=1000, type_vocab=2, ln_eps=1e-12, word_emb=1, type_emb=1, emb_ln_g=1,
                 emb_ln_b=1, alibi_slope_log2=1)
        a.update(kw)
        return _JbW(layer=ctypes.cast(layers, ctypes.POINTER(_JbLayerW)), **a)

    def err():
        return lib.tt_last_error().decode()

    assert wsb(ctypes.byref(weights()), 256) > 0
    for kw, text in ((dict(hidden=200, heads=3), "hidden=200"), (dict(hidden=1152, heads=18), "hidden=1152"),
                     (dict(hidden=768, heads=24), "head_dim"), (dict(hidden=256, heads=8), "head_dim"), (dict(ffn=100), "ffn=100"),
                     (dict(ffn=192), "ffn=192")):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        rc = fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st)
        assert rc == -2 and text in err(), (kw, rc, err())
    for kw in (dict(word_emb=None), dict(type_emb=None), dict(alibi_slope_log2=None), dict(ln_eps=0.0)):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        assert fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st) == -1, kw
    w = weights(layers=0)
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    need = wsb(ctypes.byref(w), 256)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    rc = fwd(ctypes.byref(w), p, p, p, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "type_ids" in err()
    rc = fwd(ctypes.byref(w), p, None, None, p, p, 4, 256, 16, p, base, need, st)          # `pos` is part of the contract
    assert rc == -1 and "null pointer" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 0, 256, 16, p, base, need, st)
    assert rc == -1 and "n_seq" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 200, 16, p, base, need, st)
    assert rc == -1 and "n_rows" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, need - 1, st)         # a workspace one byte short
    assert rc != 0 and "workspace" in err()
    w = weights()                                                                          # a layer with a missing matrix
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, wsb(ctypes.byref(w), 256), st)
    assert rc == -1 and "null weight" in err()
    # the building block
    assert att(p, 1536, 0, 512, p, 4096, p, 512, p, p, 1, 256, 8, 32, 16, p, st) == -2 and "head_dim=32" in err()
    assert att(p, 1536, 0, 512, p, 4096, p, 512, p, p, 1, 256, 8, 64, 16, None, st) == -1 and "null pointer" in err()
    assert att(p, 1536, 0, 512, p, 4096, p, 512, p, p, 1, 256, 8, 64, 300, p, st) == -1 and "max_len" in err()
    assert att(p, 1000, 0, 512, p, 4096, p, 512, p, p, 1, 256, 8, 64, 16, p, st) == -1 and "ld=1000" in err()
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0                      # nothing was launched: the output buffer is untouched
