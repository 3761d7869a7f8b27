"""GPU: the EmbeddingGemma path (csrc/gemma.hip, tensor_truth_amd/gemma.py), bf16.

* The fixture checkpoint (tests/golden/make_gemma_golden.py) against transformers.  The bound is the project's rule for a 16-bit
  path: twice the reference's own error in that type, read from the fixture at test time (``hidden_e_bf16`` for the hidden states,
  ``e_ref`` for the embeddings), plus the project's embedding bound cos >= 0.999.  The five defect references of the fixture (window
  off, one RoPE base, causal mask, norms without the 1 +, no Dense pair) lie outside that bound on every sequence the generator
  counted.  Every figure is printed before it is asserted.
* ``tt_attention_window_gqa`` (head_dim 256, 4 query heads over 2 KV heads) against an fp64 softmax attention with the exact mask on
  the bf16 operands, under the bound tests/test_modernbert_gpu.py applies to ``tt_attention_window`` (its module docstring: P and the
  output rounded to bf16, fp32 accumulation of scores, values and the row sum), with head_dim 256 and the score scale 1 / 16 in its
  terms.  A result computed with KV head h % kv_heads instead of h / group lies outside it.
* ``tt_gemma_qk_norm_rope`` at both RoPE bases and ``tt_gemma_add_norm`` (both fused residual ops are this kernel; and its plain
  form) against fp64, every element within ONE bf16 ulp of the fp64 value: ulp(v) = 2^(floor(log2 |v|) - 7).  No term for the
  evaluation's own error is added: the kernels evaluate in fp64, so what is left is the one rounding of the stored value (half an ulp)
  -- where h + norm(y) or a cos - b sin cancels, an fp32 evaluation misses this bound.
* Packing independence (``torch.equal``), the embedder surface and its refusals, the 300m geometry with seeded weights.
"""
import ctypes
import dataclasses
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAME = "gemma_mean_l5"
FIXTURE = os.path.join(GOLDEN, NAME)
FACTOR = 2.0
U = 2.0 ** -24
LAM = 4.0
EPS = dict(p=2.0 ** -8 + 2 * U, out=2.0 ** -8 + 2 * U)      # what the attention kernel rounds to bf16: P and the output
LENGTHS = [1, 2, 15, 16, 17, 33, 34, 129, 257, 600]
OFFSETS = [3, 5, 1, 7, 2, 6, 3, 5, 1, 4]                    # rows skipped in front of each sequence: starts off the 8-row grid


def _lib_and_stream(dev):
    from tensor_truth_amd import _lib

    return _lib, _lib.load_library(), torch.cuda.current_stream(dev).cuda_stream


def _v8(x):                                          # [T][F] -> the V8 layout [T/8][F][8]
    T, F = x.shape
    return x.reshape(T // 8, 8, F).permute(0, 2, 1).contiguous()


def _ratio(err, bound):
    assert torch.isfinite(bound).all() and (bound >= 0).all(), "the bound itself is not finite"
    return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()


def _ulp(v):
    """bf16 ulp at the magnitude of v (fp64): 2^(floor(log2 |v|) - 7); the smallest subnormal's spacing below the normal range."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v.device), e - 7)


# ---- windowed GQA attention against fp64 --------------------------------------------------------------------------------------------
def _attention_reference(q, k, v, starts, lens, heads, kv_heads, w, kv_of=None, with_bound=True):
    """fp64 attention per sequence and query head (KV head ``kv_of(h)``, default h // group), key j live for query i iff
    |i - j| <= w (w None: every key) -> (O, bound) over the sequences' rows in order."""
    D, scale, group = 256, 1.0 / 16.0, heads // kv_heads
    kv_idx = torch.tensor([(kv_of(h) if kv_of else h // group) for h in range(heads)], device=q.device)
    outs, bounds = [], []
    for s0, n in zip(starts, lens):
        Q = q[s0:s0 + n].double().view(n, heads, D).transpose(0, 1)
        K = k[s0:s0 + n].double().view(n, kv_heads, D).transpose(0, 1)[kv_idx]
        V = v[s0:s0 + n].double().view(n, kv_heads, D).transpose(0, 1)[kv_idx]
        i = torch.arange(n, device=q.device)
        live = torch.ones(n, n, dtype=torch.bool, device=q.device) if w is None else (i[:, None] - i[None, :]).abs() <= w
        S = ((Q @ K.transpose(1, 2)) * scale).masked_fill(~live, -math.inf)
        P = torch.softmax(S, dim=-1)
        O = P @ V
        outs.append(O.transpose(0, 1).reshape(n, heads * D))
        if not with_bound:
            continue
        Sa = torch.where(live, S.abs(), torch.zeros_like(S))
        dS = LAM * U * math.sqrt(D) * (Q.abs() @ K.abs().transpose(1, 2)) * scale + 2 * U * (Sa + Sa.amax(-1, keepdim=True))
        dS = torch.where(live, dS, torch.zeros_like(dS))
        dS = dS * (1.0 + dS.amax())                    # (second order)
        PW, Oa, Vabs = P * dS, O.abs(), V.abs()
        PV = P @ Vabs
        kn = live.sum(-1, keepdim=True).double()       # keys a query sums over
        b = PW @ Vabs + Oa * PW.sum(-1, keepdim=True) + EPS["p"] * (PV + Oa) + LAM * U * kn.sqrt() * (PV + Oa) + EPS["out"] * Oa
        bounds.append(b.transpose(0, 1).reshape(n, heads * D))
    return torch.cat(outs), (torch.cat(bounds) if with_bound else None)


@pytest.mark.parametrize("w", [16, None], ids=lambda w: f"w{w}")
def test_windowed_gqa_attention_matches_fp64(dev, built_lib, w):
    _lib, lib, st = _lib_and_stream(dev)
    heads, kv_heads, D = 4, 2, 256
    starts, row = [], 0
    for n, o in zip(LENGTHS, OFFSETS):
        row += o
        starts.append(row)
        row += n
    T = (row + 7) // 8 * 8 + 8
    assert any(s % 8 for s in starts)
    g = torch.Generator(device=dev).manual_seed(11 + (w or 0))
    q = (torch.randn(T, heads * D, generator=g, device=dev) * 1.5).bfloat16()
    k = (torch.randn(T, kv_heads * D, generator=g, device=dev) * 1.5).bfloat16()
    v = torch.randn(T, kv_heads * D, generator=g, device=dev).bfloat16()
    qkv = torch.cat([q, k, v], dim=1).contiguous()
    ld = (heads + 2 * kv_heads) * D
    vt = _v8(v)
    out = torch.zeros(T, heads * D, dtype=torch.bfloat16, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(LENGTHS, dtype=torch.int32, device=dev)
    rc = lib.tt_attention_window_gqa(qkv.data_ptr(), ld, 0, heads * D, vt.data_ptr(), 8 * kv_heads * D, out.data_ptr(), heads * D,
                                     ss.data_ptr(), sl.data_ptr(), len(LENGTHS), T, heads, kv_heads, D, max(LENGTHS),
                                     -1 if w is None else w, st)
    _lib.check(rc, "tt_attention_window_gqa")
    torch.cuda.synchronize()
    live = torch.zeros(T, dtype=torch.bool, device=dev)
    for s, n in zip(starts, LENGTHS):
        live[s:s + n] = True
    assert (out[~live].view(torch.int16) == 0).all()                     # rows of no sequence are not written
    got = torch.cat([out[s:s + n] for s, n in zip(starts, LENGTHS)]).double()
    want, bound = _attention_reference(q, k, v, starts, LENGTHS, heads, kv_heads, w)
    assert torch.isfinite(got).all()
    ratio = _ratio((got - want).abs(), bound)
    print(f"\nwindow {w}: max error / bound = {ratio:.3f} (max abs error {(got - want).abs().max().item():.3g})")
    assert ratio <= 1.0, f"window {w}: error {ratio:.3g} x its bound"
    # teeth: the wrong KV head, and (with a window) a window off by one row on either side, lie outside the bound
    wrong, _ = _attention_reference(q, k, v, starts, LENGTHS, heads, kv_heads, w, kv_of=lambda h: h % kv_heads, with_bound=False)
    assert _ratio((got - wrong).abs(), bound) > 1.0, "a result computed with KV head h % kv_heads lands inside the bound"
    for bad in ([] if w is None else [w - 1, w + 1]):
        other, _ = _attention_reference(q, k, v, starts, LENGTHS, heads, kv_heads, bad, with_bound=False)
        assert _ratio((got - other).abs(), bound) > 1.0, bad


# ---- row ops against fp64, one bf16 ulp ---------------------------------------------------------------------------------------------
def _norm64(x, w, eps):
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * (1.0 + w.double())


def _positions(rows, g, dev):
    pos = torch.randint(0, 2048, (rows,), generator=g, device=dev, dtype=torch.int32)
    pos[:4] = torch.tensor([0, 1, 2047, 1023], dtype=torch.int32, device=dev)
    return pos


@pytest.mark.parametrize("rows", [8, 264, 1000])
@pytest.mark.parametrize("theta", [1e6, 1e4])
def test_qk_norm_rope_within_one_ulp_of_fp64(dev, built_lib, theta, rows):
    _lib, lib, st = _lib_and_stream(dev)
    nq, nkv, D, eps = 3, 1, 256, 1e-6
    ld = (nq + 2 * nkv) * D
    g = torch.Generator(device=dev).manual_seed(int(theta) % 1000 + rows)
    x = (torch.randn(rows, ld, generator=g, device=dev) * 3).bfloat16()
    pos = _positions(rows, g, dev)
    gq, gk = (0.3 * torch.randn(D, generator=g, device=dev) for _ in range(2))
    y = x.clone()
    vt = torch.zeros(rows // 8, nkv * D, 8, dtype=torch.bfloat16, device=dev)
    rc = lib.tt_gemma_qk_norm_rope(y.data_ptr(), ld, pos.data_ptr(), gq.data_ptr(), gk.data_ptr(), rows, nq, nkv, D, eps, theta,
                                   vt.data_ptr(), 8 * nkv * D, st)
    _lib.check(rc, "tt_gemma_qk_norm_rope")
    torch.cuda.synchronize()
    assert torch.equal(vt, _v8(x[:, (nq + nkv) * D:].contiguous())) and torch.equal(y[:, (nq + nkv) * D:], x[:, (nq + nkv) * D:])

    def reference(base, shift=0, plus_one=True):
        half = D // 2
        inv = torch.tensor(base, dtype=torch.float64, device=dev) ** (-torch.arange(half, dtype=torch.float64, device=dev) * 2 / D)
        ang = (pos.double() + shift)[:, None] * inv[None, :]
        c, s = torch.cos(ang)[:, None], torch.sin(ang)[:, None]
        hd = x[:, :(nq + nkv) * D].double().view(rows, nq + nkv, D)
        gain = torch.stack([gq] * nq + [gk] * nkv).double()
        n = _norm64(hd, gain if plus_one else gain - 1.0, eps)
        a, b = n[..., :half], n[..., half:]
        return torch.cat([a * c - b * s, b * c + a * s], dim=-1).reshape(rows, (nq + nkv) * D)

    want = reference(theta)
    got = y[:, :(nq + nkv) * D].double()
    ratio = _ratio((got - want).abs(), _ulp(want))
    print(f"\nq/k norm + RoPE theta {theta:g} rows {rows}: max |error| = {ratio:.3f} ulp")
    assert ratio <= 1.0
    # teeth: the other base, positions off by one and norms without the 1 + lie outside it
    for bad in (reference(1.01e6 - theta), reference(theta, shift=1), reference(theta, plus_one=False)):
        assert _ratio((got - bad).abs(), _ulp(want)) > 4.0


@pytest.mark.parametrize("rows", [8, 264, 1000])
@pytest.mark.parametrize("H", [256, 768])
def test_fused_add_norm_within_one_ulp_of_fp64(dev, built_lib, H, rows):
    """h' = h + norm(y; wa) and x' = norm(h'; wb): the op behind the attention (post_attention / pre_feedforward norms) and the one
    behind the MLP (post_feedforward / the next input norm or the final norm) are this kernel with other weights -- two draws of
    them here -- and the plain x' = norm(h; wb) in front of the first layer is its form without y."""
    _lib, lib, st = _lib_and_stream(dev)
    eps = 1e-6
    g = torch.Generator(device=dev).manual_seed(H + rows)
    for draw in range(2):
        y = (torch.randn(rows, H, generator=g, device=dev) * (0.5 + 4 * draw)).bfloat16()
        h = (torch.randn(rows, H, generator=g, device=dev) * (3.0 - 2 * draw)).bfloat16()
        wa, wb = (0.3 * torch.randn(H, generator=g, device=dev) for _ in range(2))
        h_out, x_out, x_plain = (torch.zeros(rows, H, dtype=torch.bfloat16, device=dev) for _ in range(3))
        rc = lib.tt_gemma_add_norm(y.data_ptr(), h.data_ptr(), wa.data_ptr(), wb.data_ptr(), rows, H, eps, h_out.data_ptr(),
                                   x_out.data_ptr(), st)
        _lib.check(rc, "tt_gemma_add_norm")
        rc = lib.tt_gemma_add_norm(None, h.data_ptr(), None, wb.data_ptr(), rows, H, eps, None, x_plain.data_ptr(), st)
        _lib.check(rc, "tt_gemma_add_norm")
        torch.cuda.synchronize()
        want_h = h.double() + _norm64(y.double(), wa, eps)
        want_x = _norm64(want_h, wb, eps)
        want_plain = _norm64(h.double(), wb, eps)
        ratios = [_ratio((got.double() - want).abs(), _ulp(want)) for got, want in ((h_out, want_h), (x_out, want_x), (x_plain, want_plain))]
        print(f"\nadd + norm H {H} rows {rows} draw {draw}: max |error| in ulp: h' {ratios[0]:.3f}, x' {ratios[1]:.3f}, plain {ratios[2]:.3f}")
        assert max(ratios) <= 1.0
        # teeth: norms without the 1 +, and a second norm of y's sum without the residual, lie outside it
        bad_h = h.double() + _norm64(y.double(), wa - 1.0, eps)
        assert _ratio((h_out.double() - bad_h).abs(), _ulp(want_h)) > 4.0
        assert _ratio((x_out.double() - _norm64(want_h, wb - 1.0, eps)).abs(), _ulp(want_x)) > 4.0
        assert _ratio((x_out.double() - _norm64(_norm64(y.double(), wa, eps), wb, eps)).abs(), _ulp(want_x)) > 4.0


# ---- the fixture checkpoint against transformers ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(os.path.join(GOLDEN, f"{NAME}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return [z["ids"][f:f + n].tolist() for f, n in zip(first, lens)], z


@functools.lru_cache(maxsize=None)
def _fixture_encoder():
    from tensor_truth_amd import gemma, weights
    from tensor_truth_amd.encoder import Encoder

    with open(os.path.join(FIXTURE, "config.json")) as f:
        cfg = weights._config_from_hf(json.load(f))
    state = weights.load_state(FIXTURE)
    state.update(gemma.dense_modules(FIXTURE))
    return Encoder(gemma.GemmaWeights(cfg, state, torch.device("cuda:0")))


def _embed(enc, seqs):
    from tensor_truth_amd.encoder import pack_tokens

    emb, emb16 = enc.embed_packed(pack_tokens(seqs, enc.cfg), pooling="mean")
    torch.cuda.synchronize()
    return emb.clone(), emb16.clone()


@functools.lru_cache(maxsize=None)
def _ragged():
    """every fixture sequence in one packed batch -> (fp32 embeddings, their bf16 copies), computed once"""
    return _embed(_fixture_encoder(), _fixture()[0])


def test_hidden_states_match_transformers(dev, built_lib):
    """max |hidden_hip - hidden_fp32| <= 2 hidden_e_bf16 over the four stored sequences (17, 34, 129 and 600 tokens)."""
    from tensor_truth_amd.encoder import pack_tokens

    seqs, _ = _fixture()
    zh = np.load(os.path.join(GOLDEN, f"{NAME}_hidden.npz"))
    e_ref = float(zh["hidden_e_bf16"])
    assert 1e-3 < e_ref < 0.5
    enc = _fixture_encoder()
    idx = zh["hidden_idx"].tolist()
    assert [len(seqs[i]) for i in idx] == [17, 34, 129, 600]
    batch = pack_tokens([seqs[i] for i in idx], enc.cfg)
    hidden, _ = enc.forward_packed(batch)
    torch.cuda.synchronize()
    hidden = hidden.double().cpu().numpy()
    errs = [float(np.abs(hidden[s:s + n] - zh[f"hidden_{k}"]).max()) for k, (s, n) in enumerate(zip(batch.seq_start, batch.seq_len))]
    print(f"\nhidden states max |hip - fp32| per sequence = {[round(e, 5) for e in errs]}, e_ref = {e_ref:.5f}, "
          f"ratio = {max(errs) / e_ref:.3f}")
    assert max(errs) <= FACTOR * e_ref, f"{max(errs):.5f} > {FACTOR} x e_ref = {FACTOR * e_ref:.5f}"


def test_embeddings_match_transformers(dev, built_lib):
    """All 44 sequences in one packed batch: max |hip - emb_fp32| <= 2 e_ref, cos >= 0.999, unit norm; the bf16 copy is the fp32
    vector rounded."""
    _, z = _fixture()
    e_ref = float(z["e_ref"])
    assert 5e-4 < e_ref < 2e-2 and float(np.abs(z["emb_bf16"] - z["emb_fp32"]).max()) == pytest.approx(e_ref)
    emb, emb16 = _ragged()
    got = emb.double().cpu().numpy()
    err = np.abs(got - z["emb_fp32"]).max(1)
    cos = (got * z["emb_fp32"]).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(z["emb_fp32"], axis=1))
    print(f"\nembeddings: max |hip - fp32| = {err.max():.5f}, e_ref = {e_ref:.5f}, ratio = {err.max() / e_ref:.3f}; "
          f"min cos = {cos.min():.6f}")
    assert err.max() <= FACTOR * e_ref, f"{err.max():.5f} > {FACTOR} x e_ref = {FACTOR * e_ref:.5f}"
    assert cos.min() >= 0.999
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-5
    assert torch.equal(emb16, emb.bfloat16())


@pytest.mark.parametrize("defect", ["nowindow", "onetheta", "causal", "plainnorm", "nodense"])
def test_defect_references_lie_outside_the_bound(dev, built_lib, defect):
    _, z = _fixture()
    bound = FACTOR * float(z["e_ref"])
    counted = z[f"{defect}_counted"]
    assert counted.sum() >= 20
    got = _ragged()[0].double().cpu().numpy()
    gap = np.abs(got - z[f"emb_{defect}"]).max(1)[counted]
    print(f"\ndefect {defect}: min |hip - defect| over {int(counted.sum())} sequences = {gap.min():.5f}, bound = {bound:.5f}")
    assert gap.min() > bound, f"the defect reference '{defect}' lands inside the bound"


def test_embeddings_do_not_depend_on_packing(dev, built_lib):
    """A sequence embedded alone, in the ragged batch and at another position of the batch (two batch orders) has the same bits."""
    seqs, z = _fixture()
    enc = _fixture_encoder()
    lens = z["lens"].tolist()
    ragged = _ragged()
    order_a = list(reversed(range(len(seqs))))
    order_b = list(np.random.default_rng(5).permutation(len(seqs)))
    shuffled = [(o, _embed(enc, [seqs[i] for i in o])) for o in (order_a, order_b)]
    for n in (1, 17, 34, 129, 600):
        i = lens.index(n)
        alone = _embed(enc, [seqs[i]])
        for a, r in zip(alone, ragged):
            assert torch.equal(a[0], r[i]), (n, "alone / ragged differ")
        for o, res in shuffled:
            at = o.index(i)
            assert at != i
            for a, m in zip(alone, res):
                assert torch.equal(a[0], m[at]), (n, "alone / reordered differ")
    for o, res in shuffled:
        assert torch.equal(res[0][torch.tensor(np.argsort(o), device=dev)], ragged[0])


# ---- surface -------------------------------------------------------------------------------------------------------------------------
def test_embedder_surface(dev, built_lib):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    _, z = _fixture()
    bound = FACTOR * float(z["e_ref"])
    emb = HipHuggingFaceEmbedding(model_name=FIXTURE, device="cuda", model_kwargs={"torch_dtype": "bfloat16"})
    assert emb.pooling == "mean" and emb.config.arch == "gemma3_text" and emb.embed_dim == 256
    assert (emb.query_instruction, emb.text_instruction) == ("task: search result | query: ", "title: none | text: ")
    assert emb.max_length == 1024 and HipHuggingFaceEmbedding(FIXTURE, device="cuda", max_length=4096,
                                                              model_kwargs={"torch_dtype": "bfloat16"}).max_length == 1024
    texts = z["text"].tolist()
    docs = np.asarray(emb.get_text_embedding_batch(texts))
    err_d = np.abs(docs - z["text_document_emb"]).max()
    queries = np.asarray([emb.get_query_embedding(t) for t in texts])
    err_q = np.abs(queries - z["text_query_emb"]).max()
    print(f"\nstrings: max |hip - fp32| documents {err_d:.5f}, queries {err_q:.5f}, bound = {bound:.5f}")
    assert err_d <= bound and err_q <= bound
    assert np.abs(np.linalg.norm(docs, axis=1) - 1).max() < 1e-5
    # the two prompts give different vectors for the same text
    assert np.abs(docs - queries).max(1).min() > bound
    ids = emb._tokenizer.encode(emb.query_instruction + texts[0], None)
    assert ids[0] == 1 and ids[-1] == 2 and 3 not in ids


@pytest.mark.default_precision
@pytest.mark.parametrize("mk", [None, {"torch_dtype": "float32"}, {"torch_dtype": "float16"}], ids=["none", "float32", "float16"])
def test_other_precisions_are_refused(dev, built_lib, mk):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    with pytest.raises(NotImplementedError, match="bfloat16"):
        HipHuggingFaceEmbedding(model_name=FIXTURE, device="cuda", model_kwargs=mk)


def test_the_reranker_surface_refuses_an_embedder(dev, built_lib):
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank

    with pytest.raises(ValueError, match="has no classification head"):
        HipSentenceTransformerRerank(FIXTURE, device="cuda", model_kwargs={"torch_dtype": "bfloat16"})


# ---- the 300m geometry ---------------------------------------------------------------------------------------------------------------
def test_300m_geometry_with_seeded_weights(dev, built_lib):
    """google/embeddinggemma-300m's layers (24 x 768, 3 heads over 1 KV head of 256, 1152, window +-256, full attention every sixth)
    with seeded weights, a vocabulary cut to 2048 and the Dense pair 768 -> 3072 -> 768: 64 ragged sequences of up to 2048 tokens."""
    from tensor_truth_amd.encoder import Encoder
    from tensor_truth_amd.gemma import EMBEDDINGGEMMA_300M, GemmaWeights, _GemmaLayerW, _GemmaW, synthetic_state

    cfg = dataclasses.replace(EMBEDDINGGEMMA_300M, vocab_size=2048)
    weights = GemmaWeights(cfg, synthetic_state(cfg, seed=9), dev)
    assert weights.out_dim == 768 and weights.struct.dense1_out == 3072 and weights.struct.embed_scale == 27.75
    enc = Encoder(weights)
    g = np.random.default_rng(13)
    lens = [2048, 1, 2047, 257] + g.integers(2, 1200, 60).tolist()
    seqs = [g.integers(0, cfg.vocab_size, n).tolist() for n in lens]
    emb, emb16 = _embed(enc, seqs)
    assert emb.shape == (64, 768) and torch.isfinite(emb).all()
    assert torch.allclose(emb.norm(dim=1), torch.ones(64, device=dev), atol=1e-5)
    assert len({bytes(r) for r in emb.cpu().numpy().view(np.uint8)}) == 64  # 64 different vectors
    for i in (0, 1, 40):
        alone = _embed(enc, [seqs[i]])
        other = _embed(enc, [seqs[5], seqs[i], seqs[2]])
        assert torch.equal(alone[0][0], emb[i]) and torch.equal(alone[1][0], emb16[i]) and torch.equal(other[0][1], emb[i])
    # the workspace size the host asks for is accepted; a byte less, and a shape off the limits, are refused before any launch
    _lib, lib, st = _lib_and_stream(dev)
    w = ctypes.byref(weights.struct)
    need = lib.tt_gemma_workspace_bytes(w, 256)
    assert need > 0
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    rc = lib.tt_gemma_forward(w, p, p, None, p, p, 4, 256, 16, p, base, need - 1, st)
    assert rc != 0 and "workspace" in lib.tt_last_error().decode()
    assert lib.tt_gemma_forward(w, p, p, p, p, p, 4, 256, 16, p, base, need, st) == -1 and "type_ids" in lib.tt_last_error().decode()
    assert lib.tt_gemma_forward(w, p, p, None, p, p, 4, 200, 16, p, base, need, st) == -1 and "n_rows" in lib.tt_last_error().decode()
    layers = (_GemmaLayerW * 1)()
    for kw, text in ((dict(hidden=1152), "hidden"), (dict(head_dim=128), "head_dim"), (dict(ffn=1100), "ffn"),
                     (dict(heads=3, kv_heads=2), "kv_heads")):
        a = dict(hidden=768, layers=1, heads=3, kv_heads=1, head_dim=256, ffn=1152, vocab=2048, window=256, rms_eps=1e-6,
                 global_rope_theta=1e6, local_rope_theta=1e4, embed_scale=27.75, embed=1, final_norm=1)
        a.update(kw)
        bad = _GemmaW(layer=ctypes.cast(layers, ctypes.POINTER(_GemmaLayerW)), **a)
        assert lib.tt_gemma_workspace_bytes(ctypes.byref(bad), 256) == 0
        rc = lib.tt_gemma_forward(ctypes.byref(bad), None, None, None, None, None, 1, 256, 16, None, None, 0, st)
        assert rc in (-1, -2) and text in lib.tt_last_error().decode(), (kw, rc, lib.tt_last_error())
    assert lib.tt_attention_window_gqa(p, 1280, 0, 768, p, 2048, p, 768, p, p, 1, 256, 3, 1, 128, 16, 8, st) == -2
    assert lib.tt_gemma_qk_norm_rope(p, 1280, p, p, p, 256, 3, 1, 64, 1e-6, 1e4, p, 2048, st) == -2
    assert lib.tt_gemma_add_norm(p, p, p, p, 8, 320, 1e-6, p, p, st) == -2
    torch.cuda.synchronize()
