"""GPU: the T5 encoder path (csrc/t5.hip, the ReLU epilogue of csrc/gemm.hip, tensor_truth_amd/t5.py).

* Both fixture checkpoints (tests/golden/make_t5_golden.py: two relu layers; one gated-gelu layer) through
  ``HipHuggingFaceEmbedding``: hidden states within 2 e_bf16 of the fp64 model's, e_bf16 transformers' own error in bfloat16 on the
  CPU, read from the fixture at test time (the factor 2 is the one the MPNet, ModernBERT and Gemma tests give a second 16-bit
  implementation); embeddings (mean -> Dense -> Normalize) with cos >= 0.999 and unit norm; every defect reference of the fixture
  outside the bound.
* A batch of one 510-token sequence and sixty-three 1-token sequences: the long sequence's rows have the bits they have in the
  fixture's own batch, the single-token rows are identical to one another.
* One layer at the published width (768, 12 heads, 3072, relu), 256 rows, against transformers in fp32 on the device, within 2 x
  the deviation of transformers' own bfloat16 run there.
* ``tt_t5_pool_dense`` against fp64 on the bf16 hidden states.  The bound is per output element, from the fp64 terms, u = 2^-24:
    mean     n sequential fp32 additions of exact bf16 values, then the product with 1 / n (two roundings):
             dp_i = (n + 2) u mean_r |x_ri|
    Dense    K sequential multiply-adds (fused or not: at most one rounding more each) plus what dp carries in:
             dv_o = (K + 1) u sum_i |p_i| |W_oi| + sum_i dp_i |W_oi|          (no Dense: dv = dp)
    norm     the sum of squares over N values (lanes of 64, a butterfly), its square root, the reciprocal and the product:
             d out_o = dv_o / ||v|| + |v_o| / ||v|| (||dv||_2 / ||v|| + ((N + 8) / 2 + 8) u)
  times 1 + 2^-10 for the second-order terms.  The bf16 copy must be the fp32 vector rounded to nearest even, bit for bit.
* The ReLU epilogue in each GEMM form (skinny, staged 128 x 128, tiled 128 x 128, tiled 256 x 256) against an fp64 product on the
  rounded operands: |got - relu(ref)| <= 2^-8 (|relu(ref)| + a) + a, a = (K + 2) u (|A| |W|^T + |b|) (fp32 accumulation, one rounding to bf16),
  exact zeros wherever the pre-activation is below minus that accumulation bound, and the bits of relu(bias epilogue).
* Refused arguments: return code and error text for each shape limit.
Every figure is printed before it is asserted.
"""
import ctypes
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("t5_mean_dense_l2", "t5_gated_mean_dense_l2")
FACTOR = 2.0
U = 2.0 ** -24
EPI_BIAS, EPI_RELU = 0, 7


def _lib_and_stream(dev):
    from tensor_truth_amd import _lib

    return _lib, _lib.load_library(), torch.cuda.current_stream(dev).cuda_stream


def _ratio(err, bound):
    """largest error in units of its bound (an exact result under a zero bound counts as 0)"""
    assert torch.isfinite(bound).all() and (bound >= 0).all(), "the bound itself is not finite"
    return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()


# ---- the fixture checkpoints ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(name):
    z = np.load(os.path.join(GOLDEN, f"{name}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seqs = [z["ids"][f:f + n].tolist() for f, n in zip(first, lens)]
    hidden = {}
    for fn in (f"{name}_hidden.npz", f"{name}_hidden_510.npz"):
        zh = np.load(os.path.join(GOLDEN, fn))
        hidden.update({int(k.split("_")[1]): zh[k].astype(np.float64) for k in zh.files})
    assert sorted(hidden) == list(range(len(seqs))) and all(hidden[i].shape == (n, 256) for i, n in enumerate(lens))
    return seqs, {k: z[k] for k in z.files}, hidden


@functools.lru_cache(maxsize=None)
def _embedder(name):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding
    from tensor_truth_amd.tokenization import HashTokenizer

    # the fixture directory brings no tokenizer: the test hands token ids over, and says so
    return HipHuggingFaceEmbedding(os.path.join(GOLDEN, name), device="cuda",
                                   model_kwargs={"torch_dtype": "bfloat16", "tokenizer": HashTokenizer("t5", 600)})


@functools.lru_cache(maxsize=None)
def _fixture_forward(name):
    """The fixture's seven sequences in one batch -> (batch, hidden states on the device): computed once, shared, left unchanged."""
    from tensor_truth_amd.encoder import pack_tokens

    emb = _embedder(name)
    batch = pack_tokens(_fixture(name)[0], emb.config)
    hidden, _ = emb._encoder.forward_packed(batch)
    torch.cuda.synchronize()
    return batch, hidden


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_the_embedder(dev, built_lib, name):
    from tensor_truth_amd.t5 import T5Weights

    seqs, z, want = _fixture(name)
    assert [len(s) for s in seqs] == [1, 9, 17, 92, 130, 300, 510]
    e_ref = float(z["e_bf16"])
    assert 1e-4 < e_ref < 0.5
    bound = FACTOR * e_ref
    emb = _embedder(name)
    assert emb.config.arch == "t5" and emb.pooling == "mean" and isinstance(emb._model, T5Weights)
    assert emb.config.mlp_kind == (1 if "gated" in name else 0) and emb.config.layers == (1 if "gated" in name else 2)
    assert emb.max_length == 512 and emb.embed_dim == 128 and emb.include_prompt
    assert (emb.query_instruction, emb.text_instruction) == ("", "")
    batch, hidden = _fixture_forward(name)
    assert int(batch.pos.max()) == 509 and batch.max_len == 510 and int(batch.ids[1]) == 0     # rows of no sequence: <pad>
    hidden = hidden.double().cpu().numpy()
    got = [hidden[s:s + n] for s, n in zip(batch.seq_start, batch.seq_len)]
    assert all(np.isfinite(g).all() for g in got)
    err = max(float(np.abs(g - want[i]).max()) for i, g in enumerate(got))
    print(f"\n{name}: hidden states max |hip - fp64| = {err:.5f}, e_bf16 = {e_ref:.5f}, ratio = {err / e_ref:.3f}, bound = {bound:.5f}")
    assert err <= bound, f"{name}: {err:.5f} > {FACTOR} x e_bf16 = {bound:.5f}"
    vec = emb.embed_token_batches(seqs).double().cpu().numpy()
    assert vec.shape == (7, 128)
    cos = (vec * z["emb"]).sum(1) / np.linalg.norm(vec, axis=1)
    print(f"{name}: min cos to the fp64 embeddings = {cos.min():.6f}")
    assert np.abs(np.linalg.norm(vec, axis=1) - 1).max() < 1e-3 and cos.min() >= 0.999
    # every defect reference lies outside the bound
    names = [str(x) for x in z["defects"].tolist()]
    assert set(names) >= {"nobias", "mirrored", "nexthead", "div8", "layernorm", "nofinalnorm"} and ("block0only" in names) == ("gated" not in name)
    for defect in names:
        gap = max(float(np.abs(got[i] - z[f"{defect}_{k}"].astype(np.float64)).max()) for k, i in enumerate(z["defect_idx"].tolist()))
        print(f"{name}: defect {defect}: max |hip - defect| = {gap:.5f}")
        assert gap > bound, f"the defect reference '{defect}' lands inside the bound"
    cos_nd = ((vec * z["nodense_emb"]).sum(1) / np.linalg.norm(vec, axis=1)).max()
    print(f"{name}: max cos to the Dense-skipped embeddings = {cos_nd:.4f}")
    assert cos_nd < 0.999
    # strings go through the tokenizer the caller handed over: words, then </s>
    v = np.asarray(emb.get_text_embedding("a few words of text"))
    assert v.shape == (128,) and np.isfinite(v).all() and abs(np.linalg.norm(v) - 1) < 1e-3
    assert emb._tokenizer.encode("two words")[-1] == 1 and len(emb._tokenizer.encode("two words")) == 3


def test_one_long_sequence_among_sixty_three_single_tokens(dev, built_lib):
    """A batch whose longest sequence (510 tokens) sets the grid for sixty-three sequences of one token: the long sequence's rows
    are the bits it has in the fixture's own batch, the single-token rows are identical to one another, all within the bound."""
    from tensor_truth_amd.encoder import pack_tokens

    name = FIXTURES[0]
    seqs, z, want = _fixture(name)
    bound = FACTOR * float(z["e_bf16"])
    emb = _embedder(name)
    enc, cfg = emb._encoder, emb.config
    many = [seqs[0]] * 31 + [seqs[6]] + [seqs[0]] * 32
    batch = pack_tokens(many, cfg)
    assert len(batch.seq_len) == 64 and batch.max_len == 510 and sorted(batch.seq_len.tolist())[:63] == [1] * 63
    hidden, _ = enc.forward_packed(batch)
    ref_batch, ref = _fixture_forward(name)
    torch.cuda.synchronize()
    s_long, s_ref = int(batch.seq_start[31]), int(ref_batch.seq_start[6])
    assert torch.equal(hidden[s_long:s_long + 510], ref[s_ref:s_ref + 510])
    h = hidden.double().cpu().numpy()
    err_long = float(np.abs(h[s_long:s_long + 510] - want[6]).max())
    ones = np.stack([h[int(s)] for i, s in enumerate(batch.seq_start) if i != 31])
    err_one = float(np.abs(ones - want[0][0]).max())
    print(f"\n510-token sequence max error {err_long:.5f}, single tokens {err_one:.5f}, bound {bound:.5f}")
    assert (ones == ones[0]).all() and err_long <= bound and err_one <= bound
    vec, vec16 = enc.embed_packed(batch, pooling="mean")
    assert torch.isfinite(vec).all() and torch.equal(vec[0], vec[40]) and torch.equal(vec16, vec.to(torch.bfloat16))
    with pytest.raises(ValueError, match="pools the mean"):
        enc.embed_packed(batch, pooling="cls")


def test_prompt_rows_stay_out_of_the_mean(dev, built_lib):
    """``include_prompt: false``: the tail reads (seq_start + p, seq_len - p); a text with nothing behind its prompt is refused."""
    from tensor_truth_amd.encoder import pack_tokens

    name = FIXTURES[0]
    seqs, z, _ = _fixture(name)
    emb = _embedder(name)
    enc = emb._encoder
    sel = [seqs[1], seqs[2], seqs[3]]
    batch = pack_tokens(sel, emb.config)
    hidden, _ = enc.forward_packed(batch)
    vec, _ = enc.embed_packed(batch, pooling="mean", skip=5)
    torch.cuda.synchronize()
    from safetensors.torch import load_file

    W = load_file(os.path.join(GOLDEN, name, "2_Dense", "model.safetensors"))["linear.weight"].double().to(dev)
    for b, (s, n) in enumerate(zip(batch.seq_start, batch.seq_len)):
        v = W @ hidden[s + 5:s + n].double().mean(0)
        cos = float(torch.nn.functional.cosine_similarity(v, vec[b].double(), dim=0))
        full = W @ hidden[s:s + n].double().mean(0)
        cos_full = float(torch.nn.functional.cosine_similarity(full, vec[b].double(), dim=0))
        print(f"\nsequence of {n} tokens, 5 left out: cos to the fp64 tail {cos:.7f}; to the tail over every row {cos_full:.5f}")
        assert cos > 1 - 1e-5 and cos_full < cos
    with pytest.raises(ValueError, match="no token left behind its 9-token prompt"):
        enc.embed_packed(batch, pooling="mean", skip=9)
    # through the strings: the instruction's tokens are counted without its </s>
    try:
        emb.include_prompt = False
        a = np.asarray(emb._embed_texts(["alpha beta gamma"], "represent this: ").cpu())
        tk = emb._tokenizer
        ids = tk.encode("represent this: alpha beta gamma")
        assert len(tk.encode("represent this: ")) - 1 == 3 and len(ids) == 7
        b, _ = enc.embed_packed(pack_tokens([ids], emb.config), pooling="mean", skip=3)
        assert np.array_equal(a[0], b[0].cpu().numpy())
        # an empty text keeps its </s>: one row is left, and it is the whole mean
        c = emb._embed_texts([""], "represent this: ")
        d, _ = enc.embed_packed(pack_tokens([tk.encode("represent this: ")], emb.config), pooling="mean", skip=3)
        assert torch.isfinite(c).all() and torch.equal(c[0], d[0])
    finally:
        emb.include_prompt = True


# ---- one layer at the published width -----------------------------------------------------------------------------------------------
def test_one_layer_at_the_published_width(dev, built_lib):
    """768 wide, 12 heads, d_ff 3072, relu, seeded weights, 238 token rows padded to 256 (the skinny GEMMs, the ReLU epilogue among
    them): against transformers' T5EncoderModel in fp32 on the device, within 2 x the deviation of transformers' own bfloat16 run."""
    from transformers import T5Config as HFT5Config
    from transformers import T5EncoderModel

    from tensor_truth_amd.encoder import Encoder, pack_tokens
    from tensor_truth_amd.t5 import DENSE_NAME, T5_BASE, T5Weights, synthetic_state

    cfg = dataclasses.replace(T5_BASE, vocab_size=1000, layers=1)
    state = synthetic_state(cfg, seed=7)
    hf = T5EncoderModel(HFT5Config(vocab_size=cfg.vocab_size, d_model=768, d_kv=64, d_ff=3072, num_layers=1, num_heads=12,
                                   dropout_rate=0.0, layer_norm_epsilon=cfg.ln_eps, feed_forward_proj="relu",
                                   is_encoder_decoder=False, use_cache=False)).eval()
    missing, unexpected = hf.load_state_dict({k: v for k, v in state.items() if k != DENSE_NAME}, strict=False)
    assert not unexpected and all("embed_tokens" in m for m in missing), (missing, unexpected)
    g = np.random.default_rng(5)
    seqs = [g.integers(3, cfg.vocab_size, n - 1).tolist() + [1] for n in (200, 37)] + [[1]]
    batch = pack_tokens(seqs, cfg)
    assert batch.n_rows == 256 and batch.n_tokens == 238
    w = T5Weights(cfg, state, dev)
    assert w.out_dim == 768 and w.struct.dense_out == 768
    enc = Encoder(w)
    hidden, _ = enc.forward_packed(batch)
    torch.cuda.synchronize()

    def run(model):
        with torch.no_grad():
            return [model(input_ids=torch.tensor([s], device=dev)).last_hidden_state[0].double() for s in seqs]

    want = run(hf.to(dev, torch.float32))
    low = run(hf.to(torch.bfloat16))
    e_ref = max(float((a - b).abs().max()) for a, b in zip(low, want))
    err = max(float((hidden[s:s + n].double() - x).abs().max()) for s, n, x in zip(batch.seq_start, batch.seq_len, want))
    print(f"\nbase width: max |hip - fp32| = {err:.5f}, transformers' own bfloat16 error = {e_ref:.5f}, ratio = {err / e_ref:.3f}")
    assert 1e-4 < e_ref < 0.5 and err <= FACTOR * e_ref


# ---- the tail against fp64 ------------------------------------------------------------------------------------------------------------
def _tail_reference(hidden, starts, lens, W):
    """fp64 mean -> Dense (W [N][K] or None) -> Normalize over rows [start, start + len) of ``hidden`` -> (out, bound)."""
    outs, bounds = [], []
    for s, n in zip(starts, lens):
        x = hidden[s:s + n].double()
        p = x.mean(0)
        dp = (n + 2) * U * x.abs().mean(0)
        if W is None:
            v, dv = p, dp
        else:
            Wd = W.double()
            v = Wd @ p
            dv = (W.shape[1] + 1) * U * (Wd.abs() @ p.abs()) + Wd.abs() @ dp
        nv = v.norm()
        N = v.numel()
        d_out = dv / nv + v.abs() / nv * (dv.norm() / nv + ((N + 8) / 2 + 8) * U)
        outs.append(v / nv)
        bounds.append(d_out * (1 + 2.0 ** -10))
    return torch.stack(outs), torch.stack(bounds)


@pytest.mark.parametrize("dense", [128, 0], ids=["dense128", "nodense"])
@pytest.mark.parametrize("n_seq", [1, 8, 9])
def test_pool_dense_matches_fp64(dev, built_lib, n_seq, dense):
    from tensor_truth_amd.t5 import _T5W

    _lib, lib, st = _lib_and_stream(dev)
    H = 256
    g = torch.Generator(device=dev).manual_seed(100 + n_seq)
    lens = [1, 9, 17, 92, 130, 300, 5, 8, 64][:n_seq]
    starts, row = [], 3                      # ranges that start on any row, back to back with gaps of 0..2 rows
    for i, n in enumerate(lens):
        starts.append(row)
        row += n + i % 3
    T = (row + 7) // 8 * 8
    hidden = (torch.randn(T, H, generator=g, device=dev) * 1.5 + 0.25).to(torch.bfloat16)
    W = torch.randn(dense, H, generator=g, device=dev) * H ** -0.5 if dense else None
    wt = W.t().contiguous() if dense else None
    w = _T5W(d_model=H, dense_out=dense, dense_wt=wt.data_ptr() if dense else None)
    width = dense or H

    def run(ss, sl):
        s_t = torch.tensor(ss, dtype=torch.int32, device=dev)
        l_t = torch.tensor(sl, dtype=torch.int32, device=dev)
        out = torch.full((len(ss), width), float("nan"), dtype=torch.float32, device=dev)
        out16 = torch.zeros((len(ss), width), dtype=torch.bfloat16, device=dev)
        rc = lib.tt_t5_pool_dense(ctypes.byref(w), hidden.data_ptr(), H, s_t.data_ptr(), l_t.data_ptr(), len(ss), out.data_ptr(),
                                  out16.data_ptr(), st)
        _lib.check(rc, "tt_t5_pool_dense")
        torch.cuda.synchronize()
        return out, out16

    out, out16 = run(starts, lens)
    want, bound = _tail_reference(hidden, starts, lens, W)
    assert torch.isfinite(out).all()
    ratio = _ratio((out.double() - want).abs(), bound)
    print(f"\npool_dense n_seq={n_seq} dense={dense}: max error / bound = {ratio:.3f} (max abs error {(out.double() - want).abs().max().item():.3g})")
    assert ratio <= 1.0
    assert torch.equal(out16, out.to(torch.bfloat16)) and (out.double().norm(dim=1) - 1).abs().max() < 1e-6
    # a sequence alone gives the bits it gets in the batch, wherever it sits in its workgroup
    for b in {0, n_seq - 1}:
        alone, _ = run([starts[b]], [lens[b]])
        assert torch.equal(alone[0], out[b]), b
    # a shifted sub-range is another mean: its own fp64 value within its own bound, and not the full range's
    sub = [(s + 1, n - 1) for s, n in zip(starts, lens) if n > 2]
    if sub:
        ss, sl = [a for a, _ in sub], [b for _, b in sub]
        got, _ = run(ss, sl)
        want_s, bound_s = _tail_reference(hidden, ss, sl, W)
        assert _ratio((got.double() - want_s).abs(), bound_s) <= 1.0
        full = torch.stack([want[i] for i, n in enumerate(lens) if n > 2])
        assert _ratio((got.double() - full).abs(), bound_s) > 1.0


# ---- the ReLU epilogue in every GEMM form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,M,N,K", [("skinny", 192, 400, 288), ("skinny-64", 64, 128, 64), ("staged", 384, 384, 256),
                                        ("tiled-128", 2304, 2048, 128), ("tiled-256", 4096, 2048, 128)])
def test_relu_epilogue_matches_fp64(dev, built_lib, form, M, N, K):
    _lib, lib, st = _lib_and_stream(dev)
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g, device=dev) * 0.25

    def run(epi):
        C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        rc = lib.tt_gemm_bf16(A.data_ptr(), W.data_ptr(), bias.data_ptr(), None, C.data_ptr(), M, N, K, epi, st)
        _lib.check(rc, "tt_gemm_bf16")
        torch.cuda.synchronize()
        return C

    got, plain = run(EPI_RELU), run(EPI_BIAS)
    ref = A.double() @ W.double().t() + bias.double()
    acc = (K + 2) * U * (A.double().abs() @ W.double().abs().t() + bias.double().abs())
    want = ref.clamp_min(0)
    bound = 2.0 ** -8 * (want + acc) + acc
    assert torch.isfinite(got.float()).all()
    ratio = _ratio((got.double() - want).abs(), bound)
    neg = ref < -acc
    print(f"\nrelu epilogue {form} {M}x{N}x{K}: max error / bound = {ratio:.3f}; {int(neg.sum())} of {M * N} pre-activations negative")
    assert ratio <= 1.0
    assert neg.float().mean() > 0.3 and (got[neg].view(torch.int16) == 0).all(), "a negative pre-activation must give +0, bit for bit"
    assert (got >= 0).all() and (got == torch.relu(plain)).all() and (got[ref > acc] > 0).all()


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_refused_before_a_launch(dev, built_lib):
    from tensor_truth_amd.t5 import _T5LayerW, _T5W

    _, lib, st = _lib_and_stream(dev)
    fwd, wsb, tail = lib.tt_t5_forward, lib.tt_t5_workspace_bytes, lib.tt_t5_pool_dense
    layers = (_T5LayerW * 1)()

    def weights(**kw):
        a = dict(d_model=768, layers=1, heads=12, d_kv=64, d_ff=3072, vocab=1000, mlp_kind=0, num_buckets=32, max_distance=128,
                 eps=1e-6, embed=1, final_norm=1, rel_bias=1, bias_table=1, dense_out=768, dense_wt=1)
        a.update(kw)
        return _T5W(layer=ctypes.cast(layers, ctypes.POINTER(_T5LayerW)), **a)

    def err():
        return lib.tt_last_error().decode()

    assert wsb(ctypes.byref(weights()), 256) > 0 and wsb(ctypes.byref(weights(dense_out=0, dense_wt=None)), 256) > 0
    assert wsb(ctypes.byref(weights(mlp_kind=1)), 256) > wsb(ctypes.byref(weights()), 256)
    for kw, text in ((dict(d_model=1152, heads=18), "d_model"), (dict(d_model=320, heads=5), "d_model"), (dict(heads=8), "num_heads"),
                     (dict(d_kv=32, heads=24), "d_kv"), (dict(d_model=384, heads=12), "d_kv"), (dict(d_ff=1100), "d_ff"),
                     (dict(dense_out=192), "dense_out"), (dict(dense_out=2048), "dense_out"), (dict(dense_wt=None), "dense_out"),
                     (dict(num_buckets=64), "relative_attention_num_buckets"), (dict(max_distance=64), "relative_attention_max_distance"),
                     (dict(mlp_kind=2), "mlp_kind")):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        rc = fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st)
        assert rc == -2 and text in err(), (kw, rc, err())
    for kw in (dict(d_model=1152), dict(dense_out=192), dict(dense_out=2048)):
        assert tail(ctypes.byref(weights(**kw)), None, 768, None, None, 1, None, None, st) == -2 and list(kw)[0] in err()
    for kw in (dict(rel_bias=None), dict(bias_table=None)):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        assert fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st) == -1 and "bias_table" in err()
    w = weights(layers=0)
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    need = wsb(ctypes.byref(w), 1024)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    rc = fwd(ctypes.byref(w), p, p, p, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "type_ids" in err()
    rc = fwd(ctypes.byref(w), p, None, None, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "null" in err()                       # pos must be present (its values are not used)
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 0, 256, 16, p, base, need, st)
    assert rc == -1 and "n_seq" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 200, 16, p, base, need, st)
    assert rc == -1 and "n_rows" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 1024, 600, p, base, need, st)
    assert rc == -2 and "max_len" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, wsb(ctypes.byref(w), 256) - 1, st)
    assert rc != 0 and "workspace" in err()
    w = weights()
    for f in ("ln_attn", "qkv_w", "o_w", "ln_ffn", "wi"):      # every tensor of the layer but wo
        setattr(layers[0], f, 1)
    assert fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, need, st) == -1 and "layer 0" in err()
    assert tail(ctypes.byref(weights()), p, 700, p, p, 1, p, None, st) == -1 and "ld" in err()
    assert tail(ctypes.byref(weights()), p, 768, p, p, 0, None, None, st) == 0                     # nothing to do
    assert lib.tt_gemm_bf16(p, p, p, None, p, 128, 128, 64, 5, st) == -1 and "epilogue" in err()   # the internal epilogues stay internal
    torch.cuda.synchronize()
