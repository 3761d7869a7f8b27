"""GPU: the decoder embedder (Qwen3Model architecture) -- its kernels against fp64 restatements of the values they were given,
the whole model against the transformers fixtures (tests/golden/make_qwen3_golden.py) and a 0.6B-shaped model against an fp32
torch restatement, and the embedding surface (batching invariance, prompts, retrieval).

Attention bound (per output element, query q, feature d; u = unit roundoff of the element type: 2^-8 bf16, 2^-11 fp16).  The
kernel computes scores s_j in fp32 from the given Q, K (exact products, fp32 sums: |err| <= D 2^-24 sum_i |q_i k_ji| / sqrt(D)),
scales them to the log2 domain (2^-24 relative) and exponentiates (exp2f, a few ulp): the weights' relative error is at most
e_q = 2 max_j(err_j) + 2^-20.  P is rounded to the element type (relative u) and the denominator sums the ROUNDED weights, so
    |O~ - O| <= (u + e_q) / (1 - u) * sum_j w_j |v_jd - O_d| + L 2^-24 sum_j w_j |v_jd|
(w = the exact softmax weights; the P.V sum is fp32 over L keys) and the output rounding adds u |O_d|.  The test takes 1.05x the
first two terms, with sum_j w_j |v_jd - O_d| <= sum_j w_j |v_jd| + |O_d|.

RoPE bound: q and k heads are RMS-normalised in fp32 (a few ulp), the angle pos * theta^(-2i/D) is fp32 (inverse frequency and
product each within 2^-23 relative: |d angle| <= pos inv_i 2^-21), sincosf within 2^-21, and the output rounded once:
    |out~ - out| <= u |out| + (|xa| + |xb|) (pos inv_i 2^-21 + 2^-18)
with xa, xb the normalised, gained pair (fp64)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("qwen3_d64_r1", "qwen3_d128_r2")
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _lib():
    from tensor_truth_amd import _lib as L

    return L.load_library()


def _sfx(dt):
    return "_f16" if dt == torch.float16 else ""


def _vt_of(v, n_rows):
    """V [n_rows][F] -> the V8 layout [n_rows / 8][F][8]."""
    return v.reshape(n_rows // 8, 8, v.shape[1]).transpose(1, 2).contiguous()


def _pack(lengths, offsets):
    starts, r = [], 0
    for n, o in zip(lengths, offsets):
        r += o
        starts.append(r)
        r += n
    n_rows = (r + 7) // 8 * 8 + 8
    return starts, n_rows


# ---- causal GQA attention ----------------------------------------------------------------------------------------------------
def _attn_reference(q, k, v, starts, lengths, nq, nkv, D, rows_of, causal=True, kv_map=None):
    """fp64 restatement on the device: -> {(b, h): (query rows, O [n][D], bound terms)}."""
    group = nq // nkv
    out = {}
    for b, (s0, L) in enumerate(zip(starts, lengths)):
        qi = rows_of(L)
        for h in range(nq):
            kvh = kv_map(h) if kv_map else h // group
            Q = q[s0 + qi, h * D:(h + 1) * D].double()
            K = k[s0:s0 + L, kvh * D:(kvh + 1) * D].double()
            V = v[s0:s0 + L, kvh * D:(kvh + 1) * D].double()
            S = Q @ K.T / math.sqrt(D)
            A = (Q.abs() @ K.abs().T) / math.sqrt(D)
            keys = torch.arange(L, device=q.device)
            live = keys[None, :] <= qi[:, None] if causal else torch.ones_like(S, dtype=torch.bool)
            S = S.masked_fill(~live, -math.inf)
            W = torch.softmax(S, dim=1)
            O = W @ V
            err = (D * 2.0 ** -24 * A).masked_fill(~live, 0).amax(dim=1, keepdim=True)
            mag = W @ V.abs()
            spread = mag + O.abs()      # >= sum_j w_j |v_jd - O_d|
            out[(b, h)] = (qi, O, 2 * err + 2.0 ** -20, spread, mag, live.sum(1, keepdim=True).double(), S.amax(1))
    return out


def _rows_of(L):
    if L <= 2100:
        return torch.arange(L, device="cuda")
    g = torch.Generator().manual_seed(L)
    pick = torch.cat([torch.arange(48), torch.arange(L - 48, L), torch.randint(48, L - 48, (160,), generator=g)])
    return torch.unique(pick).to("cuda")


ATT_CASES = [(128, 4, 2), (64, 4, 2), (64, 2, 2)]
LENGTHS = [1, 15, 17, 31, 33, 47, 49, 2049, 8192, 3, 1]
OFFSETS = [0, 3, 5, 1, 7, 2, 6, 3, 5, 1, 4]      # starts off the 8-row grid


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("D,nq,nkv", ATT_CASES)
def test_causal_gqa_attention_vs_fp64(dev, built_lib, dt, D, nq, nkv):
    lib = _lib()
    starts, n_rows = _pack(LENGTHS, OFFSETS)
    g = torch.Generator(device=dev).manual_seed(1000 + D + nq)
    ld = (nq + 2 * nkv) * D
    # logits of about 100: q and k entries N(0, 5^2) make q.k / sqrt(D) N(0, 25^2) whatever D, so a row over L keys peaks near
    # 25 sqrt(2 ln L), ~100 for L = 2049 .. 8192 -- near-one-hot softmax rows (asserted below); v entries N(0, 1)
    qkv = torch.randn(n_rows, ld, device=dev, generator=g)
    qkv[:, :(nq + nkv) * D] *= 5.0
    qkv = qkv.to(dt)
    q, k, v = qkv[:, :nq * D], qkv[:, nq * D:(nq + nkv) * D], qkv[:, (nq + nkv) * D:]
    vt = _vt_of(qkv[:, (nq + nkv) * D:].contiguous(), n_rows)
    out = torch.full((n_rows, nq * D), float("nan"), dtype=dt, device=dev)
    st = torch.tensor(starts, dtype=torch.int32, device=dev)
    ln = torch.tensor(LENGTHS, dtype=torch.int32, device=dev)
    rc = getattr(lib, "tt_attention_causal_gqa" + _sfx(dt))(qkv.data_ptr(), ld, 0, nq * D, vt.data_ptr(), 8 * nkv * D, out.data_ptr(),
                                                            nq * D, st.data_ptr(), ln.data_ptr(), len(LENGTHS), n_rows, nq, nkv, D,
                                                            max(LENGTHS), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.tt_last_error()
    torch.cuda.synchronize()
    u = U[dt]
    ref = _attn_reference(q, k, v, starts, LENGTHS, nq, nkv, D, _rows_of)
    worst = 0.0
    bounds = {}
    row_max = torch.cat([r[-1] for r in ref.values()])
    assert row_max.max().item() >= 100 and (row_max >= 90).sum().item() >= 100, "the pack does not reach logits of about 100"
    for (b, h), (qi, O, e, spread, mag, nkeys, _) in ref.items():
        got = out[starts[b] + qi, h * D:(h + 1) * D].double()
        bound = 1.05 * ((u + e) / (1 - u) * spread + nkeys * 2.0 ** -24 * mag) + u * O.abs() + 1e-30
        bounds[(b, h)] = (qi, got, bound)
        assert torch.isfinite(got).all()
        ratio = ((got - O).abs() / bound).max().item()
        worst = max(worst, ratio)
    assert worst <= 1.0, f"attention outside its bound: {worst:.3f}"
    # rows that belong to no sequence are not written
    used = torch.zeros(n_rows, dtype=torch.bool)
    for s0, L in zip(starts, LENGTHS):
        used[s0:s0 + L] = True
    assert torch.isnan(out[~used.to(dev)].float()).all()

    def outside(**defect):
        r = _attn_reference(q, k, v, starts, LENGTHS, nq, nkv, D, _rows_of, **defect)
        return any(((bounds[key][1] - r[key][1]).abs() > bounds[key][2]).any().item() for key in r)

    assert outside(causal=False), "a reference without the causal mask lands inside the bound"
    if nq != nkv:
        assert outside(kv_map=lambda h: h % nkv), "a reference with the wrong KV head lands inside the bound"


# ---- q/k RMSNorm + RoPE ----------------------------------------------------------------------------------------------------
def _rope_reference(x, pos, gq, gk, nq, nkv, D, eps, theta, shift=0, norm=True):
    xs = x.double()
    out = xs.clone()
    half = D // 2
    inv = theta ** (-torch.arange(half, dtype=torch.float64, device=x.device) * 2 / D)
    ang = (pos.double() + shift)[:, None] * inv[None, :]
    c, s = torch.cos(ang), torch.sin(ang)
    terms = torch.zeros_like(xs)
    for h in range(nq + nkv):
        hd = xs[:, h * D:(h + 1) * D]
        gain = (gq if h < nq else gk).double()
        y = hd / torch.sqrt((hd * hd).mean(1, keepdim=True) + eps) * gain if norm else hd * gain
        a, b = y[:, :half], y[:, half:]
        out[:, h * D:h * D + half] = a * c - b * s
        out[:, h * D + half:(h + 1) * D] = b * c + a * s
        t = (a.abs() + b.abs()) * (pos.double()[:, None] * inv[None, :] * 2.0 ** -21 + 2.0 ** -18)
        terms[:, h * D:h * D + half] = t
        terms[:, h * D + half:(h + 1) * D] = t
    return out[:, :(nq + nkv) * D], terms[:, :(nq + nkv) * D]


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("D,nq,nkv", [(128, 16, 8), (64, 4, 2), (64, 2, 2)])
def test_qk_norm_rope_vs_fp64(dev, built_lib, dt, D, nq, nkv):
    lib = _lib()
    n_rows = 1024
    g = torch.Generator(device=dev).manual_seed(77 + D + nq)
    ld = (nq + 2 * nkv) * D
    x = (torch.randn(n_rows, ld, device=dev, generator=g) * 5).to(dt)
    pos = torch.cat([torch.arange(512, device=dev), torch.randint(0, 8192, (n_rows - 512,), device=dev, generator=g)]).to(torch.int32)
    gq = (1 + 0.3 * torch.randn(D, device=dev, generator=g)).float()
    gk = (1 + 0.3 * torch.randn(D, device=dev, generator=g)).float()
    y = x.clone()
    vt = torch.zeros(n_rows // 8, nkv * D, 8, dtype=dt, device=dev)
    eps, theta = 1e-6, 1e6
    rc = getattr(lib, "tt_qk_norm_rope" + _sfx(dt))(y.data_ptr(), ld, pos.data_ptr(), gq.data_ptr(), gk.data_ptr(), n_rows, nq, nkv, D,
                                                    eps, theta, vt.data_ptr(), 8 * nkv * D, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.tt_last_error()
    torch.cuda.synchronize()
    u = U[dt]
    ref, terms = _rope_reference(x, pos, gq, gk, nq, nkv, D, eps, theta)
    got = y[:, :(nq + nkv) * D].double()
    bound = 1.01 * u * ref.abs() + terms + 1e-30
    ratio = ((got - ref).abs() / bound).max().item()
    assert ratio <= 1.0, f"q/k-norm + RoPE outside its bound: {ratio:.3f}"
    assert torch.equal(vt, _vt_of(x[:, (nq + nkv) * D:].contiguous(), n_rows)), "V heads not copied to the V8 layout"
    assert torch.equal(y[:, (nq + nkv) * D:], x[:, (nq + nkv) * D:])
    for defect in (dict(shift=1), dict(norm=False)):
        r, _ = _rope_reference(x, pos, gq, gk, nq, nkv, D, eps, theta, **defect)
        assert ((got - r).abs() > bound).any(), f"a reference with {defect} lands inside the bound"


# ---- whole model ---------------------------------------------------------------------------------------------------------------
def _fixture(name):
    z = np.load(os.path.join(GOLDEN, f"{name}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return [z["ids"][f:f + n].tolist() for f, n in zip(first, lens)], torch.from_numpy(z["emb"])


def _embedder(name, dtype, **mk):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    return HipHuggingFaceEmbedding(os.path.join(GOLDEN, name), device="cuda", model_kwargs=dict(torch_dtype=dtype, **mk))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_models_match_transformers(dev, built_lib, name, dtype):
    seqs, want = _fixture(name)
    emb = _embedder(name, dtype)
    assert emb.pooling == "last" and emb.config.arch == "qwen3"
    got = emb.embed_token_batches(seqs).cpu()
    cos = (got * want).sum(1)
    assert cos.min().item() >= 0.999, f"{name} {dtype}: per-sequence cosine {cos.tolist()}"
    # first-token pooling of the same forward is far off (the last token carries the sequence)
    first = _embedder(name, dtype, pooling="cls").embed_token_batches(seqs).cpu()
    multi = torch.tensor([len(s) > 1 for s in seqs])
    assert ((first * want).sum(1)[multi] < 0.95).all()


def _torch_qwen3(sd, cfg, ids, device):
    """fp32 restatement of Qwen3Model for ONE sequence -> last hidden state [L, H]."""
    H, D, nq, nkv = cfg.hidden, cfg.head_dim, cfg.heads, cfg.kv_heads
    eps = cfg.ln_eps

    def rms(x, w):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w

    W = lambda n: sd[n].to(device=device, dtype=torch.float32)  # noqa: E731
    x = W("embed_tokens.weight")[ids]
    L = x.shape[0]
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, D, 2, device=device, dtype=torch.float32) / D))
    ang = torch.arange(L, device=device, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = torch.cat([ang.cos()] * 2, 1), torch.cat([ang.sin()] * 2, 1)

    def rope(t):
        a, b = t[..., :D // 2], t[..., D // 2:]
        return t * cos[:, None, :] + torch.cat([-b, a], -1) * sin[:, None, :]

    mask = torch.ones(L, L, dtype=torch.bool, device=device).tril()
    for i in range(cfg.layers):
        p = f"layers.{i}."
        h = rms(x, W(p + "input_layernorm.weight"))
        q = (h @ W(p + "self_attn.q_proj.weight").T).view(L, nq, D)
        k = (h @ W(p + "self_attn.k_proj.weight").T).view(L, nkv, D)
        v = (h @ W(p + "self_attn.v_proj.weight").T).view(L, nkv, D)
        q, k = rope(rms(q, W(p + "self_attn.q_norm.weight"))), rope(rms(k, W(p + "self_attn.k_norm.weight")))
        k, v = k.repeat_interleave(nq // nkv, 1), v.repeat_interleave(nq // nkv, 1)
        s = torch.einsum("qhd,khd->hqk", q, k) / math.sqrt(D)
        a = torch.softmax(s.masked_fill(~mask, -math.inf), -1)
        ctx = torch.einsum("hqk,khd->qhd", a, v).reshape(L, nq * D)
        x = x + ctx @ W(p + "self_attn.o_proj.weight").T
        h = rms(x, W(p + "post_attention_layernorm.weight"))
        x = x + (torch.nn.functional.silu(h @ W(p + "mlp.gate_proj.weight").T) * (h @ W(p + "mlp.up_proj.weight").T)) @ \
            W(p + "mlp.down_proj.weight").T
    return rms(x, W("norm.weight"))


def test_qwen3_0_6b_shape_vs_fp32_torch(dev, built_lib):
    """28 x 1024, 16 / 8 heads of 128, SwiGLU 3072, seeded synthetic weights: bf16 forward vs an fp32 torch restatement."""
    from tensor_truth_amd.decoder import QWEN3_EMBEDDING_0_6B, synthetic_state
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    cfg = QWEN3_EMBEDDING_0_6B
    sd = synthetic_state(cfg, seed=606)
    emb = HipHuggingFaceEmbedding("test/qwen3-0.6b-shaped", device="cuda",
                                  model_kwargs={"encoder_config": cfg, "state_dict": sd, "torch_dtype": "bfloat16",
                                                "pooling": "last"})
    g = torch.Generator().manual_seed(5)
    seqs = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (1, 37, 300, 1100)]
    got = emb.embed_token_batches(seqs).cpu().double()
    cos = []
    with torch.no_grad():
        for s, e in zip(seqs, got):
            h = _torch_qwen3(sd, cfg, torch.tensor(s, device=dev), dev)[-1].double().cpu()
            cos.append(float((e * h).sum() / h.norm()))
    assert min(cos) >= 0.999, f"0.6B-shaped bf16 vs fp32: cosines {cos}"


# ---- surface -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_embeddings_do_not_depend_on_batching(dev, built_lib, dtype):
    seqs, _ = _fixture("qwen3_d128_r2")
    g = torch.Generator().manual_seed(3)
    seqs = seqs + [torch.randint(0, 383, (n,), generator=g).tolist() for n in (5, 9, 70, 130, 250, 8, 1)]
    emb = _embedder("qwen3_d128_r2", dtype)
    whole = emb.embed_token_batches(seqs)
    one = _embedder("qwen3_d128_r2", dtype)
    one.embed_batch_size, one.forward_tokens = 1, 1
    singles = one.embed_token_batches(seqs)
    perm = torch.randperm(len(seqs), generator=g).tolist()
    shuffled = emb.embed_token_batches([seqs[i] for i in perm])
    assert torch.equal(whole, singles)
    assert torch.equal(whole[perm], shuffled)


def test_query_prompt_and_retrieval(dev, built_lib):
    from tensor_truth_amd import scan as tscan
    from tensor_truth_amd.schema import TextNode
    from tensor_truth_amd.vector_index import HipVectorIndex

    d = os.path.join(GOLDEN, "qwen3_d64_r1")
    with open(os.path.join(d, "config_sentence_transformers.json")) as f:
        prompt = json.load(f)["prompts"]["query"]
    emb = _embedder("qwen3_d64_r1", "bfloat16", pooling=None)
    assert emb.query_instruction == prompt and emb.text_instruction == ""
    q = "w5 w17 w3 w99"
    assert emb.get_query_embedding(q) == emb.get_text_embedding(prompt + q)
    # the tokenizer's post-processor appends <|endoftext|>: that is the token pooled
    assert emb._tokenizer.encode("w1 w2")[-1] == 383
    g = torch.Generator().manual_seed(9)
    texts = [" ".join(f"w{j}" for j in torch.randint(0, 382, (int(n),), generator=g).tolist())
             for n in torch.randint(3, 60, (300,), generator=g)]
    index = HipVectorIndex(256, embed_model=emb)
    index.add([TextNode(text=t, id_=f"n{j}") for j, t in enumerate(texts)])
    vecs = torch.tensor(emb.get_text_embedding_batch(texts), device=dev).to(torch.bfloat16)
    for qs in ("w1 w2 w3", texts[17]):
        qv = emb.query_embedding_device([qs]).to(torch.bfloat16)
        _, want = tscan.scan_topk(vecs, qv, 10)
        got = [h.node.id_ for h in index.as_retriever(similarity_top_k=10).retrieve(qs)]
        assert got == [f"n{int(i)}" for i in want[0].tolist()]


@pytest.mark.default_precision
def test_no_torch_dtype_is_refused(dev, built_lib):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    with pytest.raises(NotImplementedError, match="bfloat16.*float16"):
        HipHuggingFaceEmbedding(os.path.join(GOLDEN, "qwen3_d64_r1"), device="cuda")


def test_bad_shapes_refused_before_a_launch(dev, built_lib):
    import ctypes

    from tensor_truth_amd.decoder import _DecLayerW, _DecW

    lib = _lib()
    layers = (_DecLayerW * 1)()
    for kw, code, text in ((dict(head_dim=96), -2, "head_dim"), (dict(heads=6, kv_heads=4), -1, "kv_heads"),
                           (dict(hidden=1152), -2, "hidden")):
        a = dict(hidden=1024, layers=1, heads=16, kv_heads=8, head_dim=128, ffn=3072, vocab=1000, rms_eps=1e-6, rope_theta=1e6,
                 embed=1, final_norm=1)
        a.update(kw)
        w = _DecW(layer=ctypes.cast(layers, ctypes.POINTER(_DecLayerW)), **a)
        rc = lib.tt_decoder_forward(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0,
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == code, (kw, lib.tt_last_error())
        assert text in lib.tt_last_error().decode()
    rc = lib.tt_attention_causal_gqa(None, 0, 0, 0, None, 0, None, 0, None, None, 1, 8, 6, 4, 128, 8, None)
    assert rc == -1 and "kv_heads" in lib.tt_last_error().decode()      # (the NULL-pointer check behind it gives -1 too)
    rc = lib.tt_qk_norm_rope(None, 0, None, None, None, 8, 16, 8, 96, 1e-6, 1e6, None, 0, None)
    assert rc == -2 and "head_dim" in lib.tt_last_error().decode()
    torch.cuda.synchronize()


def test_more_sequences_than_a_grid_row_holds(dev, built_lib):
    """70 000 texts of one or two tokens in ONE forward (more than the 65535 a grid's y extent holds: the ingest feeder fills a
    forward up to forward_tokens): every embedding equals the one from small forwards, bit for bit."""
    emb = _embedder("qwen3_d64_r1", "bfloat16", forward_tokens=1 << 20)
    forwards = []
    run = emb._encoder.embed_packed
    emb._encoder.embed_packed = lambda batch, pooling="cls": (forwards.append(len(batch.seq_len)), run(batch, pooling=pooling))[1]
    g = torch.Generator().manual_seed(70)
    n = 70000
    lens = torch.randint(1, 3, (n,), generator=g)
    flat = torch.randint(0, 383, (int(lens.sum()),), generator=g).to(torch.int32).numpy()
    whole = emb.embed_flat(flat, lens.numpy())
    assert forwards == [n]
    small = _embedder("qwen3_d64_r1", "bfloat16", forward_tokens=4096)
    assert torch.equal(whole, small.embed_flat(flat, lens.numpy()))


def test_decoder_without_a_pooling_config_pools_the_last_token(dev, built_lib, tmp_path):
    import shutil

    d = tmp_path / "qwen3_no_pooling"
    shutil.copytree(os.path.join(GOLDEN, "qwen3_d128_r2"), d, ignore=shutil.ignore_patterns("1_Pooling"))
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    emb = HipHuggingFaceEmbedding(str(d), device="cuda", model_kwargs={"torch_dtype": "bfloat16"})
    assert emb.pooling == "last"
    seqs, want = _fixture("qwen3_d128_r2")
    assert torch.equal(emb.embed_token_batches(seqs), _embedder("qwen3_d128_r2", "bfloat16").embed_token_batches(seqs))
