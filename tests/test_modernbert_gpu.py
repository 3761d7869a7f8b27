"""GPU: the ModernBERT path (csrc/modernbert.hip, tensor_truth_amd/modernbert.py).

* ``tt_attention_window[_f16]`` against an fp64 softmax attention with the exact mask, on the element-rounded operands.  The bound
  is tests/test_attention_parity_gpu.py's, per output element and derived from the operands (its module docstring), with the terms
  of a kernel that rounds P to the element type for the value product: e_p = the element type's unit roundoff (2^-8 bf16, 2^-11
  fp16 with its 2^-24 subnormal grid), e_out the same, fp32 accumulation of scores, values and the row sum (LAM u sqrt(n)).  The
  score chain's sum_t s_t^2 is bounded by dh (sum_d |q_d k_d|)^2 instead of evaluated exactly.  A window off by one row on either
  side is a defect the bound must catch: shown on the fp64 references themselves.
* ``tt_rope_v8[_f16]`` against fp64 for both bases and positions up to 8191.  Angles are fp32 in the kernel as in transformers:
  inv_freq to 5 u relative (powf within 2 ulp = 4 u, the reciprocal u), the product another u: 6 u pos inv_freq; sincosf within
  1 ulp = 2 u and the rotation's own roundings 3 u: 6 u; then the output's format (unit roundoff 2^-8 / 2^-11).  The V8 copy is
  exact.
* The fixture checkpoints (tests/golden/make_modernbert_golden.py) against transformers: the bound is the reference's own 16-bit
  error, read from the fixture at test time, e_ref[d] = max |x_d(transformers, CPU) - x_fp32|, times 2 (DESIGN.md section 4.8's
  bound and factor).  Every figure is printed before it is asserted.
* Packing independence (``torch.equal``), the embedder and reranker surfaces, 8192-token sequences at the base geometry.
"""
import ctypes
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("modernbert_cls_l4", "modernbert_mean_l5")
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
KEY = {"bfloat16": "bf16", "float16": "fp16"}
FACTOR = 2.0          # head-room over e_ref (DESIGN.md sections 4.8 / 4.9)
U = 2.0 ** -24
LAM = 4.0
# what the windowed kernel rounds: P and the output to the element type (fp16: subnormals on a grid of 2^-24)
EPS = {torch.bfloat16: dict(p=2.0 ** -8 + 2 * U, p_abs=0.0, out=2.0 ** -8 + 2 * U, out_abs=0.0),
       torch.float16: dict(p=2.0 ** -11 + 2 * U, p_abs=2.0 ** -25, out=2.0 ** -11 + 2 * U, out_abs=2.0 ** -25)}
EDGE_LENS = [1, 8, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 129, 257, 300]


def _lib_and_stream(dev):
    from tensor_truth_amd import _lib

    return _lib, _lib.load_library(), torch.cuda.current_stream(dev).cuda_stream


def _sfx(dt):
    return "_f16" if dt == torch.float16 else ""


def _pack(lens, mode):
    """"alt": every other sequence follows its neighbour without a gap (start rows off the 8-row grid, 8-row groups shared);
    "tight": every sequence does; "aligned": every start on the 8-row grid (what pack_tokens gives)."""
    starts, row = [], 0
    for i, n in enumerate(lens):
        starts.append(row)
        row += n if (mode == "tight" or (mode == "alt" and i % 2)) else (n + 7) // 8 * 8
    return starts, (row + 255) // 256 * 256


def _v8(x):                                          # [T][H] -> the V8 layout [T/8][H][8]
    T, H = x.shape
    return x.reshape(T // 8, 8, H).permute(0, 2, 1).contiguous()


def _ratio(err, bound):
    """largest error in units of its bound (an exact result under a zero bound -- an output that is exactly 0 -- counts as 0)"""
    assert torch.isfinite(bound).all() and (bound >= 0).all(), "the bound itself is not finite"
    return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()


# ---- windowed attention against fp64 ----------------------------------------------------------------------------------------------
def _window_reference(q, k, v, starts, lens, heads, w, eps=None):
    """fp64 attention of (q, k, v) [T][H] per sequence and head, key j live for query i iff |i - j| <= w (w None: every key)
    -> (O, bound) over the sequences' rows in order; bound None without eps."""
    dh, scale = 64, 0.125
    outs, bounds = [], []
    for s0, n in zip(starts, lens):
        Q, K, V = (x[s0:s0 + n].double().view(n, heads, dh).transpose(0, 1) for x in (q, k, v))
        i = torch.arange(n, device=q.device)
        live = torch.ones(n, n, dtype=torch.bool, device=q.device) if w is None else (i[:, None] - i[None, :]).abs() <= w
        S = ((Q @ K.transpose(1, 2)) * scale).masked_fill(~live, -math.inf)
        P = torch.softmax(S, dim=-1)
        O = P @ V
        outs.append(O.transpose(0, 1).reshape(n, heads * dh))
        if eps is None:
            continue
        Sa = torch.where(live, S.abs(), torch.zeros_like(S))
        dS = LAM * U * math.sqrt(dh) * (Q.abs() @ K.abs().transpose(1, 2)) * scale + 2 * U * (Sa + Sa.amax(-1, keepdim=True))
        dS = torch.where(live, dS, torch.zeros_like(dS))
        dS = dS * (1.0 + dS.amax())                    # (second order)
        PW, Oa, Vabs = P * dS, O.abs(), V.abs()
        PV = P @ Vabs
        kn = live.sum(-1, keepdim=True).double()      # keys a query sums over
        V2 = ((live.double() @ V.pow(2))).sqrt()       # sqrt(sum_j v_jd^2) over the query's live keys
        l_inv = torch.exp(S.amax(-1, keepdim=True) - torch.logsumexp(S, -1, keepdim=True))
        b = (PW @ Vabs + Oa * PW.sum(-1, keepdim=True) + eps["p"] * (PV + Oa) + LAM * eps["p_abs"] * V2 * l_inv
             + LAM * U * kn.sqrt() * (PV + Oa) + eps["out"] * Oa + eps["out_abs"])
        bounds.append(b.transpose(0, 1).reshape(n, heads * dh))
    return torch.cat(outs), (torch.cat(bounds) if eps is not None else None)


def _run_window(dev, dt, heads, lens, mode, w, seed):
    _lib, lib, st = _lib_and_stream(dev)
    H = heads * 64
    starts, T = _pack(lens, mode)
    g = torch.Generator(device=dev).manual_seed(seed)
    q, k, v = (torch.randn(T, H, generator=g, device=dev) * s for s in (1.5, 1.5, 1.0))
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    qkv = torch.cat([q, k, v], dim=1).contiguous()
    vt = _v8(v)
    out = torch.zeros(T, H, dtype=dt, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    fn = getattr(lib, "tt_attention_window" + _sfx(dt))
    rc = fn(qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, ss.data_ptr(), sl.data_ptr(), len(lens), T, heads, 64,
            max(lens), -1 if w is None else w, st)
    _lib.check(rc, "tt_attention_window")
    torch.cuda.synchronize()
    rows = torch.cat([out[s:s + n] for s, n in zip(starts, lens)])
    # rows of no sequence are not written
    live = torch.zeros(T, dtype=torch.bool, device=dev)
    for s, n in zip(starts, lens):
        live[s:s + n] = True
    assert (out[~live].view(torch.int16) == 0).all()
    return rows, (q, k, v, starts)


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("mode", ["alt", "tight", "aligned"])
@pytest.mark.parametrize("w", [0, 1, 16, 64, None], ids=lambda w: f"w{w}")
def test_windowed_attention_matches_fp64(dev, built_lib, w, mode, dt):
    heads = 4
    got, (q, k, v, starts) = _run_window(dev, dt, heads, EDGE_LENS, mode, w, seed=5 + (w or 0))
    want, bound = _window_reference(q, k, v, starts, EDGE_LENS, heads, w, EPS[dt])
    assert torch.isfinite(got.float()).all()
    err = (got.double() - want).abs()
    ratio = _ratio(err, bound)
    print(f"\nwindow {w} {mode} {dt}: max error / bound = {ratio:.3f} (max abs error {err.max().item():.3g})")
    assert ratio <= 1.0, f"window {w} {mode} {dt}: error {ratio:.3g} x its bound"
    if w is None:
        return
    # teeth: a window off by one row on either side lies outside the bound -- of the references themselves, and of the kernel
    for bad in ([w + 1] if w == 0 else [w - 1, w + 1]):
        other, _ = _window_reference(q, k, v, starts, EDGE_LENS, heads, bad)
        gap = _ratio((other - want).abs(), bound)
        assert gap > 2.0, f"window {w}: the fp64 references of {w} and {bad} are only {gap:.3g} bounds apart on these inputs"
        assert _ratio((got.double() - other).abs(), bound) > 1.0


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_a_window_that_covers_everything_is_no_window(dev, built_lib, dt):
    """300 is the longest sequence: windows of 299 and more keep every key, walk the same key blocks and give the bits of the
    kernel with the window off; 298 masks one pair of the longest sequence and does not."""
    off, _ = _run_window(dev, dt, 12, EDGE_LENS, "alt", None, seed=9)
    for w in (299, 300, 4096, 2 ** 31 - 1):
        got, _ = _run_window(dev, dt, 12, EDGE_LENS, "alt", w, seed=9)
        assert torch.equal(got, off), w
    less, _ = _run_window(dev, dt, 12, EDGE_LENS, "alt", 298, seed=9)
    assert not torch.equal(less, off)


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("mode", ["tight", "aligned"])
def test_causal_and_unwindowed_tiles_agree_on_last_rows(dev, built_lib, mode, dt):
    """The decoder's causal kernel and the window kernel run one tile routine (csrc/varlen.h), whose arithmetic for a query does
    not depend on what the other 15 queries of its tile may see.  For the last row of a sequence "keys <= q" and "every key of the
    sequence" are the same set, walked in the same blocks: that row comes out of ``tt_attention_causal_gqa`` (heads == kv_heads,
    head_dim 64) and of ``tt_attention_window`` (no window) with the same bits."""
    _lib, lib, st = _lib_and_stream(dev)
    heads, lens = 2, [1, 7, 8, 16, 17, 33, 40, 75]
    H = heads * 64
    starts, T = _pack(lens, mode)
    assert T == 256
    g = torch.Generator(device=dev).manual_seed(23)
    q, k, v = (torch.randn(T, H, generator=g, device=dev) * s for s in (1.5, 1.5, 1.0))
    qkv = torch.cat([q.to(dt), k.to(dt), v.to(dt)], dim=1).contiguous()
    vt = _v8(v.to(dt))
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    causal, window = (torch.zeros(T, H, dtype=dt, device=dev) for _ in range(2))
    rc = getattr(lib, "tt_attention_causal_gqa" + _sfx(dt))(qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, causal.data_ptr(), H,
                                                            ss.data_ptr(), sl.data_ptr(), len(lens), T, heads, heads, 64, max(lens), st)
    _lib.check(rc, "tt_attention_causal_gqa")
    rc = getattr(lib, "tt_attention_window" + _sfx(dt))(qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, window.data_ptr(), H,
                                                        ss.data_ptr(), sl.data_ptr(), len(lens), T, heads, 64, max(lens), -1, st)
    _lib.check(rc, "tt_attention_window")
    torch.cuda.synchronize()
    last = torch.tensor([s + n - 1 for s, n in zip(starts, lens)], device=dev)
    assert torch.isfinite(causal[last].float()).all(dim=1).all() and torch.isfinite(window[last].float()).all(dim=1).all()
    assert torch.equal(causal[last], window[last])


# ---- RoPE row op against fp64 -------------------------------------------------------------------------------------------------------
def _rope_reference(x, pos, theta, heads):
    """fp64 rotate-half RoPE of the q and k heads of x [T][3H] -> (rotated [T][2H], angles [T][32])."""
    T = x.shape[0]
    i = torch.arange(32, device=x.device, dtype=torch.float64)
    ang = pos.double()[:, None] * theta ** (-2.0 * i / 64.0)                    # [T][32]
    h = x[:, : 2 * heads * 64].double().view(T, 2 * heads, 2, 32)
    a, b = h[:, :, 0], h[:, :, 1]
    c, s = ang.cos()[:, None], ang.sin()[:, None]
    return torch.stack([a * c - b * s, b * c + a * s], dim=2).reshape(T, 2 * heads * 64), ang


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("theta", [160000.0, 10000.0])
def test_rope_row_op_matches_fp64(dev, built_lib, theta, dt):
    _lib, lib, st = _lib_and_stream(dev)
    heads, T = 4, 512
    H = heads * 64
    g = torch.Generator(device=dev).manual_seed(17)
    x = torch.randn(T, 3 * H, generator=g, device=dev).to(dt)
    pos = torch.randint(0, 8192, (T,), generator=g, device=dev, dtype=torch.int32)
    pos[:4] = torch.tensor([0, 1, 8191, 8190], dtype=torch.int32, device=dev)
    qkv = x.clone()
    vt = torch.zeros(T // 8, H, 8, dtype=dt, device=dev)
    rc = getattr(lib, "tt_rope_v8" + _sfx(dt))(qkv.data_ptr(), 3 * H, pos.data_ptr(), T, heads, 64, theta, vt.data_ptr(), 8 * H, st)
    _lib.check(rc, "tt_rope_v8")
    torch.cuda.synchronize()
    assert torch.equal(vt, _v8(x[:, 2 * H:])) and torch.equal(qkv[:, 2 * H:], x[:, 2 * H:])       # the V8 copy, exactly
    want, ang = _rope_reference(x, pos, theta, heads)
    e_out, out_abs = (2.0 ** -8, 0.0) if dt == torch.bfloat16 else (2.0 ** -11, 2.0 ** -25)
    mag = x[:, : 2 * H].double().view(T, 2 * heads, 2, 32).abs().sum(2, keepdim=True).expand(-1, -1, 2, -1).reshape(T, 2 * H)
    d_ang = (6 * U * ang + 6 * U)[:, None, None, :].expand(-1, 2 * heads, 2, -1).reshape(T, 2 * H)
    bound = mag * d_ang + e_out * want.abs() + out_abs
    err = (qkv[:, : 2 * H].double() - want).abs()
    ratio = _ratio(err, bound)
    print(f"\nrope theta {theta:g} {dt}: max error / bound = {ratio:.3f} (max abs error {err.max().item():.3g})")
    assert ratio <= 1.0
    # teeth: the other base, and positions off by one, lie outside the bound
    for bad_theta, bad_pos in ((170000.0 - theta, pos), (theta, pos + 1)):
        bad, _ = _rope_reference(x, bad_pos, bad_theta, heads)
        assert _ratio((qkv[:, : 2 * H].double() - bad).abs(), bound) > 10.0


# ---- the fixture checkpoints against transformers ---------------------------------------------------------------------------------
def _fixture(name):
    z = np.load(os.path.join(GOLDEN, f"{name}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return [z["ids"][f:f + n].tolist() for f, n in zip(first, lens)], z


def _fixture_encoder(name, dt, dev):
    from tensor_truth_amd import weights
    from tensor_truth_amd.encoder import Encoder
    from tensor_truth_amd.modernbert import ModernBertWeights

    d = os.path.join(GOLDEN, name)
    with open(os.path.join(d, "config.json")) as f:
        cfg = weights._config_from_hf(json.load(f))
    return Encoder(ModernBertWeights(cfg, weights.load_state(d), dev, dtype=dt))


def _reranker(name, dtype, **kw):
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank

    mk = dict(torch_dtype=dtype)
    mk.update(kw.pop("model_kwargs", {}))
    return HipSentenceTransformerRerank(os.path.join(GOLDEN, name), device="cuda", model_kwargs=mk, **kw)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_hidden_states_match_transformers(dev, built_lib, name, dtype):
    """max |hidden_hip - hidden_fp32| <= 2 e_ref[d] over the four stored sequences (17, 34, 129 and 600 tokens), e_ref[d] the
    largest deviation of transformers' own CPU run in d from its fp32 run on the same sequences."""
    from tensor_truth_amd.encoder import pack_tokens

    seqs, _ = _fixture(name)
    zh = np.load(os.path.join(GOLDEN, f"{name}_hidden.npz"))
    e_ref = float(zh[f"hidden_e_{KEY[dtype]}"])
    assert 1e-4 < e_ref < 0.5
    enc = _fixture_encoder(name, DTYPES[dtype], dev)
    idx = zh["hidden_idx"].tolist()
    batch = pack_tokens([seqs[i] for i in idx], enc.cfg)
    hidden, _ = enc.forward_packed(batch)
    torch.cuda.synchronize()
    hidden = hidden.double().cpu().numpy()
    err = max(float(np.abs(hidden[s:s + n] - zh[f"hidden_{k}"]).max()) for k, (s, n) in enumerate(zip(batch.seq_start, batch.seq_len)))
    print(f"\n{name} {dtype}: hidden states max |hip - fp32| = {err:.5f}, e_ref = {e_ref:.5f}, ratio = {err / e_ref:.3f}")
    assert err <= FACTOR * e_ref, f"{name} {dtype}: {err:.5f} > {FACTOR} x e_ref = {FACTOR * e_ref:.5f}"


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_logits_match_transformers(dev, built_lib, name, dtype):
    """max |logit_hip - logit_fp32| <= 2 e_ref[d], e_ref[d] = max |logit_d - logit_fp32| of transformers' own CPU run in d.  In
    fp16 (where the defects are larger than the reference's own error, as the generator asserts): the window switched off, one RoPE
    base for every layer and a missing final norm lie outside the bound on the sequences the generator counted."""
    seqs, z = _fixture(name)
    want = z["logit_fp32"]
    e_ref = float(np.abs(z[f"logit_{KEY[dtype]}"] - want).max())
    assert 1e-4 < e_ref < 0.5 and np.ptp(want) > 8, "the fixture's own scale"
    bound = FACTOR * e_ref
    rr = _reranker(name, dtype)
    assert rr.config.num_labels == 1 and rr.activation == "sigmoid" and not rr._use_types
    got = rr._encoder.rerank(seqs, max_len=None, want_logits=True)[1].double().cpu().numpy()
    err = float(np.abs(got - want).max())
    print(f"\n{name} {dtype}: max |hip - fp32| = {err:.5f}, e_ref = {e_ref:.5f}, ratio = {err / e_ref:.3f}, bound = {bound:.5f}")
    assert err <= bound, f"{name} {dtype}: {err:.5f} > {FACTOR} x e_ref = {bound:.5f}"
    scores = rr._encoder.rerank(seqs, max_len=None).double().cpu().numpy()
    assert np.abs(scores - 1 / (1 + np.exp(-got))).max() <= 1e-6          # the head's sigmoid is its logit's
    if dtype != "float16":
        return
    for defect in ("allglobal", "onetheta", "nonorm"):
        counted = z[f"{defect}_counted"]
        assert counted.sum() >= 10
        gap = np.abs(got - z[f"logit_{defect}"])[counted]
        print(f"{name} {dtype}: defect {defect}: min |hip - defect| over {int(counted.sum())} sequences = {gap.min():.5f}")
        assert gap.min() > bound, f"the defect reference '{defect}' lands inside the bound"
    # order: two sequences whose fp32 logits are more than 4 e_ref apart keep their order
    clear = (want[:, None] - want[None, :]) > 4 * e_ref
    assert clear.sum() > 100 and ((got[:, None] - got[None, :])[clear] > 0).all()


# ---- packing independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_results_do_not_depend_on_packing(dev, built_lib, name, dt):
    """A sequence's embedding, score and logit are the same bits alone, in a ragged batch and in a batch of more than 256 sequences."""
    from tensor_truth_amd.encoder import pack_tokens

    seqs, z = _fixture(name)
    enc = _fixture_encoder(name, dt, dev)
    pooling = enc.cfg.classifier_pooling
    lens = z["lens"].tolist()
    pick = [lens.index(n) for n in (1, 17, 34, 129, 600)]

    def run(batch_seqs):
        batch = pack_tokens(batch_seqs, enc.cfg)
        emb, emb16 = enc.embed_packed(batch, pooling=pooling)
        score, logit = enc.rerank_packed(batch, want_logits=True)
        torch.cuda.synchronize()
        return emb.clone(), emb16.clone(), score.clone(), logit.clone()

    ragged = run(seqs)
    g = np.random.default_rng(7)
    filler = [g.integers(0, enc.cfg.vocab_size, int(n)).tolist() for n in g.integers(1, 40, 300)]
    where = [3, 77, 150, 151, 299]
    many_seqs = list(filler)
    for at, i in zip(where, pick):
        many_seqs[at] = seqs[i]
    many = run(many_seqs)
    for at, i in zip(where, pick):
        alone = run([seqs[i]])
        for a, r, m in zip(alone, ragged, many):
            assert torch.equal(a[0], r[i]) and torch.equal(a[0], m[at]), (lens[i], "alone / ragged / many differ")
    assert torch.isfinite(ragged[3]).all() and torch.isfinite(many[0]).all()


# ---- surface -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_embedder_surface(dev, built_lib, name, dtype):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    seqs, z = _fixture(name)
    emb = HipHuggingFaceEmbedding(os.path.join(GOLDEN, name), device="cuda", model_kwargs={"torch_dtype": dtype})
    assert emb.pooling == ("cls" if name == FIXTURES[0] else "mean") and emb.config.arch == "modernbert"
    if name == FIXTURES[1]:   # the prompts of config_sentence_transformers.json
        assert (emb.query_instruction, emb.text_instruction) == ("search_query: ", "search_document: ")
    else:
        assert (emb.query_instruction, emb.text_instruction) == ("", "")
    got = emb.embed_token_batches(seqs).double().cpu().numpy()
    cos = (got * z["emb"]).sum(1) / np.linalg.norm(got, axis=1)
    print(f"\n{name} {dtype}: min cos to transformers' pooled embeddings = {cos.min():.6f}")
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-3 and cos.min() >= 0.999
    # strings go through the checkpoint's tokenizer: [CLS] text [SEP]
    words = " ".join(f"w{t - 4}" for t in seqs[4][1:-1] if t >= 4)
    ids = emb._tokenizer.encode(words, None)
    assert ids[0] == 1 and ids[-1] == 2
    v = np.asarray(emb.get_text_embedding(words))
    assert np.isfinite(v).all() and abs(np.linalg.norm(v) - 1) < 1e-3


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("name", FIXTURES)
def test_string_pairs_through_the_postprocessor(dev, built_lib, name, dtype):
    from tensor_truth_amd.schema import NodeWithScore, QueryBundle, TextNode

    _, z = _fixture(name)
    pairs = list(zip(z["pair_query"].tolist(), z["pair_passage"].tolist()))
    want = z["pair_logit"]
    bound = FACTOR * float(np.abs(z[f"logit_{KEY[dtype]}"] - z["logit_fp32"]).max())
    raw = _reranker(name, dtype, model_kwargs={"activation": "identity"})
    assert raw.activation == "identity" and raw.max_length == 512 and _reranker(name, dtype, max_length=4096).max_length == 1024
    logits = np.asarray(raw.predict(pairs))
    print(f"\n{name} {dtype}: string pairs max |hip - fp32| = {np.abs(logits - want).max():.5f}, bound = {bound:.5f}")
    assert np.abs(logits - want).max() <= bound
    rr = _reranker(name, dtype, top_n=3, keep_retrieval_score=True)
    scores = np.asarray(rr.predict(pairs))
    assert np.abs(scores - 1 / (1 + np.exp(-want))).max() <= bound       # (sigmoid contracts: |s(a) - s(b)| <= |a - b| / 4)
    assert rr.predict([]) == [] and not rr.accepts_token_source("hf:anything")
    query = pairs[0][0]
    passages = [p for _, p in pairs]
    per_passage = rr.predict([(query, p) for p in passages])
    for call in (lambda n: rr.postprocess_nodes(n, query_bundle=QueryBundle(query_str=query)),
                 lambda n: rr.postprocess_nodes(n, QueryBundle(query_str=query))):
        nodes = [NodeWithScore(node=TextNode(text=p, id_=f"p{i}"), score=0.25) for i, p in enumerate(passages)]
        ranked = call(nodes)
        order = sorted(range(len(passages)), key=lambda i: -per_passage[i])[:3]
        assert [n.node.id_ for n in ranked] == [f"p{i}" for i in order]
        assert [n.score for n in ranked] == [per_passage[i] for i in order]
        assert all(n.node.metadata["retrieval_score"] == 0.25 for n in ranked)
    with pytest.raises(ValueError, match="Missing query bundle"):
        rr.postprocess_nodes(nodes)
    got = rr.rerank(query, passages, top_n=2)
    assert [r["index"] for r in got] == order[:2]
    # the tokenizer's template: [CLS] query [SEP] passage [SEP], no token types
    ids, types = rr._tokenizer.encode_pair_batch([pairs[0]], rr.max_length)[0]
    assert ids[0] == 1 and ids[-1] == 2 and ids.count(2) == 2 and types is None


def test_coalesced_request_threads_get_their_own_scores(dev, built_lib):
    from concurrent.futures import ThreadPoolExecutor

    name = FIXTURES[0]
    _, z = _fixture(name)
    pairs = list(zip(z["pair_query"].tolist(), z["pair_passage"].tolist()))
    rr = _reranker(name, "bfloat16")
    serial = _reranker(name, "bfloat16", coalesce=False)
    calls = [pairs[i:] + pairs[:i] for i in range(len(pairs))] * 3
    want = [serial.predict(c) for c in calls]
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(rr.predict, calls))
    assert got == want


@pytest.mark.default_precision
def test_no_torch_dtype_is_refused(dev, built_lib):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank

    with pytest.raises(NotImplementedError, match="ModernBERT.*bfloat16.*float16"):
        HipSentenceTransformerRerank(os.path.join(GOLDEN, FIXTURES[0]), device="cuda")
    with pytest.raises(NotImplementedError, match="ModernBERT.*bfloat16.*float16"):
        HipHuggingFaceEmbedding(os.path.join(GOLDEN, FIXTURES[1]), device="cuda")


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_base_geometry_runs_8192_token_sequences(dev, built_lib, dt):
    """ModernBERT-base's layers (22 x 768, 12 heads, 1152, window +-64, global every third) with seeded weights and a small vocabulary:
    two 8192-token sequences and a short one, embedded both ways and scored."""
    from tensor_truth_amd.encoder import Encoder, pack_tokens
    from tensor_truth_amd.modernbert import MODERNBERT_BASE, ModernBertWeights, synthetic_state

    cfg = dataclasses.replace(MODERNBERT_BASE, vocab_size=4096, pad_id=0, num_labels=1)
    enc = Encoder(ModernBertWeights(cfg, synthetic_state(cfg, seed=5), dev, dtype=dt))
    g = np.random.default_rng(3)
    seqs = [g.integers(0, cfg.vocab_size, n).tolist() for n in (8192, 40, 8192)]
    batch = pack_tokens(seqs, cfg)
    assert batch.max_len == 8192 and int(batch.pos.max()) == 8191
    hidden, _ = enc.forward_packed(batch)
    for pooling in ("cls", "mean"):
        emb, _ = enc.embed_packed(batch, pooling=pooling)
        assert torch.isfinite(emb).all() and torch.allclose(emb.norm(dim=1), torch.ones(3, device=dev), atol=1e-3)
    scores, logits = enc.rerank_packed(batch, want_logits=True)
    torch.cuda.synchronize()
    live = np.zeros(batch.n_rows, dtype=bool)
    for s, n in zip(batch.seq_start, batch.seq_len):
        live[s:s + n] = True
    assert torch.isfinite(hidden.float()).all() and hidden[torch.from_numpy(live).to(dev)].float().abs().mean() > 0.1
    assert torch.isfinite(logits).all() and ((scores > 0) & (scores < 1)).all()


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["", "_f16"])
def test_bad_arguments_refused_before_a_launch(dev, built_lib, sfx):
    from tensor_truth_amd.modernbert import _MbLayerW, _MbW

    _, lib, st = _lib_and_stream(dev)
    layers = (_MbLayerW * 1)()
    fwd, wsb, head, rope, att = (getattr(lib, n + sfx) for n in ("tt_modernbert_forward", "tt_modernbert_workspace_bytes",
                                                                 "tt_modernbert_head", "tt_rope_v8", "tt_attention_window"))

    def weights(**kw):
        a = dict(hidden=768, layers=1, heads=12, ffn=1152, vocab=1000, local_attention=128, norm_eps=1e-5, global_rope_theta=160000.0,
                 local_rope_theta=10000.0, embed=1, emb_norm=1, final_norm=1)
        a.update(kw)
        return _MbW(layer=ctypes.cast(layers, ctypes.POINTER(_MbLayerW)), **a)

    assert wsb(ctypes.byref(weights()), 256) > 0
    for kw, text in ((dict(hidden=1152, heads=18), "hidden"), (dict(hidden=320, heads=5), "hidden"), (dict(heads=8), "head_dim"),
                     (dict(ffn=1100), "ffn")):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        rc = fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st)
        assert rc == -2 and text in lib.tt_last_error().decode(), (kw, rc, lib.tt_last_error())
    w = weights(layers=0)
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    need = wsb(ctypes.byref(w), 256)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    rc = fwd(ctypes.byref(w), p, p, p, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "type_ids" in lib.tt_last_error().decode()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 0, 256, 16, p, base, need, st)
    assert rc == -1 and "n_seq" in lib.tt_last_error().decode()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 200, 16, p, base, need, st)
    assert rc == -1 and "n_rows" in lib.tt_last_error().decode()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, need - 1, st)
    assert rc != 0 and "workspace" in lib.tt_last_error().decode()
    rc = head(ctypes.byref(w), p, 768, p, p, 4, 0, p, None, st)
    assert rc == -1 and "no classification head" in lib.tt_last_error().decode()
    rc = head(ctypes.byref(weights(head_dense_wt=1, head_norm=1, cls_w=1, cls_b=1)), p, 768, p, p, 4, 2, p, None, st)
    assert rc == -1 and "pooling" in lib.tt_last_error().decode()
    assert rope(p, 768, p, 256, 4, 128, 1e4, p, 2048, st) == -2 and "head_dim" in lib.tt_last_error().decode()
    assert rope(p, 700, p, 256, 4, 64, 1e4, p, 2048, st) == -1
    assert att(p, 768, 0, 256, p, 2048, p, 256, p, p, 1, 256, 4, 32, 16, 8, st) == -2 and "head_dim" in lib.tt_last_error().decode()
    assert att(p, 768, 0, 600, p, 2048, p, 256, p, p, 1, 256, 4, 64, 16, 8, st) == -1     # K columns past the row
    assert att(p, 768, 0, 256, p, 2048, p, 256, p, p, 1, 256, 4, 64, 300, 8, st) == -1    # max_len > n_rows
    torch.cuda.synchronize()
