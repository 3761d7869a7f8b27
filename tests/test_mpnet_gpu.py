"""GPU: the MPNet path (csrc/mpnet.hip, the RelBias policy of csrc/varlen.h's attention tile, tensor_truth_amd/mpnet.py).

* ``tt_attention_relbias[_f16]`` against an fp64 softmax attention that adds the bias, on the element-rounded operands.  The bound is
  tests/test_modernbert_gpu.py's ``_window_reference`` bound, per output element and derived from the fp64 terms, with the score's
  error grown by what the bias adds: the table entry is an fp32 product (rel_bias * log2 e, one rounding) added in fp32 (the sum's
  rounding is the existing 2 u (|s| + max |s|) term, s now holding the bias): 2 u |bias|.  A mirrored bias and a bias shifted one
  row are defects the bound must catch: shown on the fp64 references themselves.  An all-zero table gives ``tt_attention_window``'s
  bits.
* The fixture checkpoint (tests/golden/make_mpnet_golden.py) through ``HipHuggingFaceEmbedding``: hidden states within 2 e_<type>
  of the fp64 model's, e_<type> the same model's own error in that type on the CPU, read from the fixture at test time (the factor 2
  is the one the ModernBERT and Gemma tests give a second 16-bit implementation); embeddings with cos >= 0.999; every defect
  reference of the fixture outside the bound.
* One layer at the published width (768, 12 heads, 3072) against transformers in fp32 on the device, bounded the same way by
  transformers' own 16-bit run there.
* Refused arguments, and a batch of one 510-token sequence and sixty-three 1-token sequences.
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
NAME = "mpnet_mean_l2"
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
KEY = {"bfloat16": "bf16", "float16": "fp16"}
FACTOR = 2.0
U = 2.0 ** -24
LAM = 4.0
LOG2E = 1.4426950408889634
R = 128
# what the kernel rounds: P and the output to the element type (fp16: subnormals on a grid of 2^-24)
EPS = {torch.bfloat16: dict(p=2.0 ** -8 + 2 * U, p_abs=0.0, out=2.0 ** -8 + 2 * U, out_abs=0.0),
       torch.float16: dict(p=2.0 ** -11 + 2 * U, p_abs=2.0 ** -25, out=2.0 ** -11 + 2 * U, out_abs=2.0 ** -25)}
ATT_LENS = [1, 8, 9, 92, 129, 300]      # packed back to back: 8-row groups shared, 539 rows in 640
ATT_HEADS = 4


def _lib_and_stream(dev):
    from tensor_truth_amd import _lib

    return _lib, _lib.load_library(), torch.cuda.current_stream(dev).cuda_stream


def _sfx(dt):
    return "_f16" if dt == torch.float16 else ""


def _v8(x):                                          # [T][H] -> the V8 layout [T/8][H][8]
    T, H = x.shape
    return x.reshape(T // 8, 8, H).permute(0, 2, 1).contiguous()


def _ratio(err, bound):
    """largest error in units of its bound (an exact result under a zero bound counts as 0)"""
    assert torch.isfinite(bound).all() and (bound >= 0).all(), "the bound itself is not finite"
    return torch.where(err == 0, torch.zeros_like(err), err / bound).max().item()


# ---- biased attention against fp64 ----------------------------------------------------------------------------------------------
def _bias_matrix(table, n, kind="right"):
    """table [heads][257] (natural units) -> B [heads][n][n], B[h][i][j] = table[h][clamp(j - i, -R, R) + R]; the defects:
    "mirrored" reads the distance i - j, "shifted" gives query i the row of query i + 1."""
    i = torch.arange(n, device=table.device)
    d = i[None, :] - i[:, None]
    if kind == "mirrored":
        d = -d
    elif kind == "shifted":
        d = d - 1
    return table[:, d.clamp(-R, R) + R]


def _relbias_reference(q, k, v, table, starts, lens, heads, eps=None, kind="right"):
    """fp64 attention of (q, k, v) [T][H] per sequence and head with the bias added to the scaled scores -> (O, bound) over the
    sequences' rows in order; bound None without eps.  The terms are ``_window_reference``'s (tests/test_modernbert_gpu.py) with
    every key live and 2 u |bias| more in the score's error."""
    dh, scale = 64, 0.125
    outs, bounds = [], []
    for s0, n in zip(starts, lens):
        Q, K, V = (x[s0:s0 + n].double().view(n, heads, dh).transpose(0, 1) for x in (q, k, v))
        B = _bias_matrix(table.double(), n, kind)
        S = (Q @ K.transpose(1, 2)) * scale + B
        P = torch.softmax(S, dim=-1)
        O = P @ V
        outs.append(O.transpose(0, 1).reshape(n, heads * dh))
        if eps is None:
            continue
        Sa = S.abs()
        dS = (LAM * U * math.sqrt(dh) * (Q.abs() @ K.abs().transpose(1, 2)) * scale + 2 * U * (Sa + Sa.amax(-1, keepdim=True))
              + 2 * U * B.abs())
        dS = dS * (1.0 + dS.amax())                    # (second order)
        PW, Oa, Vabs = P * dS, O.abs(), V.abs()
        PV = P @ Vabs
        V2 = V.pow(2).sum(1, keepdim=True).sqrt().expand(-1, n, -1)       # sqrt(sum_j v_jd^2) over the sequence's keys
        l_inv = torch.exp(S.amax(-1, keepdim=True) - torch.logsumexp(S, -1, keepdim=True))
        b = (PW @ Vabs + Oa * PW.sum(-1, keepdim=True) + eps["p"] * (PV + Oa) + LAM * eps["p_abs"] * V2 * l_inv
             + LAM * U * math.sqrt(n) * (PV + Oa) + eps["out"] * Oa + eps["out_abs"])
        bounds.append(b.transpose(0, 1).reshape(n, heads * dh))
    return torch.cat(outs), (torch.cat(bounds) if eps is not None else None)


def _attention_inputs(dev, dt, seed=11):
    H = ATT_HEADS * 64
    starts = np.concatenate([[0], np.cumsum(ATT_LENS)[:-1]]).tolist()
    T = 640
    assert starts[-1] + ATT_LENS[-1] == 539 and any(s % 8 for s in starts)
    g = torch.Generator(device=dev).manual_seed(seed)
    q, k, v = (torch.randn(T, H, generator=g, device=dev) * s for s in (1.5, 1.5, 1.0))
    table = torch.randn(ATT_HEADS, 2 * R + 1, generator=g, device=dev)          # unit scale, natural units
    return q.to(dt), k.to(dt), v.to(dt), table, starts, T


def _run_relbias(dev, dt, q, k, v, table_log2, starts, T, entry="tt_attention_relbias"):
    _lib, lib, st = _lib_and_stream(dev)
    H = ATT_HEADS * 64
    qkv = torch.cat([q, k, v], dim=1).contiguous()
    vt = _v8(v)
    out = torch.zeros(T, H, dtype=dt, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(ATT_LENS, dtype=torch.int32, device=dev)
    args = [qkv.data_ptr(), 3 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, ss.data_ptr(), sl.data_ptr(), len(ATT_LENS), T,
            ATT_HEADS, 64, max(ATT_LENS)]
    args += [table_log2.data_ptr(), st] if entry == "tt_attention_relbias" else [T, st]
    rc = getattr(lib, entry + _sfx(dt))(*args)
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    live = torch.zeros(T, dtype=torch.bool, device=dev)
    for s, n in zip(starts, ATT_LENS):
        live[s:s + n] = True
    assert (out[~live].view(torch.int16) == 0).all()          # rows of no sequence are not written
    return out, live


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_biased_attention_matches_fp64(dev, built_lib, dt):
    q, k, v, table, starts, T = _attention_inputs(dev, dt)
    table_log2 = (table * LOG2E).contiguous()
    out, live = _run_relbias(dev, dt, q, k, v, table_log2, starts, T)
    got = out[live]
    # the reference adds the table the kernel reads (fp32 entries, back in natural units in fp64)
    ref_table = table_log2.double() / LOG2E
    want, bound = _relbias_reference(q, k, v, ref_table, starts, ATT_LENS, ATT_HEADS, EPS[dt])
    assert torch.isfinite(got.float()).all()
    err = (got.double() - want).abs()
    ratio = _ratio(err, bound)
    print(f"\nrelbias {dt}: max error / bound = {ratio:.3f} (max abs error {err.max().item():.3g})")
    assert ratio <= 1.0, f"relbias {dt}: error {ratio:.3g} x its bound"
    # teeth: the mirrored and the one-row-shifted bias lie outside the bound -- of the references themselves, and of the kernel
    for kind in ("mirrored", "shifted"):
        other, _ = _relbias_reference(q, k, v, ref_table, starts, ATT_LENS, ATT_HEADS, kind=kind)
        gap = _ratio((other - want).abs(), bound)
        print(f"relbias {dt}: the {kind} bias lies {gap:.3g} bounds away")
        assert gap > 2.0, f"the fp64 references of the right and the {kind} bias are only {gap:.3g} bounds apart on these inputs"
        assert _ratio((got.double() - other).abs(), bound) > 1.0


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_zero_table_gives_the_unbiased_tiles_bits(dev, built_lib, dt):
    """The policy adds 0.0f to every score: the bits of ``tt_attention_window`` with a window of n_rows (every key of the sequence,
    the same walk over the key blocks)."""
    q, k, v, table, starts, T = _attention_inputs(dev, dt, seed=12)
    biased, _ = _run_relbias(dev, dt, q, k, v, torch.zeros_like(table), starts, T)
    plain, live = _run_relbias(dev, dt, q, k, v, None, starts, T, entry="tt_attention_window")
    assert torch.isfinite(plain[live].float()).all() and torch.equal(biased, plain)
    other, _ = _run_relbias(dev, dt, q, k, v, (table * LOG2E).contiguous(), starts, T)
    assert not torch.equal(other, plain)


# ---- the fixture checkpoint -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(os.path.join(GOLDEN, f"{NAME}_expected.npz"))
    lens = z["lens"].tolist()
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    seqs = [z["ids"][f:f + n].tolist() for f, n in zip(first, lens)]
    hidden = {}
    for fn in (f"{NAME}_hidden.npz", f"{NAME}_hidden_510.npz"):
        zh = np.load(os.path.join(GOLDEN, fn))
        hidden.update({int(k.split("_")[1]): zh[k].astype(np.float64) for k in zh.files})
    assert sorted(hidden) == list(range(len(seqs))) and all(hidden[i].shape == (n, 256) for i, n in enumerate(lens))
    return seqs, {k: z[k] for k in z.files}, hidden


def _embedder(dtype):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding
    from tensor_truth_amd.tokenization import HashTokenizer

    # the fixture directory brings no tokenizer: the test hands token ids over, and says so
    return HipHuggingFaceEmbedding(os.path.join(GOLDEN, NAME), device="cuda",
                                   model_kwargs={"torch_dtype": dtype, "tokenizer": HashTokenizer("mpnet", 600)})


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_fixture_through_the_embedder(dev, built_lib, dtype):
    from tensor_truth_amd.encoder import pack_tokens
    from tensor_truth_amd.mpnet import MpnetWeights

    seqs, z, want = _fixture()
    assert [len(s) for s in seqs] == [1, 9, 17, 92, 130, 300, 510]
    e_ref = float(z[f"e_{KEY[dtype]}"])
    assert 1e-4 < e_ref < 0.5
    bound = FACTOR * e_ref
    emb = _embedder(dtype)
    assert emb.config.arch == "mpnet" and emb.pooling == "mean" and isinstance(emb._model, MpnetWeights)
    assert emb.max_length == 512 and (emb.query_instruction, emb.text_instruction) == ("", "")
    batch = pack_tokens(seqs, emb.config)
    assert int(batch.pos[0]) == 2 and batch.max_len == 510
    hidden, _ = emb._encoder.forward_packed(batch)
    torch.cuda.synchronize()
    hidden = hidden.double().cpu().numpy()
    got = [hidden[s:s + n] for s, n in zip(batch.seq_start, batch.seq_len)]
    assert all(np.isfinite(g).all() for g in got)
    err = max(float(np.abs(g - want[i]).max()) for i, g in enumerate(got))
    print(f"\n{NAME} {dtype}: hidden states max |hip - fp64| = {err:.5f}, e_ref = {e_ref:.5f}, ratio = {err / e_ref:.3f}, bound = {bound:.5f}")
    assert err <= bound, f"{NAME} {dtype}: {err:.5f} > {FACTOR} x e_ref = {bound:.5f}"
    vec = emb.embed_token_batches(seqs).double().cpu().numpy()
    cos = (vec * z["emb"]).sum(1) / np.linalg.norm(vec, axis=1)
    print(f"{NAME} {dtype}: min cos to the fp64 pooled embeddings = {cos.min():.6f}")
    assert np.abs(np.linalg.norm(vec, axis=1) - 1).max() < 1e-3 and cos.min() >= 0.999
    # every defect reference lies outside the bound
    for defect in ("nobias", "mirrored", "shifted", "nexthead", "pos0"):
        gap = max(float(np.abs(got[i] - z[f"{defect}_{k}"].astype(np.float64)).max()) for k, i in enumerate(z["defect_idx"].tolist()))
        print(f"{NAME} {dtype}: defect {defect}: max |hip - defect| = {gap:.5f}")
        assert gap > bound, f"the defect reference '{defect}' lands inside the bound"
    # strings go through the tokenizer the caller handed over
    v = np.asarray(emb.get_text_embedding("a few words of text"))
    assert v.shape == (256,) and np.isfinite(v).all() and abs(np.linalg.norm(v) - 1) < 1e-3


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_long_sequence_among_sixty_three_single_tokens(dev, built_lib, dtype):
    """A batch whose longest sequence (510 tokens) sets the grid for sixty-three sequences of one token: every row within the bound
    of the fp64 states, the long sequence's rows the bits it has in the fixture's own batch."""
    from tensor_truth_amd.encoder import pack_tokens

    seqs, z, want = _fixture()
    bound = FACTOR * float(z[f"e_{KEY[dtype]}"])
    emb = _embedder(dtype)
    enc, cfg = emb._encoder, emb.config
    many = [seqs[0]] * 31 + [seqs[6]] + [seqs[0]] * 32
    batch = pack_tokens(many, cfg)
    assert len(batch.seq_len) == 64 and batch.max_len == 510 and sorted(batch.seq_len.tolist())[:63] == [1] * 63
    hidden, _ = enc.forward_packed(batch)
    ref, _ = enc.forward_packed(pack_tokens(seqs, cfg))
    torch.cuda.synchronize()
    ref_batch = pack_tokens(seqs, cfg)
    s_long, s_ref = int(batch.seq_start[31]), int(ref_batch.seq_start[6])
    assert torch.equal(hidden[s_long:s_long + 510], ref[s_ref:s_ref + 510])
    h = hidden.double().cpu().numpy()
    err_long = float(np.abs(h[s_long:s_long + 510] - want[6]).max())
    ones = np.stack([h[int(s)] for i, s in enumerate(batch.seq_start) if i != 31])
    err_one = float(np.abs(ones - want[0][0]).max())
    print(f"\n{dtype}: 510-token sequence max error {err_long:.5f}, single tokens {err_one:.5f}, bound {bound:.5f}")
    assert (ones == ones[0]).all() and err_long <= bound and err_one <= bound
    vec, _ = enc.embed_packed(batch, pooling="mean")
    cls, _ = enc.embed_packed(batch, pooling="cls")
    assert torch.isfinite(vec).all() and torch.allclose(vec[0], cls[0], atol=1e-6)        # one token: its mean is its first row


# ---- one layer at the published width -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_one_layer_at_the_published_width(dev, built_lib, dtype):
    """768 wide, 12 heads, FFN 3072, seeded weights, 248 token rows padded to 256: against transformers' MPNetModel in fp32 on the
    device, within 2 x the deviation of transformers' own run in the 16-bit type there."""
    from transformers import MPNetConfig, MPNetModel

    from tensor_truth_amd.encoder import Encoder, pack_tokens
    from tensor_truth_amd.mpnet import MPNET_BASE, MpnetWeights, synthetic_state

    dt = DTYPES[dtype]
    cfg = dataclasses.replace(MPNET_BASE, vocab_size=1000, layers=1)
    state = synthetic_state(cfg, seed=7)
    hf = MPNetModel(MPNetConfig(vocab_size=cfg.vocab_size, hidden_size=768, num_attention_heads=12, intermediate_size=3072,
                                num_hidden_layers=1, max_position_embeddings=514, layer_norm_eps=cfg.ln_eps, hidden_dropout_prob=0.0,
                                attention_probs_dropout_prob=0.0), add_pooling_layer=False).eval()
    missing, unexpected = hf.load_state_dict(state, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    g = np.random.default_rng(5)
    seqs = [[0] + g.integers(4, cfg.vocab_size, n - 2).tolist() + [2] for n in (200, 37)] + [[0]]
    batch = pack_tokens(seqs, cfg)
    assert batch.n_rows == 256 and batch.n_tokens == 238
    enc = Encoder(MpnetWeights(cfg, state, dev, dtype=dt))
    hidden, _ = enc.forward_packed(batch)
    torch.cuda.synchronize()

    def run(model):
        with torch.no_grad():
            return [model(input_ids=torch.tensor([s], device=dev)).last_hidden_state[0].double() for s in seqs]

    want = run(hf.to(dev, torch.float32))
    low = run(hf.to(dt))
    e_ref = max(float((a - b).abs().max()) for a, b in zip(low, want))
    err = max(float((hidden[s:s + n].double() - w).abs().max()) for s, n, w in zip(batch.seq_start, batch.seq_len, want))
    print(f"\nbase width {dtype}: max |hip - fp32| = {err:.5f}, transformers' own {dtype} error = {e_ref:.5f}, ratio = {err / e_ref:.3f}")
    assert 1e-4 < e_ref < 0.5 and err <= FACTOR * e_ref


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["", "_f16"])
def test_bad_arguments_refused_before_a_launch(dev, built_lib, sfx):
    from tensor_truth_amd.encoder import _EncW, _LayerW
    from tensor_truth_amd.mpnet import _MpW

    _, lib, st = _lib_and_stream(dev)
    fwd, wsb, att = (getattr(lib, n + sfx) for n in ("tt_mpnet_forward", "tt_mpnet_workspace_bytes", "tt_attention_relbias"))
    layers = (_LayerW * 1)()

    def weights(rel_bias=1, bias_table=1, **kw):
        a = dict(hidden=768, layers=1, heads=12, ffn=3072, vocab=1000, max_pos=514, type_vocab=1, ln_eps=1e-5, word_emb=1, pos_emb=1,
                 emb_ln_g=1, emb_ln_b=1)
        a.update(kw)
        return _MpW(enc=_EncW(layer=ctypes.cast(layers, ctypes.POINTER(_LayerW)), **a), rel_bias=rel_bias, bias_table=bias_table)

    def err():
        return lib.tt_last_error().decode()

    assert wsb(ctypes.byref(weights()), 256) > 0
    for kw, text in ((dict(hidden=1152, heads=18), "hidden"), (dict(hidden=320, heads=5), "hidden"), (dict(heads=8), "head_dim"),
                     (dict(hidden=384, heads=12), "head_dim"), (dict(ffn=1100), "ffn")):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        rc = fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st)
        assert rc == -2 and text in err(), (kw, rc, err())
    layers[0].qkv_w8 = 1                                   # an fp8 pointer in a layer
    w = weights()
    assert wsb(ctypes.byref(w), 256) == 0
    assert fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st) == -2 and "qkv_w8" in err()
    layers[0].qkv_w8 = None
    for kw in (dict(rel_bias=None), dict(bias_table=None)):
        w = weights(**kw)
        assert wsb(ctypes.byref(w), 256) == 0
        assert fwd(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, st) == -1 and "bias_table" in err()
    w = weights(layers=0)
    buf = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    need = wsb(ctypes.byref(w), 256)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    rc = fwd(ctypes.byref(w), p, p, p, p, p, 4, 256, 16, p, base, need, st)
    assert rc == -1 and "type_ids" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 0, 256, 16, p, base, need, st)
    assert rc == -1 and "n_seq" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 200, 16, p, base, need, st)
    assert rc == -1 and "n_rows" in err()
    rc = fwd(ctypes.byref(w), p, p, None, p, p, 4, 256, 16, p, base, need - 1, st)
    assert rc != 0 and "workspace" in err()
    assert att(p, 768, 0, 256, p, 2048, p, 256, p, p, 1, 256, 4, 32, 16, p, st) == -2 and "head_dim" in err()
    assert att(p, 768, 0, 256, p, 2048, p, 256, p, p, 1, 256, 4, 64, 16, None, st) == -1 and "null" in err()    # no table
    assert att(p, 768, 0, 600, p, 2048, p, 256, p, p, 1, 256, 4, 64, 16, p, st) == -1     # K columns past the row
    assert att(p, 768, 0, 256, p, 2048, p, 256, p, p, 1, 256, 4, 64, 300, p, st) == -1    # max_len > n_rows
    torch.cuda.synchronize()
