"""GPU: the kernels behind every user-visible number -- pooling + L2 normalisation (first token, mean, last token) and the
classification heads -- each against fp64 through the C ABI, on operands that are exactly representable in the operand type, under
bounds computed from the operands with ``u = 2^-24`` (tests/tail_refs.py derives them; tests/test_tail_refs_host.py holds fp32
restatements of the kernels to the same bounds on the same inputs, without a GPU).

* ``tt_embed_pool[_f16|_f32]``, ``tt_embed_pool_last[_f16]``:  ``|y - y64| <= (H/2 + 8) u |y64|``;  ``tt_embed_pool_mean[_f16|_f32]``:
  the mean's error propagated through the normalisation.  H 8 .. 1024 with every chunk pattern of the one-wave-per-row kernels,
  n_seq 1, 4, 5, 257, ld = H and H + 8 with sentinels in the padding columns and in rows of no sequence, outputs pre-filled, the
  16-bit output bit-equal to the fp32 output rounded to nearest even (bf16; IEEE fp16 from the ``_f16`` entries), an all-zero row, an
  empty sequence and a sequence whose rows nearly cancel, one sequence of 8192 rows, a sequence alone giving the bits it gives in the
  batch, and the refusals.
* ``tt_decoder_score[_f16]``:  ``(H + 1) u sum |h_i w_i|``.
* ``tt_rerank_head[_f16|_f32]``:  against the exported GEMM the head runs (``(H + 2) u (sum |t_o w_o| + |b|)``: the gather, the
  padding, the workspace layout and ``head_out_kernel`` alone), and end to end against fp64 with the GEMM's own test tolerance.
  ``tt_rerank_head_x3[_f16]`` and ``tt_rerank_head_f16c`` delegate to the fp32 head: the same bits.
* ``tt_modernbert_head[_f16]``, ``tt_deberta_head[_f16]``:  the first-order bound of ``tail_refs.pooled_head_case``.
* every head:  ``|score - sigmoid64(logit returned)| <= 4 u`` with logits near 0, +-20 and beyond +-90, ``logits = NULL``.

For every kernel a set of named wrong references (one row past the sequence, the last row skipped, a chunk dropped, the padding
column read, a bias dropped, ...) lies outside the bound, and further than the bound from what the kernel gave.  Every figure is
printed before it is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tail_refs as T

pytestmark = pytest.mark.gpu

SUFFIX = {"bf16": "", "f16": "_f16", "f32": "_f32"}
OUT16 = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.bfloat16}      # what the 16-bit output of an entry holds
FILL = -7.0


def _lib():
    from tensor_truth_amd import _lib as L

    return L.load_library()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _verdict(what, case, got, n=None, ref=None, bound=None, wrong=None):
    """Print and assert: the kernel within the bound; every wrong reference outside it, and further than the bound from the kernel."""
    ref = (case.y64 if hasattr(case, "y64") else case.logit64) if ref is None else ref
    bound = case.bound if bound is None else bound
    wrong = case.wrong if wrong is None else wrong
    n = len(ref) if n is None else n
    got = np.asarray(got, dtype=np.float64)
    r = T.ratio(got, ref[:n], bound[:n])
    bites = {k: T.outside(v[:n], ref[:n], bound[:n]) for k, v in wrong.items()}
    apart = {k: int((np.abs(got - v[:n]) > bound[:n]).sum()) for k, v in wrong.items()}
    print(f"\n{what}: max error / bound = {r:.4f}; elements with a wrong reference outside the bound {bites}, apart from the kernel {apart}")
    assert np.isfinite(got).all(), what
    assert r <= 1.0, what
    assert all(bites.values()) and all(apart.values()), f"{what}: a wrong reference is inside the bound"
    return r


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
def _pool(lib, dev, name, hidden_d, ld, index, n, H, dt16, want16=True):
    """One pooling call over the first n entries of ``index`` (device int32 tensors) -> fp32 [n + 3][H], 16-bit [n + 3][H] (or None)."""
    out = torch.full((n + 3, H), FILL, dtype=torch.float32, device=dev)
    out16 = torch.full((n + 3, H), FILL, dtype=dt16, device=dev) if want16 else None
    rc = getattr(lib, name)(hidden_d.data_ptr(), ld, *(t.data_ptr() for t in index), n, H, out.data_ptr(),
                            out16.data_ptr() if want16 else None, _stream(dev))
    assert rc == 0, (name, rc, lib.tt_last_error())
    torch.cuda.synchronize()
    return out.cpu(), out16.cpu() if want16 else None


def _pool_checks(lib, dev, name, case, hidden_d, index, dtname):
    x = case.x
    dt16 = OUT16[dtname]
    worst = 0.0
    for n in [v for v in T.N_SEQ if v <= len(case.y64)] + ([len(case.y64)] if len(case.y64) not in T.N_SEQ else []):
        out, out16 = _pool(lib, dev, name, hidden_d, x.ld, index, n, x.H, dt16)
        worst = max(worst, _verdict(f"{name} H {x.H} ld H+{x.pad} n_seq {n}", case, out[:n].numpy(), n))
        assert (out[n:] == FILL).all() and (out16[n:].float() == FILL).all(), "rows past n_seq were written"
        assert out16[:n].view(torch.int16).equal(out[:n].to(dt16).view(torch.int16)), "the 16-bit output is not the fp32 output rounded to nearest even"
        zero = np.flatnonzero((case.y64[:n] == 0).all(1))
        assert (out[:n].numpy()[zero] == 0).all(), "an all-zero row / an empty sequence must give exactly zero"
    alone, none16 = _pool(lib, dev, name, hidden_d, x.ld, index, n, x.H, dt16, want16=False)     # NULL: nothing else changes
    assert none16 is None and alone.view(torch.int32).equal(out.view(torch.int32))
    return out, worst


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("dtname", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("H", T.H_ROW)
def test_pooling_matches_fp64(dev, built_lib, H, dtname, pad):
    lib = _lib()
    x = T.pool_inputs(H, dtname, pad, 100 + H + pad)
    hidden_d = x.hidden.to(dev)
    starts_d, lens_d, rows_d = _i32(x.starts, dev), _i32(x.lens, dev), _i32(x.rows, dev)
    sfx = SUFFIX[dtname]
    runs = [("tt_embed_pool" + sfx, T.cls_case(x, f32=dtname == "f32"), (rows_d,)), ("tt_embed_pool_mean" + sfx, T.mean_case(x), (starts_d, lens_d))]
    if dtname != "f32":
        runs.append(("tt_embed_pool_last" + sfx, T.last_case(x), (starts_d, lens_d)))
    for name, case, index in runs:
        out, _ = _pool_checks(lib, dev, name, case, hidden_d, index, dtname)
        if case.kind == "mean":
            rel = case.bound.sum(1) / np.maximum(np.abs(case.y64).sum(1), 1e-300)
            print(f"  bound / |y|: the cancelling sequence {rel[T.CANCEL]:.2e}, the 65-row sequence {rel[4]:.2e}")
        if case.kind == "last":
            assert x.starts[T.EMPTY] > 0 and (out[T.EMPTY] == 0).all(), "an empty sequence pools to the zero vector"
        # batch independence: a sequence (a row) alone, at another start row, gives the bits it gives in the batch
        for b in (2, 4, 5, T.CANCEL):
            s, n = (int(x.rows[b]), 1) if case.kind == "cls" else (int(x.starts[b]), int(x.lens[b]))
            h1 = torch.full((n + 9, x.ld), T.SENTINEL).to(x.hidden.dtype)
            h1[5:5 + n] = x.hidden[s:s + n]
            one = (_i32([5], dev),) if case.kind == "cls" else (_i32([5], dev), _i32([n], dev))
            got, _ = _pool(lib, dev, name, h1.to(dev), x.ld, one, 1, H, OUT16[dtname])
            assert got[0].view(torch.int32).equal(out[b].view(torch.int32)), f"{name}: sequence {b} alone gives other bits"


@pytest.mark.parametrize("dtname", ["bf16", "f16", "f32"])
def test_mean_pooling_of_8192_rows(dev, built_lib, dtname):
    lib = _lib()
    x = T.pool_inputs(1024, dtname, 8, 7, long=True)
    case = T.mean_case(x)
    _pool_checks(lib, dev, "tt_embed_pool_mean" + SUFFIX[dtname], case, x.hidden.to(dev), (_i32(x.starts, dev), _i32(x.lens, dev)), dtname)


def test_pooling_refusals_come_before_a_launch(dev, built_lib):
    lib = _lib()
    st = _stream(dev)
    h = torch.zeros(64, 1040, dtype=torch.bfloat16, device=dev)
    idx = torch.zeros(8, dtype=torch.int32, device=dev)
    out = torch.full((8, 1040), FILL, device=dev)
    out16 = torch.full((8, 1040), FILL, dtype=torch.bfloat16, device=dev)

    def call(name, H, ld, n):
        index = (idx.data_ptr(),) if name in ("tt_embed_pool", "tt_embed_pool_f16", "tt_embed_pool_f32") else (idx.data_ptr(), idx.data_ptr())
        return getattr(lib, name)(h.data_ptr(), ld, *index, n, H, out.data_ptr(), out16.data_ptr(), st)

    for name in ("tt_embed_pool", "tt_embed_pool_f16", "tt_embed_pool_mean", "tt_embed_pool_mean_f16", "tt_embed_pool_last", "tt_embed_pool_last_f16"):
        for H, ld in ((0, 8), (12, 16), (1032, 1032)):
            assert call(name, H, ld, 4) == -2 and lib.tt_last_error(), (name, H)
        assert call(name, 128, 120, 4) == -1, name
        assert call(name, 128, 128, 0) == 0, name
    for name in ("tt_embed_pool_f32", "tt_embed_pool_mean_f32"):
        assert call(name, 128, 120, 4) == -1 and call(name, 128, 128, 0) == 0, name
    torch.cuda.synchronize()
    assert (out == FILL).all() and (out16.float() == FILL).all(), "a refused call or one of no sequence wrote"


# ---- sigmoid ---------------------------------------------------------------------------------------------------------------------
def _sigmoid_ok(what, scores, logits):
    s, a = scores.astype(np.float64), logits.astype(np.float64)
    err = float(np.abs(s - T.sigmoid64(a)).max())
    print(f"  {what}: |score - sigmoid64(logit)| <= {err / T.U:.2f} u over logits {a.min():.3g} .. {a.max():.3g}")
    assert np.isfinite(s).all() and (s >= 0).all() and (s <= 1).all() and err <= 4 * T.U, what


def _sigmoid_sweep(what, run, set_bias, logit0):
    """Move a head's output bias so that sequence 0's logit is near 0, +-20 and beyond +-90: ``run() -> scores, logits``."""
    seen = []
    for target in (0.0, 20.0, -20.0, 95.0, -95.0, 300.0, -300.0):
        set_bias(target - logit0)
        scores, logits = run(True)
        _sigmoid_ok(f"{what} target {target}", scores, logits)
        assert abs(float(logits[0]) - target) < 0.5
        seen.append(float(logits[0]))
        only, none = run(False)
        assert none is None and only.tobytes() == scores.tobytes(), "logits = NULL changes the scores"
    assert min(seen) < -90 and max(seen) > 90


# ---- tt_decoder_score ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtname", ["bf16", "f16"])
@pytest.mark.parametrize("H", T.H_ROW)
def test_decoder_score_matches_fp64(dev, built_lib, H, dtname):
    lib = _lib()
    fn = getattr(lib, "tt_decoder_score" + SUFFIX[dtname])
    for pad in (0, 8):
        c = T.score_case(H, dtname, pad, 200 + H)
        hidden_d, w_d = c.hidden.to(dev), c.w.to(dev)
        for n in T.N_SEQ:
            scores = torch.full((n + 3,), FILL, device=dev)
            logits = torch.full((n + 3,), FILL, device=dev)
            assert fn(hidden_d.data_ptr(), c.ld, w_d.data_ptr(), n, H, scores.data_ptr(), logits.data_ptr(), _stream(dev)) == 0, lib.tt_last_error()
            only = torch.full((n + 3,), FILL, device=dev)
            assert fn(hidden_d.data_ptr(), c.ld, w_d.data_ptr(), n, H, only.data_ptr(), None, _stream(dev)) == 0
            torch.cuda.synchronize()
            s, a = scores.cpu().numpy(), logits.cpu().numpy()
            _verdict(f"tt_decoder_score{SUFFIX[dtname]} H {H} ld H+{pad} n_seq {n}", c, a[:n], n)
            _sigmoid_ok("score head", s[:n], a[:n])
            assert (s[n:] == FILL).all() and (a[n:] == FILL).all() and only.cpu().numpy().tobytes() == s.tobytes()
        assert np.abs(a[:2]).max() < 0.1 and 10 < np.abs(a[2:4]).min() and np.abs(a[2:4]).max() < 40 and np.abs(a[4:8]).min() > 90


# ---- tt_rerank_head* -------------------------------------------------------------------------------------------------------------
def _enc_struct(Struct, H, keep, **head):
    p = keep["dummy"].data_ptr()
    return Struct(hidden=H, layers=0, heads=H // 64, ffn=4 * H, vocab=16, max_pos=16, type_vocab=1, ln_eps=1e-5, word_emb=p, pos_emb=p,
                  type_emb=p, emb_ln_g=p, emb_ln_b=p, **{k: v.data_ptr() for k, v in head.items()})


def _device_gemm(lib, dev, dtname):
    fn = getattr(lib, {"bf16": "tt_gemm_bf16", "f16": "tt_gemm_f16", "f32": "tt_gemm_f32"}[dtname])

    def gemm(a, w, bias, epilogue):
        a_d, w_d, b_d = a.to(dev), w.to(dev), bias.to(dev)
        c_d = torch.zeros(a.shape[0], w.shape[0], dtype=a.dtype, device=dev)
        rc = fn(a_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), None, c_d.data_ptr(), a.shape[0], w.shape[0], a.shape[1], epilogue, _stream(dev))
        assert rc == 0, lib.tt_last_error()
        torch.cuda.synchronize()
        return c_d.cpu()

    return gemm


def _rerank_setup(lib, dev, c, Struct=None, name=None):
    """Device operands of a rerank head call -> run(want_logits) -> (scores, logits | None, workspace bytes) as numpy."""
    from tensor_truth_amd.encoder import _EncW
    from tensor_truth_amd.encoder_f32 import _EncWF

    Struct = Struct or (_EncWF if c.dtname == "f32" else _EncW)
    name = name or "tt_rerank_head" + SUFFIX[c.dtname]
    keep = dict(dummy=torch.zeros(64, device=dev), hidden=c.hidden.to(dev), rows=_i32(c.rows, dev), wd=c.wd.to(dev), bd=c.bd.to(dev),
                wo=c.wo.to(dev), bo=c.bo.to(dev))
    w = _enc_struct(Struct, c.H, keep, cls_dense_w=keep["wd"], cls_dense_b=keep["bd"], cls_out_w=keep["wo"], cls_out_b=keep["bo"])
    guard = 4096

    def run(want_logits=True, ws_bytes=c.need):
        ws = torch.full((c.need + guard,), 0xA5, dtype=torch.uint8, device=dev)
        assert ws.data_ptr() % 256 == 0
        scores = torch.full((c.n_seq + 3,), FILL, device=dev)
        logits = torch.full((c.n_seq + 3,), FILL, device=dev)
        rc = getattr(lib, name)(ctypes.byref(w), keep["hidden"].data_ptr(), keep["rows"].data_ptr(), c.n_seq, scores.data_ptr(),
                                logits.data_ptr() if want_logits else None, ws.data_ptr(), ws_bytes, _stream(dev))
        torch.cuda.synchronize()
        if ws_bytes < c.need:
            return rc, ws.cpu()
        assert rc == 0, (name, rc, lib.tt_last_error())
        s, a, ws = scores.cpu().numpy(), logits.cpu().numpy(), ws.cpu()
        assert (s[c.n_seq:] == FILL).all() and (a[c.n_seq:] == FILL).all(), "scores / logits past n_seq were written"
        assert (ws[c.need:] == 0xA5).all(), "the guard region behind the workspace was written"
        return s[:c.n_seq], a[:c.n_seq] if want_logits else None, ws

    return run, keep


@functools.lru_cache(maxsize=None)
def _rerank_run(H, dtname, n_seq):
    dev = torch.device("cuda:0")
    lib = _lib()
    c = T.rerank_case(H, dtname, n_seq, 300 + H + n_seq)
    run, _ = _rerank_setup(lib, dev, c)
    scores, logits, ws = run()
    tight = T.rerank_tight(c, _device_gemm(lib, dev, dtname))
    rc, untouched = run(ws_bytes=c.need - 1)
    assert rc != 0 and b"workspace" in lib.tt_last_error() and (untouched == 0xA5).all(), "a workspace one byte short must be refused"
    return c, scores, logits, ws, tight


@pytest.mark.parametrize("n_seq", T.N_SEQ_RERANK)
@pytest.mark.parametrize("dtname", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("H", T.H_HEAD)
def test_rerank_head_against_its_gemm(dev, built_lib, H, dtname, n_seq):
    """The head's logit within ``(H + 2) u (sum |t_o w_o| + |b|)`` of the fp64 dot product of the exported GEMM's own t (epilogue 3,
    m = n_pad, over rows gathered and zero-padded on the host) with w: the gather, the padding, the workspace layout and
    head_out_kernel.  The workspace holds the gathered rows and that t, bit for bit; nothing behind ``need`` bytes is written."""
    c, scores, logits, ws, tight = _rerank_run(H, dtname, n_seq)
    _verdict(f"tt_rerank_head{SUFFIX[dtname]} against its GEMM, H {H} n_seq {n_seq}", tight, logits)
    _sigmoid_ok("rerank head", scores, logits)
    half = c.need // 2
    used = c.n_pad * H * c.hidden.element_size()
    assert ws[:used].numpy().tobytes() == c.a.contiguous().view(torch.uint8).numpy().tobytes(), "workspace: the gathered, zero-padded rows"
    assert ws[half:half + used].numpy().tobytes() == tight.t.contiguous().view(torch.uint8).numpy().tobytes(), "workspace: the GEMM's output"


@pytest.mark.parametrize("n_seq", T.N_SEQ_RERANK)
@pytest.mark.parametrize("dtname", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("H", T.H_HEAD)
def test_rerank_head_end_to_end(dev, built_lib, H, dtname, n_seq):
    """Against fp64 throughout: ``sum_o |w_o| tol(t64_o) + (H + 2) u (sum |t64_o w_o| + |b|)`` with the GEMM tests' own tolerance
    (``2^-7 |t| + 2e-3`` of test_gemm_epilogues; ``2e-6 sqrt(k / 32)`` of test_gemm_f32_building_block) and none of its own."""
    c, scores, logits, _, _ = _rerank_run(H, dtname, n_seq)
    _verdict(f"tt_rerank_head{SUFFIX[dtname]} end to end, H {H} n_seq {n_seq}", c, logits)


@pytest.mark.parametrize("H,n_seq", [(128, 129), (1024, 5)])
@pytest.mark.parametrize("name", ["tt_rerank_head_x3", "tt_rerank_head_x3_f16", "tt_rerank_head_f16c"])
def test_rerank_heads_that_delegate_give_the_fp32_heads_bits(dev, built_lib, name, H, n_seq):
    from tensor_truth_amd.encoder_f16c import _EncWC
    from tensor_truth_amd.encoder_x3 import _EncWX

    lib = _lib()
    c = T.rerank_case(H, "f32", n_seq, 300 + H + n_seq)
    want_s, want_a, _ = _rerank_setup(lib, dev, c)[0]()
    got_s, got_a, _ = _rerank_setup(lib, dev, c, Struct=_EncWC if name.endswith("f16c") else _EncWX, name=name)[0]()
    _verdict(f"{name} H {H} n_seq {n_seq}", c, got_a)
    assert got_a.tobytes() == want_a.tobytes() and got_s.tobytes() == want_s.tobytes(), f"{name} does not give tt_rerank_head_f32's bits"


@pytest.mark.parametrize("dtname", ["bf16", "f16", "f32"])
def test_rerank_head_sigmoid(dev, built_lib, dtname):
    lib = _lib()
    c = T.rerank_case(128, dtname, 5, 17)
    run, keep = _rerank_setup(lib, dev, c)
    _, base, _ = run()
    _sigmoid_sweep(f"tt_rerank_head{SUFFIX[dtname]}", lambda want: run(want)[:2], lambda v: keep["bo"].fill_(float(c.bo[0]) + v), float(base[0]))


# ---- tt_modernbert_head / tt_deberta_head ----------------------------------------------------------------------------------------
def _pooled_setup(lib, dev, c):
    """-> run(hidden, starts, lens, want_logits) -> (scores, logits | None) of a ModernBERT / DeBERTa head call."""
    keep = dict(dummy=torch.zeros(64, device=dev), wt=c.wt.to(dev), b=c.b.to(dev), gamma=c.gamma.to(dev), cw=c.cw.to(dev), cb=c.cb.to(dev))
    p = keep["dummy"].data_ptr()
    if c.model == "deberta":
        from tensor_truth_amd.deberta import _DbW
        from tensor_truth_amd.encoder import _EncW

        w = _DbW(enc=_EncW(hidden=c.H, layers=0, heads=c.H // 64, ffn=4 * c.H, vocab=16, max_pos=512, type_vocab=1, ln_eps=1e-7, word_emb=p,
                           emb_ln_g=p, emb_ln_b=p), dist_index=p, n_pos=512, max_pos=512, pooler_dense_wt=keep["wt"].data_ptr(),
                 pooler_dense_b=keep["b"].data_ptr(), cls_w=keep["cw"].data_ptr(), cls_b=keep["cb"].data_ptr())
    else:
        from tensor_truth_amd.modernbert import _MbW

        w = _MbW(hidden=c.H, layers=0, heads=c.H // 64, ffn=c.H, vocab=16, local_attention=128, norm_eps=T.NORM_EPS, global_rope_theta=160000.0,
                 local_rope_theta=10000.0, embed=p, emb_norm=p, final_norm=p, head_dense_wt=keep["wt"].data_ptr(),
                 head_norm=keep["gamma"].data_ptr(), cls_w=keep["cw"].data_ptr(), cls_b=keep["cb"].data_ptr())
    fn = getattr(lib, f"tt_{c.model}_head" + SUFFIX[c.dtname])

    def run(hidden, starts, lens, want_logits=True):
        n = len(starts)
        h_d, s_d, l_d = hidden.to(dev), _i32(starts, dev), _i32(lens, dev)
        scores = torch.full((n + 3,), FILL, device=dev)
        logits = torch.full((n + 3,), FILL, device=dev)
        rc = fn(ctypes.byref(w), h_d.data_ptr(), hidden.shape[1], s_d.data_ptr(), l_d.data_ptr(), n, c.pooling, scores.data_ptr(),
                logits.data_ptr() if want_logits else None, _stream(dev))
        assert rc == 0, (rc, lib.tt_last_error())
        torch.cuda.synchronize()
        s, a = scores.cpu().numpy(), logits.cpu().numpy()
        assert (s[n:] == FILL).all() and (a[n:] == FILL).all()
        return s[:n], a[:n] if want_logits else None

    return run, keep


@pytest.mark.parametrize("dtname", ["bf16", "f16"])
@pytest.mark.parametrize("H", T.H_HEAD)
@pytest.mark.parametrize("model,pooling", [("deberta", 0), ("modernbert", 0), ("modernbert", 1)])
def test_pooled_head_matches_fp64(dev, built_lib, model, pooling, H, dtname):
    """error / bound <= 1 under the first-order bound derived in ``tail_refs.pooled_head_case``'s docstring (pooled row, dense, GELU
    with Lipschitz constant 1.13 and erf within 16 ulp, ModernBERT's weight-only LayerNorm through rstd, the final dot)."""
    lib = _lib()
    c = T.pooled_head_case(model, H, dtname, pooling, 400 + H)
    run, keep = _pooled_setup(lib, dev, c)
    scores, logits = run(c.hidden, c.starts, c.lens)
    _verdict(f"tt_{model}_head{SUFFIX[dtname]} pooling {pooling} H {H}", c, logits)
    _sigmoid_ok(f"{model} head", scores, logits)
    for q in range(c.n):                                     # a sequence alone scores the bits it scores in the batch
        s, n = int(c.starts[q]), int(c.lens[q])
        h1 = torch.full((n + 9, c.ld), T.SENTINEL).to(c.hidden.dtype)
        h1[5:5 + n] = c.hidden[s:s + n]
        s1, a1 = run(h1, [5], [n])
        assert a1.tobytes() == logits[q:q + 1].tobytes() and s1.tobytes() == scores[q:q + 1].tobytes(), f"sequence {q} alone scores other bits"
    if H == 128:
        cb0 = float(c.cb[0])
        _sigmoid_sweep(f"tt_{model}_head{SUFFIX[dtname]}", lambda want: run(c.hidden, c.starts, c.lens, want),
                       lambda v: keep["cb"].fill_(cb0 + v), float(logits[0]))
