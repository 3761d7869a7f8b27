"""GPU: the attention kernels of the reference precision and the CLS-only kernels, each against an fp64 softmax attention of
the values the kernel was given -- split planes: hi + lo; the 16-bit kernels: the bf16 / fp16 operands; f16c: the two fp16
Q / K planes and the fp16 V.  Building blocks: ``tt_attention_x3_hd[_f16]`` (full or CLS-only, 64- or 32-wide heads),
``tt_attention_cls_varlen[_f16]`` and ``tt_attention_f16c``.

Tolerances are derived per output element from the operands, never tuned.  With u = 2^-24 (fp32), S = scale Q.K^T the
scores, p the softmax, O = p.V the reference, a kernel's error is, to first order,

    |dO_id| <= sum_j p_ij dS_ij (|v_jd| + |O_id|)          a score error moves O by p_j dS_j (v_j - O)
             + e_p sum_j p_ij |v_jd| + a_p sqrt(sum_j v_jd^2) / l_i + e_p |O_id|
             + LAM u (sqrt(n_o n) sum_j p_ij |v_jd| + sqrt(n) |O_id|)
             + e_out |O_id| + a_out

    dS_ij = scale (D_ij + LAM u sqrt(sum_t s_t^2)) + 2 u (|S_ij| + max_j |S_ij|)

  * D: the product terms a kernel drops.  Split planes (x = hi + lo) drop lo.lo: D = sum_d |q_lo,d| |k_lo,d|, evaluated on the
    planes themselves (bf16 planes: |lo| <= 2^-8 |x|, i.e. D <= 2^-16 sum |q k|; fp16 planes: 2^-11, D <= 2^-22 sum |q k|).
    The one-query CLS kernels rebuild q and k in fp32 and drop nothing (+ LAM u sqrt(2 sum_d (q_d k_d)^2): the rebuild).
  * fp32 accumulation of a score: one rounding per product at the running sum s_t, in the kernel's order (split planes and
    f16c: the 2 dh lo cross terms, then hi.hi by ascending feature; the CLS kernels: their fma chain over the features).  The
    roundings as independent errors of at most u |s_t| (the model of Higham & Mary 2019) give, by Azuma-Hoeffding,
    LAM u sqrt(sum_t s_t^2) with LAM = 4.  sum_t s_t^2 is computed exactly for the hi.hi chain (a quadratic form in the
    operands: sum_{d,e} q_d q_e k_d k_e (dh - max(d, e))), the cross-term phase with |s_t| <= sum |cross terms|.
  * the value sum and the row sum: LAM u sqrt(n_o n) sum_j p_j |v_j| and LAM u sqrt(n) |O| (n_o = 3 products per key on the
    split planes, 1 elsewhere).  The 2 u (|S| + max |S|) term is the fp32 exponent argument S * scale * log2(e) - m.
  * e_p: the probabilities as the value product sees them.  Split planes P = P_hi + P_lo and the dropped V_lo.P_lo:
    2 * 2^-16 (bf16x3) or 2 * 2^-22 (f16x3); f16c rounds P to one fp16: 2^-11; fp32 everywhere else; + 2 u for v_exp_f32.
    a_p: fp16 probabilities below 2^-14 round on an absolute grid of 2^-24 (independent errors: LAM 2^-25 per key, RMS).
  * e_out: the output's format.  bf16x3 planes 2^-16, f16x3 planes 2^-22 (+ a_out 2^-25: a residual below 2^-14 lands on the
    lo plane's subnormal grid of 2^-24), bf16 2^-8, fp16 2^-11 (+ a_out 2^-25 for fp16 subnormals), f16c c-planes hi + lo8: 2^-11 * 2^-4 = 2^-15 (+ a_out 2^-28 of the 32-element block's maximum); + 2 u for
    the normalisation.

So f16x3's bound is bf16x3's with every plane term 2^-6 as large: what is left is the fp32 floor, near 1e-5 per element
against bf16x3's 6e-5.  Every bound has a teeth check on the host: the fp64 reference recomputed with a plausible defect
(Q's lo plane dropped, V's lo plane dropped, the last key of every sequence masked off, 1/8 as the scale of 32-wide heads,
the key frame shifted by one row; for f16x3 also every operand at bf16x3's 16 bits) must differ from the kernel's output by
more than the bound somewhere.  The CLS tests put a key of logit ~12 at every sequence's last position, so that a masked
last key or a shifted key frame shows at any length, 8192 included.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LAM = 4.0

# length sets: test_x3_gpu.py's, [1], 16 j +- 1, one sequence of 8192, a mix with 2049, back-to-back packing.  "alt": every
# other sequence follows its neighbour without a gap (start rows off the 8-row grid); "tight": every sequence does.
LENS = {
    "292x7": ([292] * 7, "alt"),
    "ragged": ([1, 8, 64, 65, 127, 128, 129, 300, 17, 33], "alt"),
    "512_31_257": ([512, 31, 257], "alt"),
    "mix2049": ([1100, 40, 2049], "alt"),
    "one": ([1], "alt"),
    "16j_pm1": ([15, 17, 31, 33, 63, 65, 127, 129, 255, 257, 511, 513], "tight"),
    "tight": ([5, 13, 7, 100, 9, 3, 250, 1, 66, 130, 2], "tight"),
    "8192": ([8192], "alt"),
    "8192_unaligned": ([5, 8192, 3], "tight"),
}
# (heads, head_dim): 64-wide heads at two hidden sizes (bge-m3's 16 x 64), 32-wide ones at 384 = 12 x 32 (bge-small) and 64
HEADS = [(4, 64), (16, 64), (12, 32), (2, 32)]
PLANES = {"bf16x3": torch.bfloat16, "f16x3": torch.float16}
# what each kernel drops / rounds (module docstring): plane unit roundoff of the split planes' P, output format
EPS = {
    "bf16x3": dict(p=2 * 2.0 ** -16 + 2 * U, p_abs=0.0, out=2.0 ** -16 + 2 * U, out_abs=0.0, n_o=3),
    "f16x3": dict(p=2 * 2.0 ** -22 + 2 * U, p_abs=2.0 ** -25, out=2.0 ** -22 + 2 * U, out_abs=2.0 ** -25, n_o=3),
    "cls_bf16x3": dict(p=3 * U, p_abs=0.0, out=2.0 ** -16 + 2 * U, out_abs=0.0, n_o=1, rebuild=True),
    "cls_f16x3": dict(p=3 * U, p_abs=0.0, out=2.0 ** -22 + 2 * U, out_abs=2.0 ** -25, n_o=1, rebuild=True),
    "cls_bf16": dict(p=2 * U, p_abs=0.0, out=2.0 ** -8 + 2 * U, out_abs=0.0, n_o=1),
    "cls_f16": dict(p=2 * U, p_abs=0.0, out=2.0 ** -11 + 2 * U, out_abs=2.0 ** -25, n_o=1),
    "f16c": dict(p=2.0 ** -11 + 2 * U, p_abs=2.0 ** -25, out=2.0 ** -15 + 2 * U, out_abs=0.0, blk_abs=2.0 ** -28, n_o=1),
}
_W = {dh: (dh - torch.maximum(torch.arange(dh).unsqueeze(0), torch.arange(dh).unsqueeze(1))).float() for dh in (32, 64)}
BF16X3_ACCURACY = "operands at bf16x3 precision"
CLS_LDS_LIMIT = 40953     # largest max_len whose score buffer, (max_len + 14) / 8 * 8 floats, fits 160 KiB (attention.hip)


def _lib_and_stream(dev):
    from tensor_truth_amd import _lib

    return _lib, _lib.load_library(), torch.cuda.current_stream(dev).cuda_stream


def _pack(lens, mode):
    starts, row = [], 0
    for i, n in enumerate(lens):
        starts.append(row)
        row += n if (mode == "tight" or i % 2) else (n + 7) // 8 * 8
    return starts, (row + 255) // 256 * 256


def _split(x, dt):
    from tensor_truth_amd.encoder_x3 import split_planes

    p = split_planes(x, dt)
    c = x.shape[1]
    return p[:, :c], p[:, c:]


def _v8(x):                                          # [T][H] -> the V8 layout [T/8][H][8]
    T, H = x.shape
    return x.reshape(T // 8, 8, H).permute(0, 2, 1).contiguous()


def _data(dev, T, H, seed, qk_std=1.5):
    g = torch.Generator(device=dev).manual_seed(seed)
    return tuple(torch.randn(T, H, generator=g, device=dev) * s for s in (qk_std, qk_std, 1.0))


def _spike(q, k, starts, lens, heads, dh, where):
    """Logits of ~100 (tests/stress_weights.py: trained heads reach tens to a hundred), as test_attention_running_maximum_under_
    spiked_logits places them: keys along the sequence's mean query direction d, every query given a component 6 d.  "early" /
    "late": one key at +100; "every_tile": one per 64-key tile, rising from +40 to +100 (the reference moves every tile);
    "creep": one per tile from +95 rising by 0.5 (below the lazy reference's 2^8 slack: it never moves, p grows to 2^8)."""
    scale = 1.0 / math.sqrt(dh)
    H = heads * dh
    spiked = torch.zeros(q.shape[0], dtype=torch.bool, device=q.device)
    for s0, n in zip(starts, lens):
        d = torch.nn.functional.normalize(q[s0:s0 + n].view(n, heads, dh).mean(0), dim=-1).reshape(H)
        q[s0:s0 + n] += 6.0 * d
        spots = {"late": [n - 3], "early": [1], "every_tile": list(range(5, n, 64)), "creep": list(range(5, n, 64)),
                 "last": [n - 1]}[where]
        spots = [pos for pos in spots if 0 < pos < n]
        for j, pos in enumerate(spots):
            if where == "every_tile":
                logit = 40.0 + 60.0 * j / max(1, len(spots) - 1)
            elif where == "creep":
                logit = 95.0 + 0.5 * j
            elif where == "last":
                logit = 12.0
            else:
                logit = 100.0
            k[s0 + pos] = logit / (6.0 * scale) * d
            spiked[s0 + pos] = True
    return q, k, spiked


def _reference(q, k, v, starts, lens, heads, dh, eps, *, cls=False, q_lo=None, k_lo=None, scale=None, key_drop=None, shift=0,
               key_mask=None, want_bound=True):
    """fp64 attention of (q, k, v) [T][H] per sequence and head -> (O, bound), rows = the sequences' rows in order (cls: one
    per sequence).  q_lo / k_lo: the lo planes of a split-plane kernel (its dropped lo.lo terms); key_drop: keys excluded per
    sequence (counted from its end); shift: the key frame moved by that many rows; key_mask: key rows excluded (defects)."""
    scale = 1.0 / math.sqrt(dh) if scale is None else scale
    outs, bounds = [], []
    for s0, n in zip(starts, lens):
        ks, kn = s0 + shift, n - (key_drop or 0)
        if kn <= 0 or ks < 0:
            ks, kn = s0, n                              # (a defect that does not apply to this sequence)
        nq = 1 if cls else n
        K = k[ks:ks + kn].double().view(kn, heads, dh).transpose(0, 1)
        V = v[ks:ks + kn].double().view(kn, heads, dh).transpose(0, 1)
        Vabs, V2 = V.abs(), V.pow(2).sum(1, keepdim=True).sqrt()            # [h, kn, dh], [h, 1, dh]
        Klo = None if k_lo is None else k_lo[ks:ks + kn].double().view(kn, heads, dh).transpose(0, 1)
        Khi = K if Klo is None else K - Klo
        if want_bound:
            Y = (Khi.unsqueeze(-1) * Khi.unsqueeze(-2)).reshape(heads, kn, dh * dh).float()
            KW = (Khi * (dh - torch.arange(dh, device=K.device, dtype=K.dtype))).float()
        step = max(1, (1 << 25) // (heads * kn))
        for c0 in range(0, nq, step):
            c1 = min(nq, c0 + step)
            Q = q[s0 + c0:s0 + c1].double().view(c1 - c0, heads, dh).transpose(0, 1)
            S = (Q @ K.transpose(1, 2)) * scale
            if key_mask is not None:
                S = S.masked_fill(key_mask[ks:ks + kn], -math.inf)
            P = torch.softmax(S, dim=-1)
            O = P @ V
            if not want_bound:                             # (a defect: only O is wanted)
                outs.append(O.transpose(0, 1).reshape(c1 - c0, heads * dh))
                bounds.append(O.transpose(0, 1).reshape(c1 - c0, heads * dh))
                continue
            # fp32 accumulation: one rounding per product at the running sum, products in the kernel's order (lo cross terms,
            # then hi.hi by ascending feature); independent roundings -> LAM u sqrt(sum_t s_t^2) (Azuma-Hoeffding)
            Qhi = Q
            c_sm = c_abs = 0.0
            if q_lo is not None:
                Qlo = q_lo[s0 + c0:s0 + c1].double().view(c1 - c0, heads, dh).transpose(0, 1)
                Qhi = Q - Qlo
                D = Qlo.abs() @ Klo.abs().transpose(1, 2)                             # the dropped lo.lo terms
                c_sm = Qlo @ Khi.transpose(1, 2) + Qhi @ Klo.transpose(1, 2)          # what the cross terms add up to
                c_abs = Qlo.abs() @ Khi.abs().transpose(1, 2) + Qhi.abs() @ Klo.abs().transpose(1, 2)
            X = (Qhi.unsqueeze(-1) * Qhi.unsqueeze(-2)).float() * _W[dh].to(Q.device)
            sum_p2 = (X.reshape(heads, c1 - c0, dh * dh) @ Y.transpose(1, 2)).double().clamp_min(0.0)   # sum_t P_t^2 of hi.hi
            sum_p = (Qhi.float() @ KW.transpose(1, 2)).double()                                          # sum_t P_t
            s2 = sum_p2 + 2 * c_sm * sum_p + dh * c_sm * c_sm + 2 * dh * c_abs * c_abs                  # + the cross-term phase
            dS = LAM * U * s2.clamp_min(0.0).sqrt() * scale
            if q_lo is not None:
                dS = dS + D * scale
            if eps.get("rebuild"):   # q, k rebuilt from their planes in fp32: one rounding each
                dS = dS + LAM * U * (2 * (Q * Q) @ (K * K).transpose(1, 2)).sqrt() * scale
            Sa = S.abs()
            dS = dS + 2 * U * (Sa + Sa.amax(-1, keepdim=True))
            dS = dS * (1.0 + dS.amax())                    # (second order)
            PW = P * dS
            Oa = O.abs()
            PV = P @ Vabs
            l_inv = torch.exp(S.amax(-1, keepdim=True) - torch.logsumexp(S, -1, keepdim=True))    # 1 / l with max p = 1
            b = (PW @ Vabs + Oa * PW.sum(-1, keepdim=True)
                 + eps["p"] * (PV + Oa) + LAM * eps["p_abs"] * V2 * l_inv
                 + LAM * U * (math.sqrt(eps["n_o"] * kn) * PV + math.sqrt(kn) * Oa)
                 + eps["out"] * Oa + eps["out_abs"])
            if "blk_abs" in eps:
                b = b + eps["blk_abs"] * Oa.view(heads, c1 - c0, dh // 32, 32).amax(-1, keepdim=True).expand(-1, -1, -1, 32).reshape(Oa.shape)
            outs.append(O.transpose(0, 1).reshape(c1 - c0, heads * dh))
            bounds.append(b.transpose(0, 1).reshape(c1 - c0, heads * dh))
    return torch.cat(outs), torch.cat(bounds)


def _ref_o(*args, **kw):
    return _reference(*args, want_bound=False, **kw)[0]


def _rows(x, starts, lens, cls):
    """the kernel's output rows in _reference's order (full: every sequence's rows; the CLS kernels write row b = sequence b)"""
    if cls:
        return x[: len(lens)]
    return torch.cat([x[s:s + n] for s, n in zip(starts, lens)])


def _check(got, want, bound, what):
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    ratio = ((got - want).abs() / bound).max().item()
    assert ratio <= 1.0, f"{what}: error {ratio:.3g} x its bound (max abs error {(got - want).abs().max().item():.3g})"
    return ratio


def _teeth(got, bound, defects, what):
    """each defect's fp64 reference must sit outside the bound somewhere: the bound would catch that bug"""
    for name, want_bad in defects.items():
        worst = ((got - want_bad).abs() / bound).max().item()
        assert worst > 1.0, f"{what}: the bound does not separate the kernel from the defect '{name}' ({worst:.3g})"


# ---- split planes: full attention and CLS-only (tt_attention_x3_hd[_f16]) ----------------------------------------------------
def _run_x3(dev, planes, heads, dh, lens, mode, cls, seed, spike=None):
    _lib, lib, st = _lib_and_stream(dev)
    dt = PLANES[planes]
    H = heads * dh
    starts, T = _pack(lens, mode)
    q, k, v = _data(dev, T, H, seed)
    spiked = None
    if spike:
        q, k, spiked = _spike(q, k, starts, lens, heads, dh, spike)
    (qh, ql), (kh, kl), (vh, vl) = _split(q, dt), _split(k, dt), _split(v, dt)
    qk = torch.cat([qh, kh, ql, kl], dim=1).contiguous()                  # Q hi | K hi | Q lo | K lo
    rows_out = len(lens) if cls else T
    out = torch.zeros((rows_out, 2 * H), dtype=dt, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    vth, vtl = _v8(vh), _v8(vl)                                           # (held: the kernel reads them after the call returns)
    fn = lib.tt_attention_x3_hd if planes == "bf16x3" else lib.tt_attention_x3_hd_f16
    rc = fn(qk.data_ptr(), 4 * H, 0, H, 2 * H, vth.data_ptr(), vtl.data_ptr(), 8 * H, out.data_ptr(), 2 * H, H,
            ss.data_ptr(), sl.data_ptr(), len(lens), heads, max(lens), dh, int(cls), st)
    _lib.check(rc, "tt_attention_x3_hd")
    torch.cuda.synchronize()
    got = _rows(out[:, :H].double() + out[:, H:].double(), starts, lens, cls)
    q64, k64, v64 = qh.double() + ql.double(), kh.double() + kl.double(), vh.double() + vl.double()
    eps = EPS[("cls_" if cls else "") + planes]
    lo = {} if cls else dict(q_lo=ql, k_lo=kl)
    want, bound = _reference(q64, k64, v64, starts, lens, heads, dh, eps, cls=cls, **lo)
    what = f"{planes} {'cls' if cls else 'full'} {heads}x{dh} {lens[:4]}"
    _check(got, want, bound, what)
    if not cls:
        used = torch.zeros(T, dtype=torch.bool, device=dev)
        for s, n in zip(starts, lens):
            used[s:s + n] = True
        assert not out[~used].any(), "rows of no sequence are written"
    defects = {"V lo plane dropped": _ref_o(q64, k64, vh.double(), starts, lens, heads, dh, eps, cls=cls, **lo)}
    if max(lens) > 1:        # (one key: p = 1 whatever the scores)
        defects["Q lo plane dropped"] = _ref_o(qh.double(), k64, v64, starts, lens, heads, dh, eps, cls=cls, **lo)
        defects["last key masked"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, cls=cls, key_drop=1, **lo)
    if dh == 32 and max(lens) > 1:
        defects["scale 1/8"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, cls=cls, scale=0.125, **lo)
    if cls and max(lens) > 1 and max(starts) > 0:          # (a sequence at row 0 has no row before it)
        defects["key frame one row early"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, cls=True, shift=-1)
    if planes == "f16x3":    # a kernel that carries its operands to 16 bits (bf16x3's accuracy) instead of 22
        j16 = [(h.double() + l.double()) for h, l in (_split(x, torch.bfloat16) for x in (q, k, v))]
        defects[BF16X3_ACCURACY] = _ref_o(*j16, starts, lens, heads, dh, eps, cls=cls)
    if spike:
        defects["spike keys masked"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, cls=cls, key_mask=spiked)
    return got, bound, defects, what


@pytest.mark.parametrize("lens_id", list(LENS))
@pytest.mark.parametrize("heads,dh", HEADS, ids=[f"{h}x{d}" for h, d in HEADS])
@pytest.mark.parametrize("planes", list(PLANES))
def test_attention_x3_full_against_fp64(dev, built_lib, planes, heads, dh, lens_id):
    lens, mode = LENS[lens_id]
    got, bound, defects, what = _run_x3(dev, planes, heads, dh, lens, mode, False, seed=sum(lens) + heads)
    if lens_id in ("ragged", "tight", "16j_pm1"):          # (short sequences: every defect is visible)
        _teeth(got, bound, defects, what)
    else:                    # (long ones average a 16-bit operand's score errors below the fp32 floor of the value sum)
        _teeth(got, bound, {k: w for k, w in defects.items() if k not in ("last key masked", BF16X3_ACCURACY)}, what)


@pytest.mark.parametrize("lens_id", list(LENS))
@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("planes", list(PLANES))
def test_attention_x3_cls_against_fp64(dev, built_lib, planes, dh, lens_id):
    lens, mode = LENS[lens_id]
    heads = 16 if dh == 64 else 12
    # (a key of logit ~12 at every sequence's last position: a masked last key or a shifted key frame shows at any length)
    got, bound, defects, what = _run_x3(dev, planes, heads, dh, lens, mode, True, seed=3 * sum(lens) + dh, spike="last")
    skip = ("spike keys masked",) if lens_id in ("ragged", "tight") else ("spike keys masked", BF16X3_ACCURACY)
    _teeth(got, bound, {k: w for k, w in defects.items() if k not in skip}, what)


# ---- the 16-bit CLS kernels (tt_attention_cls_varlen[_f16]) ------------------------------------------------------------------
def _run_cls16(dev, dt, heads, dh, lens, mode, seed, spike=None):
    _lib, lib, st = _lib_and_stream(dev)
    H = heads * dh
    starts, T = _pack(lens, mode)
    q, k, v = _data(dev, T, H, seed)
    spiked = None
    if spike:
        q, k, spiked = _spike(q, k, starts, lens, heads, dh, spike)
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    qk = torch.cat([q, k], dim=1).contiguous()
    out = torch.zeros((len(lens), H), dtype=dt, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    vt = _v8(v)
    fn = lib.tt_attention_cls_varlen if dt == torch.bfloat16 else lib.tt_attention_cls_varlen_f16
    rc = fn(qk.data_ptr(), 2 * H, 0, H, vt.data_ptr(), 8 * H, out.data_ptr(), H, ss.data_ptr(), sl.data_ptr(), len(lens),
            heads, dh, max(lens), st)
    _lib.check(rc, "tt_attention_cls_varlen")
    torch.cuda.synchronize()
    got = out.double()
    eps = EPS["cls_bf16" if dt == torch.bfloat16 else "cls_f16"]
    q64, k64, v64 = q.double(), k.double(), v.double()
    want, bound = _reference(q64, k64, v64, starts, lens, heads, dh, eps, cls=True)
    what = f"cls {dt} {heads}x{dh} {lens[:4]}"
    _check(got, want, bound, what)
    defects = {}
    if max(lens) > 1:
        defects["last key masked"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, cls=True, key_drop=1)
    if max(lens) > 1 and max(starts) > 0:
        defects["key frame one row early"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, cls=True, shift=-1)
    if dh == 32 and max(lens) > 1:
        defects["scale 1/8"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, cls=True, scale=0.125)
    if spike:
        defects["spike keys masked"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, cls=True, key_mask=spiked)
    return got, bound, defects, what


@pytest.mark.parametrize("lens_id", list(LENS))
@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_attention_cls_16bit_against_fp64(dev, built_lib, dt, dh, lens_id):
    lens, mode = LENS[lens_id]
    heads = 16 if dh == 64 else 12
    got, bound, defects, what = _run_cls16(dev, dt, heads, dh, lens, mode, seed=5 * sum(lens) + dh, spike="last")
    _teeth(got, bound, {k: w for k, w in defects.items() if k != "spike keys masked"}, what)


# ---- large logits --------------------------------------------------------------------------------------------------------
SPIKE_LENS = [292, 320, 64, 129, 700, 1]


@pytest.mark.parametrize("where", ["late", "early", "every_tile", "creep"])
@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("kernel", ["bf16x3", "f16x3", "cls_bf16x3", "cls_f16x3", "cls_bf16", "cls_fp16"])
def test_attention_large_logits_against_fp64(dev, built_lib, kernel, dh, where):
    heads = 4
    seed = 11 + dh + len(where)
    if kernel in ("cls_bf16", "cls_fp16"):
        dt = torch.bfloat16 if kernel == "cls_bf16" else torch.float16
        got, bound, defects, what = _run_cls16(dev, dt, heads, dh, SPIKE_LENS, "alt", seed, spike=where)
    else:
        cls = kernel.startswith("cls_")
        got, bound, defects, what = _run_x3(dev, kernel.replace("cls_", ""), heads, dh, SPIKE_LENS, "alt", cls, seed, spike=where)
    # (a softmax this peaked hides operand defects; a kernel that loses the spike -- a wrong mask, a lost running maximum -- shows)
    _teeth(got, bound, {"spike keys masked": defects["spike keys masked"]}, what)


# ---- f16c (tt_attention_f16c): two fp16 Q / K planes, fp16 V, c-planes out ------------------------------------------------
def _decode_c_planes(out, scales, rows, W):
    """c-planes [rows][4 W bytes] + tiled activation scales -> hi + lo8 (oracle/f16c.py's decoding)"""
    from oracle import f16c as of

    import numpy as np

    o = out.cpu()
    hi = o[:, : 2 * W].contiguous().view(torch.float16)
    x8 = o[:, 2 * W:3 * W].contiguous().view(torch.float8_e4m3fn)
    lo8 = o[:, 3 * W:].contiguous().view(torch.float8_e4m3fn)
    rr, bb = np.meshgrid(np.arange(rows), np.arange(W // 32), indexing="ij")
    s = torch.from_numpy(scales.cpu().numpy()[of.a_scale_at(rr, bb, W // 128)].astype(np.int32))
    h, _, l = of.dequant({"hi": hi, "x8": x8, "lo8": lo8, "s": s}, False)
    return h.double() + l.double()


@pytest.mark.parametrize("lens_id", list(LENS))
@pytest.mark.parametrize("heads", [4, 16])
def test_attention_f16c_against_fp64(dev, built_lib, heads, lens_id):
    _lib, lib, st = _lib_and_stream(dev)
    lens, mode = LENS[lens_id]
    dh = 64
    H = heads * dh
    starts, T = _pack(lens, mode)
    q, k, v = _data(dev, T, H, seed=7 * sum(lens) + heads)
    (qh, ql), (kh, kl) = _split(q, torch.float16), _split(k, torch.float16)
    vh = v.to(torch.float16)
    qk = torch.cat([qh, kh, ql, kl], dim=1).contiguous()
    out = torch.zeros((T, 4 * H), dtype=torch.uint8, device=dev)
    scales = torch.zeros(int(lib.tt_f16c_scale_bytes(T, H, 0)), dtype=torch.uint8, device=dev)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    vt = _v8(vh)
    rc = lib.tt_attention_f16c(qk.data_ptr(), 4 * H, 0, H, 2 * H, vt.data_ptr(), 8 * H, out.data_ptr(), scales.data_ptr(),
                               ss.data_ptr(), sl.data_ptr(), len(lens), heads, max(lens), st)
    _lib.check(rc, "tt_attention_f16c")
    torch.cuda.synchronize()
    got = _rows(_decode_c_planes(out, scales, T, H).to(dev), starts, lens, False)
    q64, k64, v64 = qh.double() + ql.double(), kh.double() + kl.double(), vh.double()
    eps = EPS["f16c"]
    want, bound = _reference(q64, k64, v64, starts, lens, heads, dh, eps, q_lo=ql, k_lo=kl)
    what = f"f16c {heads}x{dh} {lens[:4]}"
    _check(got, want, bound, what)
    defects = {}
    if max(lens) > 1:        # (one key: p = 1 whatever the scores; V is a single fp16 plane)
        defects["Q lo plane dropped"] = _ref_o(qh.double(), k64, v64, starts, lens, heads, dh, eps, q_lo=ql, k_lo=kl)
    if lens_id in ("ragged", "tight", "16j_pm1"):
        defects["last key masked"] = _ref_o(q64, k64, v64, starts, lens, heads, dh, eps, q_lo=ql, k_lo=kl, key_drop=1)
    _teeth(got, bound, defects, what)


# ---- argument checks: refused before anything is launched ----------------------------------------------------------------
def test_new_entries_refuse_bad_head_dim_and_a_max_len_past_the_cls_score_buffer(dev, built_lib):
    """head_dim other than 32 / 64, and for the CLS-only kernels a max_len one past the LDS score buffer of attention.hip's
    formula ((max_len + 14) / 8 * 8 floats <= 160 KiB: max_len 40953), come back as an error with a message; the largest
    accepted max_len runs (on short sequences: max_len only sizes the score buffer)."""
    _lib, lib, st = _lib_and_stream(dev)
    heads, dh = 2, 64
    H = heads * dh
    lens, starts, T = [3, 9], [0, 3], 256
    q, k, v = _data(dev, T, H, seed=1)
    ss = torch.tensor(starts, dtype=torch.int32, device=dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    for name, dt in (("", torch.bfloat16), ("_f16", torch.float16)):
        (qh, ql), (kh, kl), (vh, vl) = _split(q, dt), _split(k, dt), _split(v, dt)
        qk = torch.cat([qh, kh, ql, kl], dim=1).contiguous()
        vth, vtl = _v8(vh), _v8(vl)
        out = torch.zeros((T, 2 * H), dtype=dt, device=dev)
        x3 = getattr(lib, "tt_attention_x3_hd" + name)

        def call_x3(max_len, hd, cls):
            return x3(qk.data_ptr(), 4 * H, 0, H, 2 * H, vth.data_ptr(), vtl.data_ptr(), 8 * H, out.data_ptr(), 2 * H, H,
                      ss.data_ptr(), sl.data_ptr(), 2, heads, max_len, hd, cls, st)

        qk16 = torch.cat([qh, kh], dim=1).contiguous()
        c16 = getattr(lib, "tt_attention_cls_varlen" + name)

        def call_c16(max_len, hd):
            return c16(qk16.data_ptr(), 2 * H, 0, H, vth.data_ptr(), 8 * H, out.data_ptr(), H, ss.data_ptr(), sl.data_ptr(), 2,
                       heads, hd, max_len, st)

        for hd in (0, 16, 48, 128):
            for cls in (0, 1):
                assert call_x3(9, hd, cls) != 0 and b"head_dim" in lib.tt_last_error()
            assert call_c16(9, hd) != 0 and b"head_dim" in lib.tt_last_error()
        assert call_x3(CLS_LDS_LIMIT + 1, dh, 1) != 0 and b"LDS" in lib.tt_last_error()
        assert call_c16(CLS_LDS_LIMIT + 1, dh) != 0 and b"LDS" in lib.tt_last_error()
        assert call_x3(CLS_LDS_LIMIT + 1, dh, 0) == 0           # (the full kernel has no score buffer)
        _lib.check(call_x3(CLS_LDS_LIMIT, dh, 1), "tt_attention_x3_hd cls at the limit")
        _lib.check(call_c16(CLS_LDS_LIMIT, dh), "tt_attention_cls_varlen at the limit")
        torch.cuda.synchronize()
