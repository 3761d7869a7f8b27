"""fp64 references, bounds, deliberately wrong references and fp32 restatements of the kernels behind every user-visible number:
pooling + L2 normalisation (first token, mean, last token) and the classification heads.  Shared by tests/test_tail_gpu.py (the
kernels) and tests/test_tail_refs_host.py (the restatements: the bounds are not too tight, the wrong references are outside them).

Operands are exactly representable in the operand type, references are fp64, ``U = 2^-24``.  A *case* is a namespace of inputs (CPU
torch tensors / numpy arrays), the fp64 result ``y64`` / ``logit64``, the elementwise ``bound`` and ``wrong``: named fp64 results
of the same operation done subtly wrong.  A wrong reference is *outside* the bound where it differs from the fp64 result by more
than twice the bound: nothing within the bound of the right answer is within the bound of the wrong one.

The bounds (first order in u; n terms summed in ANY order carry at most (n - 1) u of the sum of their magnitudes):

* first / last token + L2:  ``|y - y64| <= (H/2 + 8) u |y64|``: H rounded squares summed in any order give ``(H + 1) u`` on the sum
  of squares, the square root halves it, and the square root, the reciprocal, the product and the comparison's slack are the 8.
* mean + L2:  the fp32 mean of ``len`` rows summed in order and multiplied by the rounded ``1 / len`` carries
  ``e_i = (len + 1) u mean_t |x_ti|``; with ``m`` the fp64 mean, ``y = m / ||m||`` moves by at most
  ``(e_i + |m_i| ||e||_2 / ||m||) / ||m||``, and the normalisation adds the first bound.
* sigmoid:  ``|score - sigmoid64(logit_returned)| <= 4 u`` (one expf, one addition, one reciprocal on a value in [0, 1]).
* score head (no bias):  ``(H + 1) u sum |h_i w_i|``;  ``head_out``:  ``(H + 2) u (sum |t_o w_o| + |b|)``.
* the one-wave heads of ModernBERT and DeBERTa:  ``pooled_head_case``.

One wrong mean cannot be seen behind an L2 normalisation: a divisor of ``len + 1`` scales the mean and
leaves ``m / ||m||`` where it was (the clamp at 1e-12 aside).  tests/test_tail_refs_host.py asserts exactly that, and the divisor is
held outside the bound where it is visible: the mean-pooling mode of the ModernBERT head.
"""
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
SENTINEL = 3.0e4                          # padding columns and rows of no sequence (finite in bf16 and fp16)
H_ROW = [8, 384, 512, 520, 768, 1024]     # one active lane; no second chunk; exactly 64 chunks; only lane 0 has a second; serving
H_HEAD = [128, 384, 768, 1024]            # every width the heads' weight checks accept among these
N_SEQ = [1, 4, 5, 257]                    # four waves per workgroup: one wave, a full workgroup, one wave more, many workgroups
N_SEQ_RERANK = [1, 127, 128, 129]         # padded to multiples of 128 for the GEMM
MEAN_LENS = [1, 2, 63, 64, 65, 257]
CANCEL, EMPTY, ZEROS = 6, 7, 8            # sequences whose rows nearly cancel / that has no row / whose rows are all zero
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
F32 = np.float32


def f64(t):
    return t.double().numpy()


def ratio(got, ref, bound):
    """max |got - ref| / bound (inf where the bound is 0 and the value is not the reference)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def outside(wrong, ref, bound):
    """Number of elements on which a wrong reference is outside the bound."""
    return int((np.abs(wrong - ref) > 2 * bound).sum())


def teeth(case, names=None):
    """{name: elements outside the bound} over a case's wrong references."""
    ref = case.y64 if hasattr(case, "y64") else case.logit64
    return {k: outside(v, ref, case.bound) for k, v in case.wrong.items() if names is None or k in names}


def sigmoid64(x):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(x, dtype=np.float64)))


def sigmoid_f32(logit):
    """The kernels' ``1 / (1 + expf(-a))`` in fp32."""
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-np.asarray(logit, dtype=F32)))).astype(F32)


# ---- a wave's sum in fp32 ---------------------------------------------------------------------------------------------------------
def _lane_index(H, layout):
    """[64][per lane] element indices in the order a lane adds them; H (a zero column) where a lane has none."""
    if layout == "chunk8":                                   # lane l owns the 8-element chunks l, l + 64
        idx = np.full((64, 8 * ((H // 8 + 63) // 64)), H)
        for ch in range(H // 8):
            idx[ch % 64, 8 * (ch // 64):8 * (ch // 64) + 8] = np.arange(8 * ch, 8 * ch + 8)
    else:                                                    # "stride64": lane l owns the elements l, l + 64, ...
        idx = np.full((64, (H + 63) // 64), H)
        for e in range(H):
            idx[e % 64, e // 64] = e
    return idx


def wave_dot(a, b, layout, fused):
    """sum_i a_i b_i per row as a 64-lane wave computes it in fp32: each lane over its own elements in ascending order (the product
    rounded before the addition, or fused into it), then the xor butterfly 32, 16, .. 1."""
    a = np.atleast_2d(np.asarray(a, dtype=F32))
    b = np.broadcast_to(np.asarray(b, dtype=F32), a.shape)
    B, H = a.shape
    idx = _lane_index(H, layout)
    az, bz = (np.concatenate([v, np.zeros((B, 1), dtype=F32)], 1) for v in (a, b))
    acc = np.zeros((B, 64), dtype=F32)
    for j in range(idx.shape[1]):
        x, y = az[:, idx[:, j]], bz[:, idx[:, j]]
        acc = (x.astype(np.float64) * y + acc).astype(F32) if fused else (x * y + acc).astype(F32)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, np.arange(64) ^ off]).astype(F32)
    return acc[:, 0]


def l2_f32(x, layout, fused):
    """x / max(||x||, 1e-12) as the pooling kernels compute it."""
    x = np.asarray(x, dtype=F32)
    nrm = np.maximum(np.sqrt(wave_dot(x, x, layout, fused)), F32(1e-12)).astype(F32)
    return (x * (F32(1) / nrm)[:, None]).astype(F32)


# ---- pooling ---------------------------------------------------------------------------------------------------------------------
def _columns(h64, H, idx, variant):
    x = h64[idx, :H].copy()
    if variant == "padcol":                                  # the padding column in place of column 0
        x[:, 0] = h64[idx, H]
    elif variant == "lastchunk":                             # the last 8-element chunk dropped
        x[:, H - 8:] = 0
    elif variant == "chunk64":                               # the chunk that only lane 0 owns at H = 520
        x[:, 512:520] = 0
    return x


def _normalise(x):
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)


def pool_inputs(H, dtname, pad, seed, long=False):
    """A hidden-state buffer [n_rows][H + pad] with sequences packed at unaligned start rows with gaps of 0 .. 5 rows: the lengths
    MEAN_LENS, one whose rows nearly cancel, an empty one (at a start row > 0), one of all-zero rows, one of 8192 rows if ``long``,
    and short ones up to 257 (12 if ``long``) sequences.  Padding columns and rows of no sequence hold SENTINEL.  ``rows``: 257
    unsorted rows with repeats, the buffer's last row, row 0 and an all-zero row among the first five."""
    dt = DTYPES[dtname]
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    lens = MEAN_LENS + [40, 0, 3] + ([8192] if long else [])
    lens += [int(v) for v in rng.integers(1, 4, (12 if long else 257) - len(lens))]
    starts, row = [], 3
    for n in lens:
        starts.append(row)
        row += n + int(rng.integers(0, 6)) + (n == 8192)     # (a sentinel row behind the long sequence)
    n_rows, ld = row + 2, H + pad
    hidden = torch.full((n_rows, ld), SENTINEL).to(dt)
    for b, (s, n) in enumerate(zip(starts, lens)):
        x = torch.randn(n, H, generator=gen) + 0.25 * torch.randn(1, H, generator=gen)
        if b == CANCEL:                                      # 19 pairs (x, -x), then two small rows: the mean is ~1e-3 of mean |x|
            x[1:38:2] = -x[0:38:2]
            x[38:] *= 2.0 ** -6
        if b == ZEROS:
            x[:] = 0
        if n == 8192:                                        # one row in 8192 is visible only if it is a large one
            x[-1] *= 512.0
        hidden[s:s + n, :H] = x.to(dt)
    starts, lens = np.asarray(starts, dtype=np.int32), np.asarray(lens, dtype=np.int32)
    rows = rng.integers(0, n_rows, 257).astype(np.int32)
    rows[:5] = [starts[5] + 100, n_rows - 1, 0, starts[ZEROS], n_rows - 1]
    rows[200] = 0
    return SimpleNamespace(H=H, ld=ld, pad=pad, dtname=dtname, hidden=hidden, h64=f64(hidden), starts=starts, lens=lens, rows=rows,
                           n_rows=n_rows, n=len(lens))


def _row_case(x, sel, kind, wrong_rows, layout, fused):
    """First- / last-token pooling of the rows ``sel`` (-1: an empty sequence, the zero vector)."""
    H, h64 = x.H, x.h64
    live = (sel >= 0)[:, None]

    def ref(idx, variant=None):
        return _normalise(_columns(h64, H, np.clip(idx, 0, x.n_rows - 1), variant)) * (live if idx is sel else 1.0)

    y64 = ref(sel)
    wrong = {name: ref(idx) for name, idx in wrong_rows.items()}
    wrong["lastchunk"] = ref(sel, "lastchunk")
    if H == 520:
        wrong["chunk64"] = ref(sel, "chunk64")
    if x.pad:
        wrong["padcol"] = ref(sel, "padcol")

    def emulate():
        return l2_f32(h64[np.clip(sel, 0, None), :H] * live, layout, fused)

    return SimpleNamespace(x=x, kind=kind, sel=sel, y64=y64, bound=(H / 2 + 8) * U * np.abs(y64), wrong=wrong, emulate=emulate)


def cls_case(x, f32=False):
    """tt_embed_pool[_f16|_f32] over x.rows.  Wrong: the row before / behind the selected one (the row itself at the buffer's ends)."""
    return _row_case(x, x.rows.astype(np.int64), "cls", {"rowbefore": x.rows.astype(np.int64) - 1, "rowbehind": x.rows.astype(np.int64) + 1},
                     "stride64" if f32 else "chunk8", fused=f32)


def last_case(x):
    """tt_embed_pool_last[_f16].  Wrong: the last row skipped (the row before), one row past the sequence."""
    sel = np.where(x.lens > 0, x.starts.astype(np.int64) + x.lens - 1, -1)
    last = x.starts.astype(np.int64) + x.lens - 1
    return _row_case(x, sel, "last", {"skiplast": last - 1, "onepast": last + 1}, "chunk8", fused=True)


def mean_case(x):
    """tt_embed_pool_mean[_f16|_f32]."""
    H, h64 = x.H, x.h64

    def mean(rows_of, variant=None):
        out = np.zeros((x.n, H))
        for b, (s, n) in enumerate(zip(x.starts.tolist(), x.lens.tolist())):
            idx = rows_of(s, n)
            if len(idx):
                out[b] = _columns(h64, H, idx, variant).sum(0) / max(n, 1)
        return out

    exact = lambda s, n: np.arange(s, s + n)  # noqa: E731
    m = mean(exact)
    y64 = _normalise(m)
    mass = np.zeros((x.n, H))
    for b, (s, n) in enumerate(zip(x.starts.tolist(), x.lens.tolist())):
        if n:
            mass[b] = np.abs(h64[s:s + n, :H]).mean(0)
    e = (x.lens[:, None] + 1) * U * mass
    nm = np.sqrt((m * m).sum(1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.where(nm > 0, (e + np.abs(m) * np.sqrt((e * e).sum(1, keepdims=True)) / nm) / nm, 0.0)
    bound = first + (H / 2 + 8) * U * np.abs(y64)
    wrong = {"onepast": _normalise(mean(lambda s, n: np.arange(s, s + n + 1))),
             "skiplast": _normalise(mean(lambda s, n: np.arange(s, s + max(n - 1, 0)))),
             "lastchunk": _normalise(mean(exact, "lastchunk"))}
    if H == 520:
        wrong["chunk64"] = _normalise(mean(exact, "chunk64"))
    if x.pad:
        wrong["padcol"] = _normalise(mean(exact, "padcol"))
    invisible = _normalise(m * (x.lens / (x.lens + 1.0))[:, None])       # the divisor len + 1: the same unit vector

    def emulate():
        acc = np.zeros((x.n, H), dtype=F32)
        for t in range(int(x.lens.max())):                   # fp32 sums in the token order
            on = x.lens > t
            acc[on] = (acc[on] + h64[x.starts[on] + t, :H].astype(F32)).astype(F32)
        acc = (acc * (F32(1) / np.maximum(x.lens, 1).astype(F32))[:, None]).astype(F32)
        return l2_f32(acc, "chunk8", fused=False)

    return SimpleNamespace(x=x, kind="mean", y64=y64, bound=bound, wrong=wrong, invisible=invisible, emulate=emulate)


# ---- tt_decoder_score ------------------------------------------------------------------------------------------------------------
LOGIT_TARGETS = [0.02, -0.02, 20.0, -20.0, 95.0, -95.0, 190.0, -190.0]


def score_case(H, dtname, pad, seed, n=257):
    """hidden [n + 1][H + pad] (the last row is read by the wrong reference only), w fp32 [H].  The first rows are sign-aligned with w
    and scaled so that their logits are LOGIT_TARGETS up to the rounding of the row to its type."""
    dt = DTYPES[dtname]
    gen = torch.Generator().manual_seed(seed)
    hidden = torch.full((n + 1, H + pad), SENTINEL).to(dt)
    x = torch.randn(n + 1, H, generator=gen)
    w = torch.randn(H, generator=gen) * 0.1
    sgn = torch.sign(w) + (w == 0)
    k = min(len(LOGIT_TARGETS), n)
    x[:k] = x[:k].abs().clamp(0.25, 2.0) * sgn
    w = (w * (1.0 / float((x[0].double().abs() * w.double().abs()).sum()))).float()            # the aligned rows' logits: about 1
    for b in range(k):
        x[b] *= LOGIT_TARGETS[b] / float((x[b].double().abs() * w.double().abs()).sum())
    hidden[:, :H] = x.to(dt)
    h64, w64 = f64(hidden), f64(w)
    logit = lambda idx, hh=H: h64[idx, :hh] @ w64[:hh]  # noqa: E731
    rows = np.arange(n)
    logit64 = logit(rows)
    bound = (H + 1) * U * (np.abs(h64[:n, :H]) @ np.abs(w64))
    wrong = {"lastchunk": logit(rows, H - 8), "rownext": logit(rows + 1)}

    def emulate():
        return wave_dot(h64[:n, :H], w.numpy(), "chunk8", fused=True)

    return SimpleNamespace(H=H, ld=H + pad, n=n, hidden=hidden, w=w, logit64=logit64, bound=bound, wrong=wrong, emulate=emulate)


# ---- tt_rerank_head* -------------------------------------------------------------------------------------------------------------
EPI_BIAS, EPI_TANH = 0, 3                 # epilogues of tt_gemm_bf16 / tt_gemm_f16 / tt_gemm_f32


def rerank_gemm_tolerance(dtname, H, t64):
    """|t - t64| of the dense + tanh GEMM, from the GEMM's own tests: test_gemm_epilogues (16-bit) and test_gemm_f32_building_block
    (``2e-6 max(max |t64|, 1) sqrt(k / 32)``, and |tanh| <= 1)."""
    if dtname == "f32":
        return np.full_like(t64, 2e-6 * (H / 32) ** 0.5)
    return 2.0 ** -7 * np.abs(t64) + 2e-3


def rerank_case(H, dtname, n_seq, seed):
    """hidden [n_rows][H]; rows [n_seq] unsorted with repeats, the buffer's last row and row 0 first.  The dense bias is aligned with
    the signs of the output weights and the output bias is 5 % of sum |w|: dropping either, or the tanh, moves every logit the same
    way, by far more than the GEMM's tolerance."""
    dt = DTYPES[dtname]
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    n_rows = 150
    hidden = torch.randn(n_rows, H, generator=gen).to(dt)
    rows = rng.integers(0, n_rows, n_seq).astype(np.int32)
    rows[:3] = [n_rows - 1, 0, n_rows - 1][:n_seq]
    wd = (torch.randn(H, H, generator=gen) / H ** 0.5).to(dt)
    wo = torch.randn(H, generator=gen) * 0.05
    wo = (wo + 0.01 * torch.sign(wo)).to(dt)
    bd = (torch.sign(wo.float()) * (1.5 + torch.rand(H, generator=gen))).float()
    bo = torch.tensor([0.05 * float(wo.double().abs().sum())]).float()
    n_pad = (n_seq + 127) // 128 * 128
    a = torch.zeros(n_pad, H, dtype=dt)
    a[:n_seq] = hidden[rows.astype(np.int64)]
    a_next = torch.zeros(n_pad, H, dtype=dt)
    a_next[:n_seq] = hidden[(rows.astype(np.int64) + 1) % n_rows]
    wo64, bo64 = f64(wo), float(bo[0])
    pre = f64(a[:n_seq]) @ f64(wd).T + f64(bd)
    t64 = np.tanh(pre)
    logit64 = t64 @ wo64 + bo64
    head_term = lambda t: (H + 2) * U * (np.abs(t) @ np.abs(wo64) + abs(bo64))  # noqa: E731
    bound = rerank_gemm_tolerance(dtname, H, t64) @ np.abs(wo64) + head_term(t64)
    wrong = {"headbias": t64 @ wo64, "densebias": np.tanh(pre - f64(bd)) @ wo64 + bo64, "notanh": pre @ wo64 + bo64}
    c = SimpleNamespace(H=H, dtname=dtname, dt=dt, n_seq=n_seq, n_pad=n_pad, n_rows=n_rows, hidden=hidden, rows=rows, wd=wd, bd=bd, wo=wo,
                        bo=bo, a=a, a_next=a_next, logit64=logit64, bound=bound, wrong=wrong, head_term=head_term, wo64=wo64, bo64=bo64)
    c.need = 2 * ((n_pad * H * hidden.element_size() + 255) // 256 * 256)
    return c


def rerank_tight(c, gemm):
    """The head against the GEMM it runs: ``gemm(a, w, bias, epilogue) -> t`` (the exported building block on the device; a rounded
    fp64 product on the host) over the gathered, zero-padded rows.  -> the fp64 logits of that t, their bound, and the logits of the
    wrong heads: head bias dropped, dense bias dropped, W transposed, row rows[b] + 1, no tanh."""
    n, wo64, bo64 = c.n_seq, c.wo64, c.bo64
    dot = lambda t: f64(t[:n]) @ wo64  # noqa: E731
    t = gemm(c.a, c.wd, c.bd, EPI_TANH)
    ref = dot(t) + bo64
    wrong = {"headbias": dot(t),
             "densebias": dot(gemm(c.a, c.wd, torch.zeros_like(c.bd), EPI_TANH)) + bo64,
             "transposed": dot(gemm(c.a, c.wd.T.contiguous(), c.bd, EPI_TANH)) + bo64,
             "rownext": dot(gemm(c.a_next, c.wd, c.bd, EPI_TANH)) + bo64,
             "notanh": dot(gemm(c.a, c.wd, c.bd, EPI_BIAS)) + bo64}
    return SimpleNamespace(t=t, logit64=ref, bound=c.head_term(f64(t[:n])), wrong=wrong)


def host_gemm(a, w, bias, epilogue):
    """Stand-in for the device GEMM: the fp64 product rounded once to the operand type."""
    v = f64(a) @ f64(w).T + f64(bias)
    return torch.from_numpy(np.tanh(v) if epilogue == EPI_TANH else v).to(a.dtype)


def head_out_f32(c, t):
    """head_out_kernel (16-bit t and w, product rounded before the addition) / head_out_f32_kernel (fmaf, lane-strided) in fp32."""
    f32 = c.dtname == "f32"
    acc = wave_dot(f64(t[:c.n_seq]), f64(c.wo), "stride64" if f32 else "chunk8", fused=f32)
    return (acc + c.bo.numpy()[0]).astype(F32)


# ---- tt_modernbert_head / tt_deberta_head ----------------------------------------------------------------------------------------
POOLED_LENS = [1, 65, 300, 2, 1, 7]
GELU_LIPSCHITZ = 1.13
NORM_EPS = 1e-5


def _gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(torch.from_numpy(v / np.sqrt(2.0))).numpy())


def pooled_head_case(model, H, dtname, pooling, seed):
    """One wave per sequence, fp32 weights, the transposed dense matrix ``wt[i][o]`` walked in ascending i.

    The bound, first order in u, every sum taken over magnitudes (|.| of each term):

    * pooled row p: the first token is exact; the mean of n rows summed in order and multiplied by the rounded 1 / n carries
      ``e_p = (n + 1) u mean_t |x_t|``.
    * dense v_o = sum_i p_i wt[i][o] (+ b_o): ``e_v = (H + 1) u (sum_i |p_i wt_io| + |b_o|) + sum_i e_p,i |wt_io|``.
    * g = GELU(v) = 0.5 v (1 + erf(v / sqrt 2)): the input's error passes with the Lipschitz constant 1.13; erff within the OpenCL
      limit of 16 ulp of a value below 1 is ``16 u``, i.e. ``8 u |v|`` on g; the rounded argument moves erf by at most u / 2
      (``z erf'(z) <= 0.5``), the rounded ``1 + erf`` (< 2) by 2 u, together ``1.25 u |v|``; two products ``2 u |g| <= 2 u |v|``:
      ``e_g = 1.13 e_v + 12 u |v|``.
    * DeBERTa: ``e = sum_o e_g,o |c_o| + (H + 2) u (sum_o |g_o c_o| + |c_b|)``.
    * ModernBERT's weight-only LayerNorm, z_o = (g_o - mu) rstd gamma_o:  ``e_mu = mean e_g + (H + 1) u mean |g|``;
      d = g - mu: ``e_d = e_g + e_mu + u |d|``;  var = mean d^2: ``e_var = (2 / H) sum |d| e_d + (H + 2) u var``;
      rstd = (var + eps)^-1/2, relative: ``rho = e_var / (2 (var + eps)) + 4 u`` (the addition, the division by H, rsqrtf);
      term_o = d_o rstd gamma_o c_o: ``e_term = |gamma_o c_o| rstd (e_d + |d_o| rho) + 3 u |term_o|``;
      ``e = sum_o e_term + (H + 2) u (sum_o |term_o| + |c_b|)``.
    """
    dt = DTYPES[dtname]
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    pad = 8 if H in (128, 768) else 0
    lens = POOLED_LENS
    starts, row = [], 3
    for n in lens:
        starts.append(row)
        row += n + int(rng.integers(0, 4))
    n_rows = row + 2
    hidden = torch.full((n_rows, H + pad), SENTINEL).to(dt)
    hidden[:, :H] = torch.randn(n_rows, H, generator=gen).to(dt)       # rows of no sequence: plain values (a wrong row is a subtle error)
    hidden[:3, :H] = SENTINEL
    for s, n in zip(starts, lens):
        hidden[s:s + n, :H] = (0.5 + torch.randn(n, H, generator=gen) + 0.25 * torch.randn(1, H, generator=gen)).to(dt)
    hidden[:, H - 1] = 4.0
    # Two nested sums of H terms make the bound H^2 u of what the logit would be if all their terms had one sign: 6 % at H = 1024.
    # With terms of mixed signs nothing subtle is outside such a bound, so the sums are made (mostly) one-signed: the rows have a
    # mean of 0.5, a dense weight has the sign of the output weight c_o it feeds, and the logit is about sum |c_o| / 2 = 1.6.
    cw = (torch.randn(H, generator=gen) * (4.0 / H)).float()
    sgn = torch.sign(cw) + (cw == 0)
    # (ModernBERT's norm takes a common scale of the dense outputs out again: their sizes spread over a decade, so that GELU bends
    # them differently and a wrong scale of the pooled row -- the divisor n + 1, the last input dropped -- changes the logit)
    spread = torch.exp(2.4 * torch.rand(H, generator=gen) - 1.2)
    wt = torch.randn(H, H, generator=gen).abs() * (2.5 / H) * (sgn * spread)[None, :]
    wt[H - 1] = (20.0 / H) * sgn / spread                   # the last input (4 in every row) feeds the small outputs most
    wt = wt.float()
    b = (torch.randn(H, generator=gen) * 0.5).float() if model == "deberta" else torch.zeros(H)
    gamma = (1.0 + 0.2 * torch.randn(H, generator=gen)).float()
    cb = torch.tensor([0.3]).float()
    starts, lens = np.asarray(starts, dtype=np.int32), np.asarray(lens, dtype=np.int32)
    h64, wt64, b64, g64, cw64, cb64 = f64(hidden), f64(wt), f64(b), f64(gamma), f64(cw), float(cb.double()[0])
    B = len(lens)

    def forward(variant=None, want_bound=False):
        mean = bool(pooling) != (variant == "otherpool")
        p, e_p = np.zeros((B, H)), np.zeros((B, H))
        for q, (s, n) in enumerate(zip(starts.tolist(), lens.tolist())):
            if mean:
                p[q] = h64[s:s + n, :H].sum(0) / (n + 1 if variant == "divisor" else n)
                e_p[q] = (n + 1) * U * np.abs(h64[s:s + n, :H]).mean(0)
            else:
                p[q] = h64[s + int(variant == "secondtoken"), :H]
        w = wt64.T if variant == "nottransposed" else wt64
        if variant == "lastinput":
            p = p.copy()
            p[:, H - 1] = 0
        v = p @ w + (0 if variant == "nobias" else b64)
        g = _gelu64(v)
        keep = np.ones(H)
        if variant == "lastoutputs":
            keep[H - 64:] = 0
        if model == "deberta":
            terms = g * cw64 * keep
        else:
            mu = (g * keep).sum(1, keepdims=True) / H
            d = (g - mu) * keep
            var = (d * d).sum(1, keepdims=True) / H
            rstd = 1.0 / np.sqrt(var + NORM_EPS)
            terms = (g * keep if variant == "nonorm" else d * rstd * g64) * cw64
        logit = terms.sum(1) + cb64
        if not want_bound:
            return logit
        e_v = (H + 1) * U * (np.abs(p) @ np.abs(w) + np.abs(b64)) + e_p @ np.abs(w)
        e_g = GELU_LIPSCHITZ * e_v + 12 * U * np.abs(v)
        tail = (H + 2) * U * (np.abs(terms).sum(1) + abs(cb64))
        if model == "deberta":
            return logit, e_g @ np.abs(cw64) + tail
        e_mu = e_g.mean(1, keepdims=True) + (H + 1) * U * np.abs(g).mean(1, keepdims=True)
        e_d = e_g + e_mu + U * np.abs(d)
        e_var = 2.0 / H * (np.abs(d) * e_d).sum(1, keepdims=True) + (H + 2) * U * var
        rho = e_var / (2 * (var + NORM_EPS)) + 4 * U
        e_term = np.abs(g64 * cw64) * rstd * (e_d + np.abs(d) * rho) + 3 * U * np.abs(terms)
        return logit, e_term.sum(1) + tail

    logit64, bound = forward(want_bound=True)
    names = ["nottransposed", "secondtoken" if not pooling else None, "lastinput", "lastoutputs"]
    names += ["nobias"] if model == "deberta" else ["nonorm", "otherpool"] + (["divisor"] if pooling else [])
    wrong = {k: forward(k) for k in names if k}

    def emulate():
        p = np.zeros((B, H), dtype=F32)
        for q, (s, n) in enumerate(zip(starts.tolist(), lens.tolist())):
            if pooling:
                for t in range(n):
                    p[q] = (p[q] + h64[s + t, :H].astype(F32)).astype(F32)
                p[q] = (p[q] * (F32(1) / F32(n))).astype(F32)
            else:
                p[q] = h64[s, :H].astype(F32)
        y = np.zeros((B, H), dtype=F32)
        w32 = wt.numpy()
        for i in range(H):                                   # ascending inputs, fused
            y = (p[:, i:i + 1].astype(np.float64) * w32[i] + y).astype(F32)
        if model == "deberta":
            y = (y + b.numpy()).astype(F32)
        g = (F32(0.5) * y * (F32(1) + torch.erf(torch.from_numpy((y * F32(0.70710678118654752)).astype(F32))).numpy())).astype(F32)
        ones = np.ones((B, H), dtype=F32)
        if model == "deberta":
            dot = wave_dot(g, cw.numpy(), "stride64", fused=True)
        else:
            mu = (wave_dot(g, ones, "stride64", fused=False) / F32(H)).astype(F32)
            d = (g - mu[:, None]).astype(F32)
            var = wave_dot(d, d, "stride64", fused=True)
            rstd = (F32(1) / np.sqrt((var / F32(H) + F32(NORM_EPS)).astype(F32))).astype(F32)
            z = ((d * rstd[:, None]).astype(F32) * gamma.numpy()).astype(F32)
            dot = wave_dot(z, cw.numpy(), "stride64", fused=True)
        return (dot + cb.numpy()[0]).astype(F32)

    return SimpleNamespace(model=model, H=H, ld=H + pad, dtname=dtname, pooling=pooling, hidden=hidden, starts=starts, lens=lens, n=B, wt=wt,
                           b=b, gamma=gamma, cw=cw, cb=cb, logit64=logit64, bound=bound, wrong=wrong, emulate=emulate, n_rows=n_rows)
