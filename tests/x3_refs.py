"""References, operand families, deliberately wrong references, an fp32 restatement and the kernel-choice rule of the split-plane
GEMMs (gemm.hip ``GemmParams.x3``, launch_x3; x3_path.hip ``tt_gemm_x3_ex``): every matrix product of the default precision runs as
``a_hi w_hi + a_hi w_lo + a_lo w_hi`` on two 16-bit planes per operand, accumulated in fp32.  Shared by
tests/test_gemm_x3_edges_gpu.py (the kernels) and tests/test_x3_refs_host.py (the restatement, without a GPU).

Vocabulary and helpers are those of tests/tail_refs.py and tests/mid_refs.py (``U = 2^-24``, a *case* with ``y64``, ``bound`` and
``wrong``; ``ratio``, ``outside``).  ``planes`` is the planes' element type, "bf16" or "f16"; a *form* is what the epilogue writes:

=============  ==========  =====================================================================================================
form           epilogue    output
=============  ==========  =====================================================================================================
``planes``     0           v = acc + bias as planes, hi = type(v), lo = type(v - hi)
``gelu``       1           exact-erf GELU(v) as planes
``res32``      2           fp32 v + residual, the residual as fp32 rows
``resplanes``  2           fp32 v + (r_hi + r_lo), the residual rebuilt from its planes in fp32
``vt``         5           v as planes in the V8 layout, element (m, n) at [m / 8][n][m % 8], once per plane
=============  ==========  =====================================================================================================

**Why two kinds of family.**  The any-order bound ``(3K + 1) u sum |a w|`` grows with K while what a dropped lo plane costs does
not: at K = 1024 a kernel without A's lo plane is inside it on every element.  So large K is held bit for bit, on operands built
so that every partial sum of the three products is exact in fp32, and the fp64 bound is kept for K <= 128, where it bites.

* ``exact``: operands hi + lo with hi an integer (A: +-1, or 0 on whole columns; W: 1 <= |w| <= wmax) and ``lo = j q``, |j| <= 3,
  ``q = 2^-11`` (bf16 planes) / ``2^-14`` (fp16 planes: the smallest normal); bias and residual integers plus multiples of q.  The
  host split returns exactly these planes, and ``(sum |a_hi w_hi| + sum |a_hi w_lo| + sum |a_lo w_hi| + |bias| + |res|) / q < 2^24``
  on every element: all three products and every partial sum, in any order, are multiples of q below 2^24 q.  ``wmax`` shrinks
  and columns of A are zeroed with K to keep that; every 32-element K-step keeps a non-zero product in both lo planes.
* ``sublo`` (fp16 planes): ``a = +-2^-4 + j 2^-18`` on every second column, ``w = +-m 2^-4 + j 2^-18``: every lo element is an fp16
  SUBNORMAL, the products are multiples of ``2^-22``.  A matrix core that flushes subnormal inputs loses the lo plane of nearly
  every weight (|x| < 2^-3): this family shows whether it does.
* ``gauss`` (K <= 128): A ~ N(0, 1), W ~ N(0, 1 / K) in fp32, split on the host; fp64 on the planes' own values, all four
  products: ``ev = (3K + 1) u (mass3 + |bias|) + sum |a_lo| |w_lo|`` (3K products and the bias summed in any order; the term the
  kernels leave out), then per form
    - fp32 out:    ``ev + u |ref|`` (+ ``u |res|`` where hi + lo is rebuilt: 22 bits and a gap need not fit fp32's 24)
    - planes out:  ``e + U_OUT^2 |ref| + floor``: two roundings of U_OUT leave U_OUT^2; the floor is 2^-25 for fp16 planes (the lo
                   plane's subnormal grid of 2^-24) and 2^-126 for bf16
    - GELU:        ``e = 1.13 ev + 12 u |v|``: tail_refs.pooled_head_case's budget for 0.5 v (1 + erff(v / sqrt 2))
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import mid_refs as R
from mid_refs import F32, U, U_OUT, gelu64, outside, ratio, rne, sweep_values  # noqa: F401  (the tests take them from here)

PLANES = {"bf16": torch.bfloat16, "f16": torch.float16}
QUANTUM = {"bf16": 2.0 ** -11, "f16": 2.0 ** -14}
SUB_QUANTUM = 2.0 ** -22
FLOOR = {"bf16": 2.0 ** -126, "f16": 2.0 ** -25}
F16_MAX = 65504.0
FORMS = ["planes", "gelu", "res32", "resplanes", "vt"]
EPI = {"planes": 0, "gelu": 1, "res32": 2, "resplanes": 2, "vt": 5}
KSTEP = 32
MI355X_CUS = 256


# ---- which kernel launch_x3 picks -------------------------------------------------------------------------------------------------------
def x3_kernel(M, N, K, cus):
    """'relay' | 'staged' | 'tile256' | None (refused): launch_x3 in gemm.hip for planes [.][2K] (lda = ldw = 2K)."""
    if 0 < M <= 256 and M % 64 == 0 and N % 16 == 0 and K % 32 == 0:
        return "relay"
    if M <= 0 or M % 256 or N % 64 or K % 64 or K < 128:
        return None
    if N % 128 == 0 and (M // 128) * (N // 128) <= 2 * cus:
        return "staged"
    return "tile256"


# shapes for the 256 CUs of an MI355X: kernel -> [(M, N, K)], the smallest that take each branch
SHAPES = {"relay": [(64, 16, 32), (256, 48, 32),          # one step
                    (64, 48, 256), (256, 16, 256),        # exactly one turn of the eight waves
                    (64, 16, 288), (256, 48, 288),        # a second turn of one step
                    (64, 48, 2080), (256, 16, 2080)],     # a ninth turn: wave 0 refills
          "staged": [(512, 128, 128), (512, 128, 192), (512, 128, 320),     # ring depths
                     (512, 384, 128)],                                       # three column tiles
          "tile256": [(33024, 256, 128),                                      # full tiles: 516 tiles of 128^2 > 2 x CUs
                      (512, 64, 128), (512, 192, 128), (512, 320, 128),       # partial last tile: one, three, one of two's strips
                      (512, 448, 256),
                      (22016, 384, 128)]}                                     # partial last tile at bge-small's width: 516 tiles
PARAMS = [(k, s) for k, shapes in SHAPES.items() for s in shapes]
IDS = [f"{k}-{m}x{n}x{kk}" for k, (m, n, kk) in PARAMS]
SWEEP_SHAPES = {"relay": (64, 8192, 32), "staged": (512, 8192, 128), "tile256": (2304, 8192, 128)}
# one shape per kernel with the same N and K: a row's bits do not depend on the kernel
IDENTITY_ROWS = {"relay": 64, "staged": 512, "tile256": 33024}
IDENTITY_NK = (256, 128)


def families(planes, K):
    return ["exact"] + (["sublo"] if planes == "f16" else []) + (["gauss"] if K <= 128 else [])


# the cases both tests walk: (kernel, (M, N, K), planes, family)
CASES = [(k, s, pl, f) for k, s in PARAMS for pl in PLANES for f in families(pl, s[2])]
CASE_IDS = [f"{k}-{m}x{n}x{kk}-{pl}-{f}" for k, (m, n, kk), pl, f in CASES]


# ---- the host split -----------------------------------------------------------------------------------------------------------------------
def split(x, planes):
    """fp32-representable values -> (hi, lo) as fp64 arrays: ``encoder_x3.split_planes``, the split the weights get on load."""
    from tensor_truth_amd.encoder_x3 import split_planes

    with np.errstate(invalid="ignore"):                       # (a signalling NaN among the split kernels' values)
        x32 = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(F32))
        assert np.array_equal(x32.astype(np.float64), np.asarray(x, dtype=np.float64), equal_nan=True), "operands are fp32 values"
    two = x32.ndim == 2
    p = split_planes(torch.from_numpy(x32.reshape(-1, x32.shape[-1]) if two else x32.reshape(1, -1)), PLANES[planes])
    n = p.shape[1] // 2
    hi, lo = p[:, :n].double().numpy(), p[:, n:].double().numpy()
    return (hi, lo) if two else (hi.reshape(x32.shape), lo.reshape(x32.shape))


def planes_tensor(hi, lo, planes):
    """(hi, lo) exact in the type -> the planes [rows][2 cols] as a torch tensor of the type."""
    t = torch.from_numpy(np.concatenate([hi, lo], axis=1)).to(PLANES[planes])
    assert np.array_equal(t.double().numpy(), np.concatenate([hi, lo], axis=1))
    return t


def split_bits(v32, planes):
    """fp32 array [M][N] -> the host split as a torch tensor [M][2N] of the type: what a planes output must hold, bit for bit."""
    from tensor_truth_amd.encoder_x3 import split_planes

    return split_planes(torch.from_numpy(np.ascontiguousarray(v32, dtype=F32)), PLANES[planes])


def same_bits(got, want):
    """Equal bits, a NaN matching any NaN (its payload and sign are the converter's own)."""
    g, w = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    return bool(((g == w) | (got.isnan() & want.isnan())).all())


# ---- operands -----------------------------------------------------------------------------------------------------------------------------
def _thin(rng, K, per_step, candidates):
    """A column mask [K]: ``per_step`` of every K-step's candidate columns, chosen at random."""
    keep = np.zeros(K, dtype=bool)
    for s in range(0, K, KSTEP):
        c = s + candidates
        keep[rng.choice(c, size=min(per_step, len(c)), replace=False)] = True
    return keep


def _plan(K, budget, cap, candidates_per_step):
    """(largest |w_hi| in units, active columns per K-step) so that the worst row's sum of |a_hi w_hi| stays within ``budget`` units."""
    steps = K // KSTEP
    wmax = min(cap, budget // (steps * candidates_per_step))
    if wmax >= 1:
        return int(wmax), candidates_per_step
    return 1, max(1, budget // steps)


def operands(family, planes, M, N, K, seed):
    """-> namespace of fp64 arrays: the planes ah, al [M][K], wh, wl [N][K]; bias [N] (fp32 values); the residual's planes rh, rl
    [M][N] (res = rh + rl is an fp32 value); ``q``, the quantum of the exact families (None for gauss)."""
    rng = np.random.default_rng(seed)
    j = lambda *shape: rng.integers(-3, 4, shape).astype(np.float64)  # noqa: E731
    sign = lambda *shape: rng.choice([-1.0, 1.0], shape)  # noqa: E731
    if family == "exact":
        q = QUANTUM[planes]
        # 2^24 q = 8192 (bf16) / 1024 (fp16) in units of 1; |bias| <= 16.2 and |res| <= 16.2 and the lo terms (< 0.01 K) leave 0.9 of it
        wmax, per_step = _plan(K, int(0.9 * 2 ** 24 * q) - 48, 4, KSTEP)
        live = _thin(rng, K, per_step, np.arange(KSTEP))
        ah, al = sign(M, K) * live + 0.0, j(M, K) * q * live + 0.0          # (+ 0.0: no negative zeros)
        wh, wl = sign(N, K) * rng.integers(1, wmax + 1, (N, K)), j(N, K) * q + 0.0
        bias = sign(N) * rng.integers(1, 17, N) + j(N) * q
        rh, rl = sign(M, N) * rng.integers(1, 17, (M, N)), j(M, N) * q + 0.0
    elif family == "sublo":
        assert planes == "f16"
        q, h = SUB_QUANTUM, 2.0 ** -4
        # units of 2^-8 (= h h): 2^24 q = 4 = 1024 units; |bias| <= 2^-3 + and |res| <= 2^-1 + are 160 units
        mmax, per_step = _plan(K, int(0.9 * 1024) - 170, 8, KSTEP // 2)
        live = _thin(rng, K, per_step, np.arange(0, KSTEP, 2))
        ah, al = sign(M, K) * h * live + 0.0, j(M, K) * 2.0 ** -18 * live + 0.0
        wh, wl = sign(N, K) * rng.integers(1, mmax + 1, (N, K)) * h, j(N, K) * 2.0 ** -18 + 0.0
        bias = sign(N) * rng.integers(1, 9, N) * 2.0 ** -6 + j(N) * q
        rh, rl = sign(M, N) * rng.integers(1, 9, (M, N)) * h, j(M, N) * 2.0 ** -18 + 0.0
    else:
        q = None
        ah, al = split(rng.standard_normal((M, K)).astype(F32), planes)
        wh, wl = split((rng.standard_normal((N, K)) / np.sqrt(K)).astype(F32), planes)
        bias = (0.1 * rng.standard_normal(N)).astype(F32).astype(np.float64)
        rh, rl = split(rng.standard_normal((M, N)).astype(F32), planes)
    return SimpleNamespace(family=family, planes=planes, M=M, N=N, K=K, q=q, ah=ah, al=al, wh=wh, wl=wl, bias=bias, rh=rh, rl=rl)


def assert_exact_family(p):
    """The conditions of the module docstring on an exact family's operands -> the largest ratio (sum of magnitudes) / (2^24 q)."""
    for x, (hi, lo) in ((p.ah + p.al, (p.ah, p.al)), (p.wh + p.wl, (p.wh, p.wl)), (p.rh + p.rl, (p.rh, p.rl))):
        h, l = split(x, p.planes)
        assert np.array_equal(h, hi) and np.array_equal(l, lo), "the host split returns the planes the family was built from"
    if p.family == "sublo":
        assert (np.abs(p.al) < 2.0 ** -14).all() and (np.abs(p.wl) < 2.0 ** -14).all() and (np.abs(p.rl) < 2.0 ** -14).all()
        live = (p.ah != 0).any(0)
        assert (p.wl != 0).mean() > 0.8 and (p.al[:, live] != 0).mean() > 0.8, "the lo planes are fp16 subnormals, not zeros"
    mag = np.abs(p.ah) @ np.abs(p.wh).T + np.abs(p.ah) @ np.abs(p.wl).T + np.abs(p.al) @ np.abs(p.wh).T + np.abs(p.bias) + np.abs(p.rh) + np.abs(p.rl)
    r = float(mag.max() / p.q)
    assert r < 2 ** 24, f"partial sums are not all exact in fp32: {r:.3g} quanta"
    for x in (p.ah, p.al, p.wh, p.wl, p.bias, p.rh, p.rl):
        assert np.array_equal(np.rint(x / p.q) * p.q, x), "every operand is a multiple of the quantum"
    for s in range(0, p.K, KSTEP):
        ks = slice(s, s + KSTEP)
        assert (np.abs(p.ah[:, ks]).sum(0) * np.abs(p.wl[:, ks]).sum(0)).sum() > 0 and (np.abs(p.al[:, ks]).sum(0) * np.abs(p.wh[:, ks]).sum(0)).sum() > 0, \
            f"K-step {s // KSTEP} carries no product of a lo plane"
    return r


# ---- the three products, and their wrong forms ------------------------------------------------------------------------------------------
WRONG_PRODUCT = ["alo", "wlo", "lolo", "lostep", "lolast", "biascol", "striprow"]
WRONG = {"alo": "A's lo plane dropped", "wlo": "W's lo plane dropped", "lolo": "a_lo w_lo in place of a_lo w_hi",
         "lostep": "A's lo plane read one K-step off", "lolast": "the last K-step of the lo terms dropped",
         "lo0": "the output's lo plane zero", "reshi": "the residual rebuilt from its hi plane alone", "biascol": "the bias four columns off",
         "resrow": "the neighbouring residual row", "striprow": "the last valid strip computed from the tile's first W row",
         "vtswap": "V^T: m & 7 and the feature index exchanged"}


def mm64(ah, al, wh, wl, third):
    return ah @ wh.T + ah @ wl.T + al @ third.T


def mm32(ah, al, wh, wl, third):
    """The kernels' order in fp32: per 32 K elements the products hi.hi, a_hi.w_lo, a_lo.w_hi into one accumulator, K ascending (a
    step's 32 products are summed by the BLAS in fp32: the matrix core's own order within a step is not restated)."""
    ah, al, wh, wl, third = (x.astype(F32) for x in (ah, al, wh, wl, third))
    acc = np.zeros((ah.shape[0], wh.shape[0]), dtype=F32)
    for s in range(0, ah.shape[1], KSTEP):
        ks = slice(s, s + KSTEP)
        for x, y in ((ah, wh), (ah, wl), (al, third)):
            acc = (acc + x[:, ks] @ y[:, ks].T).astype(F32)
    return acc


def preact(p, variant=None, mm=mm64):
    """v = three products + bias [M][N] (the accumulator's type: fp64 for mm64, fp32 for mm32), or one of WRONG_PRODUCT."""
    ah, al, wh, wl, third, bias = p.ah, p.al, p.wh, p.wl, p.wh, p.bias
    if variant == "alo":
        al = np.zeros_like(al)
    elif variant == "wlo":
        wl = np.zeros_like(wl)
    elif variant == "lolo":
        third = wl
    elif variant == "lostep":
        al = np.roll(al, KSTEP, axis=1)
    elif variant == "lolast":
        al, wl = al.copy(), wl.copy()
        al[:, -KSTEP:], wl[:, -KSTEP:] = 0, 0
    elif variant == "biascol":
        bias = np.roll(bias, -4)
    elif variant == "striprow":
        wh, wl = wh.copy(), wl.copy()
        n0 = p.N // 256 * 256
        wh[p.N - 64:], wl[p.N - 64:] = wh[n0], wl[n0]
        third = wh
    acc = mm(ah, al, wh, wl, third)
    return acc + bias.astype(acc.dtype)


def vt_swapped(y):
    """[M][N] -> what the V8 layout's reader sees of a buffer written as [m / 8][m % 8][n]."""
    M, N = y.shape
    buf = y.reshape(M // 8, 8 * N)                                       # element (8 g + r, n) at r N + n
    return np.ascontiguousarray(buf.reshape(M // 8, N, 8).transpose(0, 2, 1)).reshape(M, N)


def named(p, form):
    """The wrong references named for one (operands, form).  What is left out, and why: ``lostep`` moves nothing at K = 32 (one
    step); ``striprow`` needs a partial last column tile of the 256^2 kernel (the shapes are sized for 256 CUs); ``lo0``
    needs a planes output, ``reshi`` a planes residual, ``resrow`` a residual, ``vtswap`` the V8 layout.  Everything else is held
    on every case: in the exact families by its bits, in the Gaussian one (K <= 128 by construction) outside the bound."""
    names = [k for k in WRONG_PRODUCT if not (k == "lostep" and p.K == KSTEP) and not (k == "striprow" and (x3_kernel(p.M, p.N, p.K, MI355X_CUS) != "tile256" or p.N % 256 == 0))]
    if form in ("planes", "gelu", "vt"):
        names.append("lo0")
    if form in ("res32", "resplanes"):
        names.append("resrow")
    if form == "resplanes":
        names.append("reshi")
    if form == "vt":
        names.append("vtswap")
    return names


def _gelu_f32(v):
    """gemm.hip's gelu_exact in fp32: 0.5 x (1 + erff(x 0.70710678)); torch's erf stands in for erff."""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=F32))
    with np.errstate(over="ignore", invalid="ignore"):
        return ((F32(0.5) * t * (1.0 + torch.erf(t * F32(0.70710678118654752)))).numpy()).astype(F32)


def finish(p, v, form, variant=None, rows=slice(None)):
    """The epilogue on a pre-activation.  fp64 v: the fp64 result (no rounding).  fp32 v: the kernels' epilogue in fp32, the planes
    outputs as hi + lo in fp64.  ``rows``: the rows of the operands that v holds (all by default)."""
    f32 = v.dtype == F32
    if form in ("res32", "resplanes"):
        res = p.rh if variant == "reshi" else p.rh + p.rl
        res = (np.roll(res, -1, axis=0) if variant == "resrow" else res)[rows]
        return (v + res.astype(F32)).astype(F32).astype(np.float64) if f32 else v + res
    y = (_gelu_f32(v) if f32 else gelu64(v)) if form == "gelu" else v
    if f32:
        hi, lo = split(y, p.planes)
        y = hi if variant == "lo0" else hi + lo
    elif variant == "lo0":
        y = rne(y, p.planes)
    return vt_swapped(y) if variant == "vtswap" else y


def reference(p, form, variant=None, mm=mm64):
    """One form's result, or a wrong one: fp64 (three products; the caller adds lo.lo where it wants all four), or with ``mm32`` the
    fp32 restatement."""
    return finish(p, preact(p, variant if variant in WRONG_PRODUCT else None, mm), form, variant)


@functools.lru_cache(maxsize=2)      # (the largest holds 0.6 GB of fp64 arrays; the tests of one shape follow each other)
def base(family, planes, M, N, K, seed=0):
    """Operands and what every form of one shape shares: the three-product value v3, the lo.lo term, ``ev``."""
    p = operands(family, planes, M, N, K, 9000 + seed + M + N + K)
    p.phh, p.phl, p.plh, p.pll = p.ah @ p.wh.T, p.ah @ p.wl.T, p.al @ p.wh.T, p.al @ p.wl.T
    p.v3 = p.phh + p.phl + p.plh + p.bias
    p.ratio = assert_exact_family(p) if family != "gauss" else None
    if family == "gauss":
        mass3 = np.abs(p.ah) @ np.abs(p.wh).T + np.abs(p.ah) @ np.abs(p.wl).T + np.abs(p.al) @ np.abs(p.wh).T
        p.ev = (3 * K + 1) * U * (mass3 + np.abs(p.bias)) + np.abs(p.al) @ np.abs(p.wl).T
    return p


WRONG_ROWS = 512      # above 4096 rows the wrong references are taken on the first and the last 512 rows (whole tiles of every kernel)


def wrong_rows(p):
    """The rows on which a case's wrong references are computed: all of them up to 4096 rows; beyond that -- the two 516-tile
    shapes, which repeat one tile's arithmetic down the rows -- the first and the last WRONG_ROWS.  The result under test is judged
    on every row either way."""
    if p.M <= 4096:
        return slice(None)
    return np.r_[0:WRONG_ROWS, p.M - WRONG_ROWS:p.M]


def _wrong_pre(p, k, rows):
    """A wrong pre-activation on ``rows`` from the shared products (one further, small product at most)."""
    ah, al, v3 = p.ah[rows], p.al[rows], p.v3[rows]
    if k == "lostep":
        return v3 - p.plh[rows] + np.roll(p.al, KSTEP, axis=1)[rows] @ p.wh.T
    if k == "alo":
        return v3 - p.plh[rows]
    if k == "wlo":
        return v3 - p.phl[rows]
    if k == "lolo":
        return v3 - p.plh[rows] + p.pll[rows]
    if k == "lolast":
        s = slice(p.K - KSTEP, p.K)
        return v3 - ah[:, s] @ p.wl[:, s].T - al[:, s] @ p.wh[:, s].T
    if k == "biascol":
        return v3 - p.bias + np.roll(p.bias, -4)
    if k == "striprow":
        n0, v = p.N // 256 * 256, v3.copy()
        row = (ah @ p.wh[n0] + ah @ p.wl[n0] + al @ p.wh[n0])[:, None]
        v[:, p.N - 64:] = row + p.bias[p.N - 64:]
        return v
    return v3


def case(p, form):
    """-> y64, bound (gauss), wrong {name: fp64 result}; exact families: ``y64`` is the exact value, ``with_lolo`` the four-product one.
    Computed once per (operands, form) and left unchanged."""
    if not hasattr(p, "_cases"):
        p._cases = {}
    if form not in p._cases:
        p._cases[form] = _case(p, form)
    return p._cases[form]


def _case(p, form):
    names, rows = named(p, form), wrong_rows(p)
    wrong = {k: finish(p, _wrong_pre(p, k, rows), form, k, rows) for k in names}
    if p.family != "gauss":
        # (GELU has no exact form: the pre-activation is exact, so ev = 0 and the epilogue's own bound is all there is)
        y64 = finish(p, p.v3, form)
        bound = 12 * U * np.abs(p.v3) + U_OUT[p.planes] ** 2 * np.abs(y64) + FLOOR[p.planes] if form == "gelu" else None
        return SimpleNamespace(p=p, form=form, y64=y64, bound=bound, with_lolo=finish(p, p.v3 + p.pll, form), wrong=wrong, names=names, rows=rows)
    v = p.v3 + p.pll
    y64 = finish(p, v, form)
    if form in ("res32", "resplanes"):
        bound = p.ev + U * np.abs(y64) + (U * np.abs(p.rh + p.rl) if form == "resplanes" else 0.0)
    else:
        e = R.GELU_LIPSCHITZ * p.ev + 12 * U * np.abs(v) if form == "gelu" else p.ev
        bound = e + U_OUT[p.planes] ** 2 * np.abs(y64) + FLOOR[p.planes]
    return SimpleNamespace(p=p, form=form, y64=y64, bound=bound, wrong=wrong, names=names, rows=rows)


def exact_f32(c):
    """An exact family's expected fp32 value [M][N], asserted to be exact; GELU has no exact form."""
    assert c.form != "gelu"
    v32 = c.y64.astype(F32)
    assert np.array_equal(v32.astype(np.float64), c.y64), "the three-product value is an fp32 value"
    return v32


def other_bits(c, wrong64):
    """Elements on which a wrong result, rounded to fp32 and (planes forms) split, differs from the exact one."""
    a, b = c.y64[c.rows].astype(F32), np.asarray(wrong64).astype(F32)
    if c.form in ("planes", "vt"):
        (ha, la), (hb, lb) = split(a, c.p.planes), split(b, c.p.planes)
        return int(((ha != hb) | (la != lb)).sum())
    return int((a != b).sum())


def verdict(what, c, got, check_wrong=True):
    """The Gaussian family's assertions on one result (a kernel's or the restatement's): error / bound <= 1; every named wrong
    reference outside twice the bound somewhere, and further than the bound from the result.  -> error / bound."""
    got = np.asarray(got, dtype=np.float64)
    r = ratio(got, c.y64, c.bound)
    y, b, g = c.y64[c.rows], c.bound[c.rows], got[c.rows]
    bites = {k: outside(w, y, b) for k, w in c.wrong.items()}
    apart = {k: int((np.abs(g - w) > b).sum()) for k, w in c.wrong.items()}
    print(f"\n{what}: max error / bound = {r:.4f}; elements with a wrong reference outside twice the bound {bites}, apart from the result {apart}")
    assert np.isfinite(got).all(), what
    assert r <= 1.0, what
    if check_wrong:
        assert all(bites.values()) and all(apart.values()), f"{what}: a wrong reference is inside the bound"
    return r


def checks(p, form, got, got_bits=None, check_wrong=True):
    """What the restatement and the kernels are both held to on one (operands, form).  ``got``: the result [M][N] as fp64 (planes
    forms: hi + lo); ``got_bits``: a planes output itself, torch [M][2N] (hi | lo).  -> error / bound (gauss, GELU) or None.
    Exact families: the fp32 output equals the three-product value bit for bit, a planes output the host split of that value; the
    value with lo.lo added is another fp32 number somewhere (``exact``; in ``sublo`` the lo.lo products are 2^-36, below what
    fp32 resolves of sums near 1: nothing to pin), and so is every named wrong reference."""
    what = f"x3 GEMM {p.M}x{p.N}x{p.K} {p.planes} planes, {p.family}, {form}"
    c = case(p, form)
    got = np.asarray(got, dtype=np.float64)
    if p.family == "gauss":
        return verdict(what, c, got, check_wrong)
    if form == "gelu":
        r = ratio(got, c.y64, c.bound)
        print(f"\n{what}: exact pre-activation (ev = 0), max error / the epilogue's own bound = {r:.4f}")
        assert np.isfinite(got).all() and r <= 1.0, what
        return r
    v32 = exact_f32(c)
    want = sum(split(v32, p.planes)) if form in ("planes", "vt") else c.y64
    diff = int((got != want).sum())
    print(f"\n{what}: {p.ratio / 2 ** 24:.3f} of the exact range used; elements that differ from the exact value: {diff}")
    assert diff == 0, what
    if got_bits is not None:
        assert same_bits(got_bits, split_bits(v32, p.planes)), f"{what}: the planes are not the host split of the exact value"
    if check_wrong:
        lolo = int((c.with_lolo.astype(F32) != v32).sum())
        others = {k: other_bits(c, w) for k, w in c.wrong.items()}
        print(f"  elements on which lo.lo added gives another fp32 value: {lolo}; on which a wrong reference has other bits: {others}")
        assert lolo > 0 or p.family == "sublo", f"{what}: lo.lo changes nothing: three products are not pinned"
        assert all(others.values()), f"{what}: a wrong reference has the same bits"
    return None


def release(p):
    """Drop the cases kept on a set of operands (the largest shape's are 0.6 GB per form)."""
    p.__dict__.pop("_cases", None)


# ---- the epilogue sweep ------------------------------------------------------------------------------------------------------------------
SWEEP_EXTRA = [65504.0, 65520.0, 1e5, 2e5, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1e-40, np.inf]


def x3_sweep_values():
    """mid_refs.sweep_values() with +-65504, +-65520, +-1e5, +-2e5, +-2^-14, +-2^-24, +-2^-25, +-1e-40, +-inf and NaN in its padding."""
    v = sweep_values().copy()
    extra = np.asarray([s * x for x in SWEEP_EXTRA for s in (1.0, -1.0)] + [np.nan], dtype=F32)
    assert (v[-len(extra):] == 0).all() and len(v) % 8192 == 0
    v[-len(extra):] = extra
    return v


def sweep_case(planes, form):
    """W = 0: the pre-activation is the bias exactly.  ``planes`` form: the host split of the bias, bit for bit.  ``gelu``: fp64
    under the epilogue's own bound (ev = 0) where the input is finite and, fp16 planes, the result inside +-65504 -- beyond it the hi
    plane saturates and the lo plane takes what is left, up to 131008 (the header); those and the non-finite ones are printed."""
    v32 = x3_sweep_values()
    v = v32.astype(np.float64)
    judged = np.isfinite(v) & ((np.abs(v) <= F16_MAX) if planes == "f16" else True)
    with np.errstate(over="ignore", invalid="ignore"):
        y64 = np.where(judged, gelu64(np.where(judged, v, 0.0)), np.nan) if form == "gelu" else v
        bound = 12 * U * np.abs(v) + U_OUT[planes] ** 2 * np.abs(y64) + FLOOR[planes]
    return SimpleNamespace(v32=v32, v=v, judged=judged, y64=y64, bound=bound, planes=planes, form=form,
                           lo0=rne(np.where(judged, y64, 0.0), planes))


# ---- tt_split_planes --------------------------------------------------------------------------------------------------------------------
def split_values():
    """fp32 values the split kernels are held to the host split on: every fp16 value widened to fp32 (infinities and NaNs among
    them); each +- one fp32 ulp; the midpoints between fp16 neighbours, the subnormal grid included; every seventh bf16 value, its
    two fp32 neighbours and the midpoint to the next bf16 value; the epilogue sweep's list."""
    h = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    w = h.float().numpy()
    bits = w.view(np.uint32)
    fin = np.isfinite(w)
    up, down = (bits[fin] + 1).view(F32), (bits[fin] - 1).view(F32)       # (on +-0 "down" is a NaN / the other zero's neighbour: kept)
    pos = np.sort(w[fin & (w >= 0)]).astype(np.float64)
    mid = ((pos[:-1] + pos[1:]) / 2).astype(F32)
    b = (np.arange(0, 65536, 7, dtype=np.uint32) << 16)
    bmid = (b + 0x8000).view(F32)
    with np.errstate(invalid="ignore"):
        v = np.concatenate([w, up, down, mid, -mid, b.view(F32), (b + 1).view(F32), (b - 1).view(F32), bmid, x3_sweep_values()]).astype(F32)
    return v


def split_bound(x, planes):
    """|x - hi - lo| for finite x (fp16 planes: inside +-65504): ``max(2^-22 |x|, 2^-25)`` -- below 2^-3 the lo plane is on fp16's
    subnormal grid of 2^-24; bf16 planes: ``2^-16 |x|``, and 2^-134 where the lo plane is on bf16's subnormal grid of 2^-133 (|x| <
    2^-118: two roundings of 2^-8 leave 2^-16 only while the second one is relative)."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    if planes == "f16":
        return np.maximum(2.0 ** -22 * a, 2.0 ** -25)
    return np.maximum(2.0 ** -16 * a, 2.0 ** -134)
