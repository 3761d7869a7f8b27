"""GPU: the epilogues of the five 16-bit GEMM kernels of gemm.hip -- skinny, staged, two-stage, 256^2 one-tile, 256^2 persistent --
through ``tt_gemm_bf16`` and ``tt_gemm_f16``, against fp64, under the bound tests/mid_refs.py derives from the operands
(``(K + 1) u (sum |a w| + |bias|)`` pushed through the epilogue, the epilogue function's own error, the output's rounding).
tests/test_mid_refs_host.py holds an fp32 restatement to the same bounds on the same operands, without a GPU.

Each test first computes which kernel the launcher will pick, from the rule in gemm.hip and ``tt_device_cu_count()``, and asserts
that its shape still picks the intended one: a changed rule fails loudly instead of moving the coverage.

* the integer family: every partial sum exact in fp32, so epilogues 0, 2 and 7 must give the single correct rounding of an exact
  value on every element, bit for bit -- and acc + bias is not representable on at least a quarter of them;
* cancelling rows; the Gaussian operands of today's tests with every named wrong reference outside the bound;
* the epilogue sweep: W = 0, so the pre-activation is the bias -- every bf16 value in [-12, 12], a grid of 2^-6 on [-10, 10], both
  zeros, +-1e-40, +-1e30, +-3e38 -- through GELU and tanh on every kernel that takes them, judged by the epilogue's bound alone;
  infinities and NaN;
* every other row of A and of the residual poisoned; 256 guard rows in front of C and behind it in C's own allocation; operands at
  offsets into larger buffers; fp16 saturation behind the residual and the GELU.

``tt_gemm_f32``, ``tt_gemm_x3`` and ``tt_gemm_f16c`` have their own files.  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import mid_refs as R

pytestmark = pytest.mark.gpu

FILL = -7.0
GUARD_ROWS = 256
ENTRY = {"bf16": "tt_gemm_bf16", "f16": "tt_gemm_f16"}
BIG = {"bf16": 3.0e38, "f16": 65504.0}
GEMM_PARAMS = [(k, s) for k, shapes in R.GEMM_SHAPES.items() for s in shapes]
GEMM_IDS = [f"{k}-{m}x{n}x{kk}" for k, (m, n, kk) in GEMM_PARAMS]


def _lib():
    from tensor_truth_amd import _lib as L

    return L.load_library()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _verdict(what, case, got, names=None):
    got = np.asarray(got, dtype=np.float64)
    r = R.ratio(got, case.y64, case.bound)
    wrong = {k: v for k, v in case.wrong.items() if names is None or k in names}
    bites = {k: R.outside(v, case.y64, case.bound) for k, v in wrong.items()}
    apart = {k: int((np.abs(got - v) > case.bound).sum()) for k, v in wrong.items()}
    print(f"\n{what}: max error / bound = {r:.4f}; elements with a wrong reference outside the bound {bites}, apart from the kernel {apart}")
    assert np.isfinite(got).all(), what
    assert r <= 1.0, what
    assert all(bites.values()) and all(apart.values()), f"{what}: a wrong reference is inside the bound"
    return r


class _Gemm:
    """Device operands of one shape.  C sits between GUARD_ROWS sentinel rows in front of it and behind it, in one allocation (with
    ldc = N a column past the row's end is the next row's first: the rows themselves are the guard beside it); ``offset`` puts A, W,
    the residual and C one 256-row block, and the bias 16 bytes, into larger allocations."""

    def __init__(self, lib, dev, dtname, a, w, bias, res, offset=False):
        self.lib, self.dev, self.dtname, self.fn = lib, dev, dtname, getattr(lib, ENTRY[dtname])
        self.M, self.K, self.N = a.shape[0], a.shape[1], w.shape[0]
        self.pad = 256 if offset else 0
        dt = R.DTYPES[dtname]

        def place(t, cols):
            buf = torch.full((self.pad + t.shape[0], cols), FILL, dtype=dt, device=dev)
            buf[self.pad:] = t.to(dev)
            return buf

        self.a, self.w = place(a, self.K), place(w, self.K)
        self.res = place(res, self.N) if res is not None else None
        self.bias = torch.full((4 + self.N,), FILL, dtype=torch.float32, device=dev)
        self.boff = 4 if offset else 0
        self.bias[self.boff:self.boff + self.N] = bias.to(dev)
        self.c = torch.empty((self.pad + 2 * GUARD_ROWS + self.M, self.N), dtype=dt, device=dev)

    def run(self, epi, a=None, res=None):
        """-> C [M][N] on the device (a view); the guards checked."""
        a = self.a if a is None else a
        res = self.res if res is None else res
        self.c.fill_(FILL)
        out = self.c[self.pad + GUARD_ROWS:self.pad + GUARD_ROWS + self.M]
        rc = self.fn(a[self.pad:].data_ptr(), self.w[self.pad:].data_ptr(), self.bias[self.boff:].data_ptr(),
                     res[self.pad:].data_ptr() if epi == R.EPI_RES else None, out.data_ptr(), self.M, self.N, self.K, epi, _stream(self.dev))
        assert rc == 0, (rc, self.lib.tt_last_error())
        torch.cuda.synchronize()
        assert (self.c[:self.pad + GUARD_ROWS] == FILL).all() and (self.c[self.pad + GUARD_ROWS + self.M:] == FILL).all(), "a guard row of C was written"
        return out


def _from_base(lib, dev, base, offset=False):
    t = lambda x: R.to_type(x, base.dtname)  # noqa: E731
    return _Gemm(lib, dev, base.dtname, t(base.a), t(base.w), torch.from_numpy(base.bias.astype(np.float32)), t(base.res), offset)


def _same_bits(x, y):
    return bool((x.contiguous().view(torch.int16) == y.contiguous().view(torch.int16)).all())


@pytest.mark.parametrize("dtname", R.LN_TYPES)
@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
@pytest.mark.parametrize("kernel,shape", GEMM_PARAMS, ids=GEMM_IDS)
def test_gemm_epilogues_match_fp64(dev, built_lib, kernel, shape, family, dtname):
    lib = _lib()
    M, N, K = shape
    cus = lib.tt_device_cu_count()
    base = R.gemm_base(family, dtname, M, N, K)
    g = _from_base(lib, dev, base)
    for epi in R.gemm_epis(kernel):
        assert R.gemm_kernel(M, N, K, epi, cus) == kernel, f"{M}x{N}x{K} epilogue {epi} no longer picks the {kernel} kernel on {cus} CUs"
        out = g.run(epi)
        R.gemm_checks(base, epi, out.cpu().double().numpy(), _verdict)
        if family != "gauss":
            continue
        # row isolation: every other row of A and of the residual poisoned: the clean rows keep their bits
        keep = out[0::2].clone()
        for poison in (float("nan"), BIG[dtname]):
            a2, r2 = g.a.clone(), g.res.clone()
            a2[1::2] = poison
            r2[1::2] = poison
            assert _same_bits(g.run(epi, a=a2, res=r2)[0::2], keep), f"{kernel} epilogue {epi}: rows next to rows of {poison} changed"


@pytest.mark.parametrize("dtname", R.LN_TYPES)
def test_residual_with_an_odd_k_step_count_falls_back(dev, built_lib, dtname):
    """K = 192 on 4096 x 2048: the one-tile kernel stages the residual as two pseudo K-tiles and needs an even K-step count; the
    launcher must hand the residual epilogue to the two-stage kernel, and the result must still be right."""
    lib = _lib()
    cus = lib.tt_device_cu_count()
    M, N, K = 4096, 2048, 192
    assert R.gemm_kernel(M, N, K, R.EPI_RES, cus) == "twostage" and R.gemm_kernel(M, N, K, R.EPI_BIAS, cus) == "onetile"
    for family in ("int", "gauss"):
        base = R.gemm_base(family, dtname, M, N, K)
        g = _from_base(lib, dev, base)
        for epi in (R.EPI_RES, R.EPI_BIAS):
            R.gemm_checks(base, epi, g.run(epi).cpu().double().numpy(), _verdict)


@pytest.mark.parametrize("dtname", R.LN_TYPES)
@pytest.mark.parametrize("kernel,shape", [("skinny", (256, 48, 96)), ("staged", (384, 128, 192)), ("twostage", (4224, 1024, 64)),
                                          ("onetile", (4096, 2048, 128)), ("persistent", (8448, 2048, 128))])
def test_gemm_operands_at_offsets(dev, built_lib, kernel, shape, dtname):
    """The bias 16 bytes, and A, W, the residual and C one 256-row block, into larger allocations: the same bits."""
    lib = _lib()
    M, N, K = shape
    base = R.gemm_base("gauss", dtname, M, N, K)
    plain, moved = _from_base(lib, dev, base), _from_base(lib, dev, base, offset=True)
    for epi in R.gemm_epis(kernel):
        assert R.gemm_kernel(M, N, K, epi, lib.tt_device_cu_count()) == kernel
        assert _same_bits(plain.run(epi), moved.run(epi)), f"{kernel} epilogue {epi}: operands at an offset give other bits"


# ---- the epilogue sweep -----------------------------------------------------------------------------------------------------------------
def _sweep(lib, dev, kernel, dtname, epi, values):
    """W = 0 and bias = values, 8192 columns a launch -> row 0 of every launch (every row must carry the same bits)."""
    M, N, K = R.SWEEP_SHAPES[kernel]
    gen = torch.Generator().manual_seed(5)
    a = torch.randn(M, K, generator=gen).to(R.DTYPES[dtname])
    g = _Gemm(lib, dev, dtname, a, torch.zeros(N, K, dtype=R.DTYPES[dtname]), torch.zeros(N), None)
    rows = []
    for i in range(0, len(values), N):
        g.bias[:N] = torch.from_numpy(values[i:i + N]).to(dev)
        out = g.run(epi)
        assert _same_bits(out, out[:1].expand(M, N)), "W = 0: every row is the epilogue of the bias"
        rows.append(out[0].cpu())
    return torch.cat(rows)


@pytest.mark.parametrize("dtname", R.LN_TYPES)
@pytest.mark.parametrize("kernel,epi", [(k, e) for k in R.SWEEP_SHAPES for e in (R.EPI_GELU, R.EPI_TANH) if not (k == "persistent" and e == R.EPI_TANH)])
def test_epilogue_sweep(dev, built_lib, kernel, epi, dtname):
    lib = _lib()
    M, N, K = R.SWEEP_SHAPES[kernel]
    assert R.gemm_kernel(M, N, K, epi, lib.tt_device_cu_count()) == kernel
    c = R.sweep_case(epi, dtname)
    got_t = _sweep(lib, dev, kernel, dtname, epi, c.v32)
    got = got_t.double().numpy()
    names = ["tanhgelu", "roundacc"] if epi == R.EPI_GELU else []
    _verdict(f"epilogue sweep, {kernel} kernel, epilogue {epi}, {dtname}", c, got, names)
    # what the output's type resolves of the function's own error: where its rounding is below 1e-6
    fine = (R.U_OUT[dtname] * np.abs(c.y64) < 1e-6) & (np.abs(c.v) < 1e3)
    err = np.abs(got - c.y64)
    neg0 = np.flatnonzero((c.v == 0) & np.signbit(c.v))[0]
    print(f"  largest |error| where the output resolves 1e-6: {err[fine].max():.3e} at v = {c.v[fine][np.argmax(err[fine])]:.4f}; "
          f"-0 gives {'-0' if np.signbit(got[neg0]) else '+0'}")
    if epi == R.EPI_GELU:
        tail = (c.v < 0) & fine & (R.gelu_correction(c.v) > 1e-30)
        rel = (err[tail] - R.U_OUT[dtname] * np.abs(c.y64[tail]) - R.TINY[dtname] - 4 * R.U * np.abs(c.v[tail])) / R.gelu_correction(c.v[tail])
        print(f"  largest (|error| - the output's rounding - 4 u |v|) / correction term on v < 0: {rel.max():.3e}")
    assert got[neg0] == 0
    # infinities and NaN: a NaN stays NaN; what the infinities give is the header's contract
    special = np.zeros(N, dtype=np.float32)
    special[:3] = [np.inf, -np.inf, np.nan]
    s = _sweep(lib, dev, kernel, dtname, epi, special)[:3].double().numpy()
    print(f"  epilogue {epi} of +inf, -inf, NaN: {s}")
    assert np.isnan(s[2]), "a NaN pre-activation must stay NaN"
    if epi == R.EPI_GELU:
        assert not np.isfinite(s[:2]).any(), "GELU of an infinite pre-activation: non-finite (the header: NaN, from inf * 2^-inf)"
    else:
        assert s[0] == 1 and s[1] == -1


# ---- fp16 only -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,shape", [("skinny", (64, 16, 32)), ("staged", (384, 128, 64)), ("onetile", (4096, 2048, 128))])
def test_fp16_saturates_behind_the_residual_and_the_gelu(dev, built_lib, kernel, shape):
    """acc + bias = 6e4 and a residual of 6e4 store +-65504, not an infinity; a GELU input of 7e4 stays finite."""
    lib = _lib()
    M, N, K = shape
    a = torch.zeros(M, K, dtype=torch.float16)
    w = torch.zeros(N, K, dtype=torch.float16)
    a[:, 0], w[:, 0] = 200.0, 200.0                          # acc = 4e4
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    w[:, 0] *= sign.half()
    res = (6.0e4 * sign).half().expand(M, N).contiguous()
    g = _Gemm(lib, dev, "f16", a, w, 2.0e4 * sign, res)
    assert R.gemm_kernel(M, N, K, R.EPI_RES, lib.tt_device_cu_count()) == kernel
    out = g.run(R.EPI_RES).cpu().float()
    assert (out == 65504.0 * sign).all(), "fp16: acc + bias + residual beyond the range must saturate at +-65504"
    g.bias[:N] = (3.0e4 * sign).to(dev)                      # pre-activation +-7e4
    out = g.run(R.EPI_GELU).cpu().float()
    print(f"\nfp16 GELU of +-7e4 on the {kernel} kernel: {out[0, :2].tolist()}")
    assert torch.isfinite(out).all() and (out[:, 0::2] == 65504.0).all() and (out[:, 1::2] == 0).all()
