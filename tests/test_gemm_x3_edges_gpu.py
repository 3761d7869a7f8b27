"""GPU: the split-plane GEMMs of the default precision -- the relay, staged and 256^2 kernels behind ``GemmParams.x3``, bf16 and fp16
planes -- through ``tt_gemm_x3_ex`` / ``tt_gemm_x3_ex_f16`` with every epilogue and layout the forward uses (planes out, GELU planes
out, fp32 out with the residual as fp32 rows or rebuilt from its planes, V^T into the V8 hi / lo buffers), and ``tt_split_planes`` /
``tt_split_planes_f16`` against the host split the weights get.  References, operand families, bounds and wrong references:
tests/x3_refs.py; tests/test_x3_refs_host.py holds an fp32 restatement to the same checks without a GPU.

* exact and subnormal-lo families: every partial sum of the three products is exact in fp32, so the fp32 output is the
  three-product value bit for bit, a planes output (V8 included) the host split of it -- at every K, where no fp64 bound can tell a
  dropped lo plane from rounding.  The subnormal-lo family is exact only if the fp16 matrix core keeps subnormal inputs;
* Gaussian family (K <= 128): error / bound <= 1 against fp64, every named wrong reference outside twice the bound;
* the epilogue sweep (W = 0: the pre-activation is the bias): epilogue 0 gives the host split of the bias bit for bit; the GELU is
  judged by its own bound.  What comes out for inputs that are not judged -- +-inf, NaN, and for fp16 planes finite values beyond
  +-65504 -- is printed: a NaN stays a NaN; +-inf gives NaN planes through the GELU (inf * 0 or inf - inf) and, through
  epilogue 0, hi = +-inf, lo = NaN (bf16) or hi = lo = +-65504 (fp16: both planes saturate), as the host split does;
* guards: sentinel rows in front of and behind every output in its own allocation, sentinel columns between n and the lo plane
  and behind it, A, W, residual and output at offsets in larger buffers; the forward's own tight layouts give the same bits;
* a row's bits do not depend on the kernel that computed it, for every form.

Each test asserts from the rule in gemm.hip (``x3_refs.x3_kernel``) and ``tt_device_cu_count()`` that its shape still picks the
intended kernel.  Every figure is printed before it is asserted.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import x3_refs as X

pytestmark = pytest.mark.gpu

FILL = -7.0
GUARD_ROWS = 256
ENTRY = {"bf16": "tt_gemm_x3_ex", "f16": "tt_gemm_x3_ex_f16"}
SPLIT = {"bf16": "tt_split_planes", "f16": "tt_split_planes_f16"}


def _lib():
    from tensor_truth_amd import _lib as L

    return L.load_library()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _X3:
    """Device operands of one shape and one output buffer per form.  A, W and the residuals sit one 256-row block, the bias 16
    bytes, into larger allocations filled with the sentinel; every output sits between GUARD_ROWS sentinel rows (V8: GUARD_ROWS / 8
    token groups) in one allocation, with sentinel columns between n and the lo plane and behind it (``tight``: the forward's own
    layouts instead, ldc = 2n / c_lo_off = n, ldr = 2n / res_lo_off = n, ldvt = 8n)."""

    def __init__(self, lib, dev, p, tight=False):
        self.lib, self.dev, self.p, self.fn = lib, dev, p, getattr(lib, ENTRY[p.planes])
        M, N, K = p.M, p.N, p.K
        dt = X.PLANES[p.planes]
        gap = 0 if tight else 8
        self.c_lo_off, self.ldc = N + 2 * gap, 2 * N + 5 * gap
        self.res_lo_off, self.ldr = N + gap, 2 * N + 3 * gap
        self.ldc32, self.ldr32, self.ldvt = N + gap, N + gap, 8 * N + 2 * gap

        def place(t, cols, dtype):
            buf = torch.full((256 + t.shape[0], cols), FILL, dtype=dtype, device=dev)
            buf[256:, :t.shape[1]] = t.to(dev)
            return buf

        self.a = place(X.planes_tensor(p.ah, p.al, p.planes), 2 * K, dt)
        self.w = place(X.planes_tensor(p.wh, p.wl, p.planes), 2 * K, dt)
        self.res32 = self.resp = None
        if p.rh is not None:                                  # (the sweep has no residual)
            self.res32 = place(torch.from_numpy((p.rh + p.rl).astype(np.float32)), self.ldr32, torch.float32)
            rp = torch.full((M, self.ldr), FILL, dtype=dt)
            rp[:, :N], rp[:, self.res_lo_off:self.res_lo_off + N] = torch.from_numpy(p.rh).to(dt), torch.from_numpy(p.rl).to(dt)
            self.resp = place(rp, self.ldr, dt)
        self.bias = torch.full((4 + N,), FILL, dtype=torch.float32, device=dev)
        self.bias[4:] = torch.from_numpy(p.bias.astype(np.float32)).to(dev)
        self.c = torch.empty((256 + 2 * GUARD_ROWS + M, self.ldc), dtype=dt, device=dev)
        self.c32 = torch.empty((256 + 2 * GUARD_ROWS + M, self.ldc32), dtype=torch.float32, device=dev)
        g8 = GUARD_ROWS // 8
        self.vt = [torch.empty((2 * g8 + M // 8, self.ldvt), dtype=dt, device=dev) for _ in range(2)]

    def run(self, form, rows=None):
        """-> (result [rows][N] as fp64 numpy -- planes forms: hi + lo --, the planes [rows][2N] on the CPU or None); the first ``rows``
        rows only (all by default); every guard checked."""
        p, N = self.p, self.p.N
        M = p.M if rows is None else rows
        epi = X.EPI[form]
        first, g8 = 256 + GUARD_ROWS, GUARD_ROWS // 8
        for t in (self.c, self.c32, *self.vt):
            t.fill_(FILL)
        rc = self.fn(self.a[256:].data_ptr(), self.w[256:].data_ptr(), self.bias[4:].data_ptr(),
                     _ptr(self.res32[256:]) if form == "res32" else None, _ptr(self.resp[256:]) if form == "resplanes" else None,
                     self.ldr if form == "resplanes" else self.ldr32, self.res_lo_off,
                     self.c[first:].data_ptr(), self.ldc32 if epi == 2 else self.ldc, self.c_lo_off, self.c32[first:].data_ptr(),
                     self.vt[0][g8:].data_ptr(), self.vt[1][g8:].data_ptr(), self.ldvt, M, N, p.K, epi, _stream(self.dev))
        assert rc == 0, (rc, self.lib.tt_last_error())
        torch.cuda.synchronize()
        lo = self.c_lo_off
        touched = {"planes": self.c, "gelu": self.c, "res32": self.c32, "resplanes": self.c32}.get(form)
        for t in (self.c, self.c32):
            body = t[first:first + M] if t is touched else t[:0]
            assert (t[:first] == FILL).all() and (t[first + body.shape[0]:] == FILL).all(), f"{form}: a guard row was written"
        for t in self.vt:
            n8 = M // 8 if form == "vt" else 0
            assert (t[:g8] == FILL).all() and (t[g8 + n8:] == FILL).all() and (t[:, 8 * N:] == FILL).all(), f"{form}: a V8 guard was written"
        if form in ("planes", "gelu"):
            out = self.c[first:first + M]
            assert (out[:, N:lo] == FILL).all() and (out[:, lo + N:] == FILL).all(), f"{form}: a guard column of the planes was written"
            bits = torch.cat([out[:, :N], out[:, lo:lo + N]], 1).cpu()
        elif form == "vt":
            hl = [t[g8:g8 + M // 8, :8 * N].reshape(M // 8, N, 8).permute(0, 2, 1).reshape(M, N) for t in self.vt]
            bits = torch.cat(hl, 1).cpu()
        else:
            out = self.c32[first:first + M]
            assert (out[:, N:] == FILL).all(), f"{form}: a guard column of the fp32 output was written"
            return out[:, :N].cpu().double().numpy(), None
        return bits[:, :N].double().numpy() + bits[:, N:].double().numpy(), bits


@pytest.mark.parametrize("kernel,shape,planes,family", X.CASES, ids=X.CASE_IDS)
def test_x3_gemm_every_form(dev, built_lib, kernel, shape, planes, family):
    lib = _lib()
    M, N, K = shape
    cus = lib.tt_device_cu_count()
    assert X.x3_kernel(M, N, K, cus) == kernel, f"{M}x{N}x{K} no longer picks the {kernel} kernel on {cus} CUs"
    p = X.base(family, planes, M, N, K)
    g = _X3(lib, dev, p)
    for form in X.FORMS:
        got, bits = g.run(form)
        X.checks(p, form, got, bits)
    X.release(p)


@pytest.mark.parametrize("planes", list(X.PLANES))
@pytest.mark.parametrize("kernel,shape", [("relay", (256, 48, 288)), ("staged", (512, 384, 128)), ("tile256", (512, 448, 256))])
def test_the_forwards_own_layouts(dev, built_lib, kernel, shape, planes):
    """Q | K as [M][4N'] with c_lo_off = 2N' (n = 2N': ldc = 2n, c_lo_off = n), the residual's planes with ldr = 2N and res_lo_off =
    N, V8 rows of exactly 8N: the same checks, and the same bits as with guard columns between the planes."""
    lib = _lib()
    M, N, K = shape
    assert X.x3_kernel(M, N, K, lib.tt_device_cu_count()) == kernel
    p = X.base("exact", planes, M, N, K)
    tight, gapped = _X3(lib, dev, p, tight=True), _X3(lib, dev, p)
    assert (tight.ldc, tight.c_lo_off, tight.ldr, tight.res_lo_off, tight.ldvt) == (2 * N, N, 2 * N, N, 8 * N)
    for form in X.FORMS:
        got, bits = tight.run(form)
        X.checks(p, form, got, bits, check_wrong=False)
        got2, bits2 = gapped.run(form)
        assert np.array_equal(got, got2) and (bits is None or torch.equal(bits.view(torch.int16), bits2.view(torch.int16))), form


@pytest.mark.parametrize("planes", list(X.PLANES))
def test_a_rows_bits_do_not_depend_on_the_kernel(dev, built_lib, planes):
    """The first rows of one A through the relay, the staged and the 256^2 kernel: the same bits in every form -- planes, GELU planes,
    fp32 with either residual, V8."""
    lib = _lib()
    cus = lib.tt_device_cu_count()
    N, K = X.IDENTITY_NK
    big = X.IDENTITY_ROWS["tile256"]
    p = X.operands("gauss", planes, big, N, K, 77)
    g = _X3(lib, dev, p)
    for kernel, rows in X.IDENTITY_ROWS.items():
        assert X.x3_kernel(rows, N, K, cus) == kernel, f"{rows}x{N}x{K} no longer picks the {kernel} kernel on {cus} CUs"
    for form in X.FORMS:
        want, wbits = g.run(form)
        assert np.isfinite(want).all()
        for kernel, rows in X.IDENTITY_ROWS.items():
            if rows == big:
                continue
            got, bits = g.run(form, rows=rows)
            same = np.array_equal(got, want[:rows]) and (bits is None or torch.equal(bits.view(torch.int16), wbits[:rows].view(torch.int16)))
            assert same, f"{form}: the {kernel} kernel's rows carry other bits than the 256^2 kernel's"


# ---- the epilogue sweep -----------------------------------------------------------------------------------------------------------------
def _sweep(lib, dev, kernel, planes, form, values):
    """W = 0 and bias = values, 8192 columns a launch -> row 0 of every launch as planes [1][2 len] (every row must carry its bits)."""
    M, N, K = X.SWEEP_SHAPES[kernel]
    ah, al = X.split(np.random.default_rng(5).standard_normal((M, K)).astype(np.float32), planes)
    zero = np.zeros((N, K))
    g = _X3(lib, dev, SimpleNamespace(planes=planes, M=M, N=N, K=K, ah=ah, al=al, wh=zero, wl=zero, bias=np.zeros(N), rh=None, rl=None))
    his, los = [], []
    for i in range(0, len(values), N):
        g.bias[4:] = torch.from_numpy(values[i:i + N]).to(dev)
        _, bits = g.run(form)
        b16 = bits.view(torch.int16)
        assert bool(((b16 == b16[:1]) | (bits.isnan() & bits[:1].isnan())).all()), "W = 0: every row is the epilogue of the bias"
        his.append(bits[0, :N])
        los.append(bits[0, N:])
    return torch.cat(his + los)[None]


@pytest.mark.parametrize("planes", list(X.PLANES))
@pytest.mark.parametrize("form", ["planes", "gelu"])
@pytest.mark.parametrize("kernel", list(X.SWEEP_SHAPES))
def test_x3_epilogue_sweep(dev, built_lib, kernel, form, planes):
    lib = _lib()
    assert X.x3_kernel(*X.SWEEP_SHAPES[kernel], lib.tt_device_cu_count()) == kernel
    c = X.sweep_case(planes, form)
    bits = _sweep(lib, dev, kernel, planes, form, c.v32)
    n = len(c.v32)
    hi, lo = bits[0, :n].double().numpy(), bits[0, n:].double().numpy()
    rest = np.flatnonzero(~c.judged)
    with np.errstate(invalid="ignore"):
        print(f"\nsweep, {kernel} kernel, {planes} planes, {form}: inputs outside the judged range and what they give (hi, lo): "
              + "; ".join(f"{c.v32[i]:g} -> ({hi[i]:g}, {lo[i]:g})" for i in rest))
    assert np.isnan(hi[-1]) and np.isnan(c.v32[-1]), "a NaN pre-activation must stay a NaN"
    if form == "planes":
        want = X.split_bits((np.float32(0) + c.v32)[None], planes)      # (the accumulator's +0 plus the bias: a bias of -0 gives +0)
        diff = int((~((bits.view(torch.int16) == want.view(torch.int16)) | (bits.isnan() & want.isnan()))).sum())
        print(f"  epilogue 0: elements of the planes that are not the host split of the bias: {diff} of {2 * n}")
        assert diff == 0
        return
    j = c.judged
    got = hi[j] + lo[j]
    r = X.ratio(got, c.y64[j], c.bound[j])
    out = X.outside(c.lo0[j], c.y64[j], c.bound[j])
    apart = int((np.abs(got - c.lo0[j]) > c.bound[j]).sum())
    print(f"  GELU: {int(j.sum())} judged values, max error / bound = {r:.4f}; the lo plane dropped is outside on {out}, apart from the kernel on {apart}")
    assert np.isfinite(got).all() and r <= 1.0 and out > 0 and apart > 0
    # the header's contract for the infinities (the values' last three are +inf, -inf, NaN): GELU(+inf) is the split of +inf, GELU(-inf) NaN
    assert np.isposinf(c.v32[-3]) and np.isneginf(c.v32[-2])
    assert hi[-3] == (np.inf if planes == "bf16" else X.F16_MAX) and (np.isnan(lo[-3]) if planes == "bf16" else lo[-3] == X.F16_MAX)
    assert np.isnan(hi[-2]) and np.isnan(lo[-2])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", list(X.PLANES))
def test_x3_ex_refuses_before_it_launches(dev, built_lib, planes):
    lib = _lib()
    p = X.operands("exact", planes, 512, 128, 128, 3)
    g = _X3(lib, dev, p, tight=True)
    for t in (g.c, g.c32, *g.vt):
        t.fill_(FILL)
    a, w, b = g.a[256:].data_ptr(), g.w[256:].data_ptr(), g.bias[4:].data_ptr()
    c, c32, r32, rp = g.c.data_ptr(), g.c32.data_ptr(), g.res32[256:].data_ptr(), g.resp[256:].data_ptr()
    vh, vl = g.vt[0].data_ptr(), g.vt[1].data_ptr()
    M, N, K = 512, 128, 128
    bad = {"lo plane inside the hi plane": (a, w, b, None, None, 0, 0, c, 2 * N, N - 8, None, None, None, 0, M, N, K, 0),
           "ldc short of the lo plane": (a, w, b, None, None, 0, 0, c, 2 * N - 8, N, None, None, None, 0, M, N, K, 1),
           "ldc not a multiple of 8": (a, w, b, None, None, 0, 0, c, 2 * N + 4, N, None, None, None, 0, M, N, K, 0),
           "no planes output": (a, w, b, None, None, 0, 0, None, 2 * N, N, None, None, None, 0, M, N, K, 0),
           "both residuals": (a, w, b, r32, rp, 2 * N, N, None, N, 0, c32, None, None, 0, M, N, K, 2),
           "no residual": (a, w, b, None, None, N, 0, None, N, 0, c32, None, None, 0, M, N, K, 2),
           "residual lo plane inside the hi plane": (a, w, b, None, rp, 2 * N, N - 8, None, N, 0, c32, None, None, 0, M, N, K, 2),
           "V8 row shorter than 8 n": (a, w, b, None, None, 0, 0, None, 0, 0, None, vh, vl, 8 * N - 8, M, N, K, 5),
           "V8 lo plane missing": (a, w, b, None, None, 0, 0, None, 0, 0, None, vh, None, 8 * N, M, N, K, 5),
           "tanh epilogue": (a, w, b, None, None, 0, 0, c, 2 * N, N, None, None, None, 0, M, N, K, 3),
           "320 rows": (a, w, b, None, None, 0, 0, c, 2 * N, N, None, None, None, 0, 320, N, K, 0),
           "n = 72 beyond 256 rows": (a, w, b, None, None, 0, 0, c, 2 * N, 72, None, None, None, 0, M, 72, K, 0),
           "k = 64 beyond 256 rows": (a, w, b, None, None, 0, 0, c, 2 * N, N, None, None, None, 0, M, N, 64, 0),
           "null bias": (a, w, None, None, None, 0, 0, c, 2 * N, N, None, None, None, 0, M, N, K, 0)}
    fn = getattr(lib, ENTRY[planes])
    for what, args in bad.items():
        rc = fn(*args, _stream(dev))
        assert rc != 0 and lib.tt_last_error(), f"{what}: accepted"
    torch.cuda.synchronize()
    assert all(bool((t == FILL).all()) for t in (g.c, g.c32, *g.vt)), "a refused call wrote"


# ---- tt_split_planes / tt_split_planes_f16 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", list(X.PLANES))
def test_split_planes_equal_the_host_split(dev, built_lib, planes):
    """The activations are split on the device (pack_e2, saturating), the weights on the host (encoder_x3.split_planes): the same
    bits on every fp16 value widened to fp32, its fp32 neighbours, the midpoints between fp16 neighbours (the subnormal grid
    included), a sample of the bf16 values likewise, and the sweep's list -- infinities, NaN, +-65504 and beyond, the fp32
    subnormals.  cols 4, 8 and 324; rows 0, 1, 777 and all of them."""
    lib = _lib()
    fn = getattr(lib, SPLIT[planes])
    dt = X.PLANES[planes]
    x = X.split_values()
    hi, lo = X.split(x, planes)
    ok = np.isfinite(x) & np.isfinite(hi) & ((np.abs(x) <= X.F16_MAX) if planes == "f16" else True)
    for cols in (4, 8, 324):
        full = len(x) // cols
        v = torch.from_numpy(x[:full * cols].reshape(full, cols).copy())
        want = X.split_bits(v.numpy(), planes)
        dv = v.to(dev)
        for rows in (0, 1, 777, full):
            out = torch.full((rows + 8, 2 * cols), FILL, dtype=dt, device=dev)
            rc = fn(dv.data_ptr(), rows, cols, out.data_ptr(), _stream(dev))
            assert rc == 0, (rc, lib.tt_last_error())
            torch.cuda.synchronize()
            assert (out[rows:] == FILL).all(), "rows behind the last one were written"
            got = out[:rows].cpu()
            bad = ~((got.view(torch.int16) == want[:rows].view(torch.int16)) | (got.isnan() & want[:rows].isnan()))
            if bad.any():
                r, c = [int(i) for i in bad.nonzero()[0]]
                print(f"\n{SPLIT[planes]} cols {cols} rows {rows}: {int(bad.sum())} elements differ from the host split, first: x = "
                      f"{float(v[r, c % cols]):.9g} ({'lo' if c >= cols else 'hi'}) device {float(got[r, c]):.9g} host {float(want[r, c]):.9g}")
            assert not bad.any()
        got64 = got.double().numpy()
        k = ok[:full * cols].reshape(full, cols)
        with np.errstate(invalid="ignore"):                  # (inf - inf among the values that are not judged)
            err = np.abs(v.double().numpy() - got64[:, :cols] - got64[:, cols:])[k]
        worst = float((err / X.split_bound(v.numpy()[k], planes)).max())
        print(f"\n{SPLIT[planes]} cols {cols}: {int(k.sum())} finite values in range, max |x - hi - lo| / bound = {worst:.4f}")
        assert worst <= 1.0
    assert fn(dv.data_ptr(), 4, 6, out.data_ptr(), _stream(dev)) != 0, "cols must be a multiple of 4"
