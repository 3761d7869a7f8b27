"""CPU: the helper of tests/test_gemm_x3_edges_gpu.py (tests/x3_refs.py) on the operands the GPU tests use.

* An fp32 restatement of the three products, taken in 32-element K-steps in the kernels' order, passes every check the kernels are
  held to: inside the fp64 bound on the Gaussian family, bit-equal to the exact value on the exact and subnormal-lo families.
* The exactness and split conditions of the two exact families hold on every shape listed.
* Every named wrong reference is outside the bound (Gaussian) or has other bits (exact families).
* Each wrong form, written into the restatement itself, fails the same checks (shapes up to 4096 rows: the two 516-tile shapes
  repeat the 512-row ones' arithmetic 43 and 64 times over).
* The restated launcher rule picks the intended kernel for every listed shape at 256 CUs.

Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

import x3_refs as X


def test_kernel_rule_picks_the_intended_kernel_at_256_cus():
    for kernel, shapes in X.SHAPES.items():
        for M, N, K in shapes:
            assert X.x3_kernel(M, N, K, X.MI355X_CUS) == kernel, (kernel, M, N, K)
    for kernel, (M, N, K) in X.SWEEP_SHAPES.items():
        assert X.x3_kernel(M, N, K, X.MI355X_CUS) == kernel, (kernel, M, N, K)
    for kernel, M in X.IDENTITY_ROWS.items():
        assert X.x3_kernel(M, *X.IDENTITY_NK, X.MI355X_CUS) == kernel
    # the edges of the rule itself
    assert X.x3_kernel(320, 64, 128, 256) is None and X.x3_kernel(512, 72, 128, 256) is None and X.x3_kernel(512, 128, 64, 256) is None
    assert X.x3_kernel(512, 128, 96, 256) is None and X.x3_kernel(256, 16, 96, 256) == "relay" and X.x3_kernel(192, 16, 48, 256) is None
    assert X.x3_kernel(512 * 128, 128, 128, 256) == "staged" and X.x3_kernel(513 * 128 * 2, 128, 128, 256) == "tile256"
    assert X.x3_kernel(33024, 256, 128, 304) == "staged", "the tiled shapes are sized for 256 CUs: on more, the GPU tests say so"
    # the partial last column tile is reached by every shape listed for it, and only by those
    partial = [(m, n, k) for m, n, k in X.SHAPES["tile256"] if n % 256]
    assert len(partial) == 5 and {n % 256 for _, n, _ in partial} == {64, 192, 128}


@pytest.mark.parametrize("kernel,shape,planes,family", X.CASES, ids=X.CASE_IDS)
def test_restatement_passes_wrong_forms_fail(kernel, shape, planes, family):
    M, N, K = shape
    p = X.base(family, planes, M, N, K)
    if family != "gauss":
        print(f"\n{family} {planes} {M}x{N}x{K}: largest sum of magnitudes = {p.ratio:.3g} quanta ({p.ratio / 2 ** 24:.3f} of 2^24)")
    pre = {None: X.preact(p, mm=X.mm32)}                  # the restatement's fp32 pre-activation, and each wrong form's, once
    for form in X.FORMS:
        names = X.named(p, form)
        assert ("striprow" in names) == (kernel == "tile256" and N % 256 != 0) and ("lostep" in names) == (K > 32)
        assert {"alo", "wlo", "lolo", "lolast", "biascol"} <= set(names)
        r = X.checks(p, form, X.finish(p, pre[None], form))
        if family == "gauss":
            assert r > 1e-4, "the restatement is not the fp64 reference itself"
        if M > 4096 or (family != "gauss" and form == "gelu"):
            continue
        for k in names:
            v = k if k in X.WRONG_PRODUCT else None
            if v not in pre:
                pre[v] = X.preact(p, v, X.mm32)
            with pytest.raises(AssertionError):
                X.checks(p, form, X.finish(p, pre[v], form, k), check_wrong=False)
    X.release(p)


@pytest.mark.parametrize("planes", list(X.PLANES))
def test_sweep_and_split_values(planes):
    v = X.x3_sweep_values()
    assert len(v) % 8192 == 0 and np.isnan(v[-1]) and np.isinf(v[-3:-1]).all()
    for x in (65504.0, 65520.0, 1e5, 2e5, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 1e-40):
        assert (v == np.float32(x)).any() and (v == np.float32(-x)).any()
    # the GELU restatement inside the sweep's bound, the output's lo plane dropped outside it
    c = X.sweep_case(planes, "gelu")
    j = c.judged
    got = sum(X.split(X._gelu_f32(c.v32[j]), planes))
    r = X.ratio(got, c.y64[j], c.bound[j])
    out = X.outside(c.lo0[j], c.y64[j], c.bound[j])
    print(f"\nsweep, GELU, {planes} planes: {int(j.sum())} judged values, max error / bound = {r:.4f}; lo plane dropped: outside on {out}")
    assert r <= 1.0 and out > 0
    # the host split on the split kernels' values: the bounds of x3_refs.split_bound hold where they are claimed
    x = X.split_values()
    hi, lo = X.split(x, planes)
    ok = np.isfinite(x) & np.isfinite(hi) & ((np.abs(x) <= X.F16_MAX) if planes == "f16" else True)
    err = np.abs(x[ok].astype(np.float64) - hi[ok] - lo[ok])
    worst = float((err / X.split_bound(x[ok], planes)).max())
    print(f"  host split, {planes} planes, {int(ok.sum())} finite values: max |x - hi - lo| / bound = {worst:.4f}")
    assert worst <= 1.0
    if planes == "f16":
        sub = ok & (np.abs(x) < 2.0 ** -3) & (lo != 0)
        assert (np.abs(lo[sub]) < 2.0 ** -14).all() and sub.sum() > 1000, "below 2^-3 the lo plane is an fp16 subnormal"
        big = np.isfinite(x) & (np.abs(x) > X.F16_MAX)
        assert (np.abs(hi[big]) == X.F16_MAX).all(), "beyond the range the hi plane saturates"
