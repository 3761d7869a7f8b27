"""CPU: the helper of tests/test_rowops_gpu.py and tests/test_gemm_edges_gpu.py (tests/mid_refs.py) on the inputs the GPU tests use.

* An fp32 numpy restatement of each kernel's arithmetic, in the kernel's own order, stays within the bound of the fp64 reference.
* Every named wrong reference lies outside the bound (further than twice the bound from fp64) on the cases it is named for.
* What is invisible by construction is asserted to be: the divisor H - 1 behind a 16-bit output where nothing cancels against beta,
  the accumulator rounded before a ReLU (the same bits) and before a tanh (never two bounds away, and yet a kernel doing it leaves
  the bound, because its two roundings add).
* The claims in gemm.hip's comments on gelu_erf2 and gelu_erfc hold for their restatements over the sweep.

Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

import mid_refs as R


def _check(what, case, got, names=None):
    r = R.ratio(got, case.y64, case.bound)
    bites = {k: R.outside(v, case.y64, case.bound) for k, v in case.wrong.items() if names is None or k in names}
    print(f"\n{what}: max error / bound = {r:.4f}; elements on which a wrong reference is outside the bound {bites}")
    assert np.isfinite(np.asarray(got)).all(), what
    assert r <= 1.0, what
    assert all(v > 0 for v in bites.values()), f"{what}: a wrong reference is inside the bound on these inputs: {bites}"
    return r


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("dtname", R.LN_TYPES)
@pytest.mark.parametrize("H", R.H_LN)
def test_layernorm_restatement_within_bound_wrong_references_outside(H, dtname, eps):
    c = R.ln_case(H, dtname, eps)
    got = c.emulate()
    _check(f"LayerNorm H {H} {dtname} eps {eps}", c, got)
    assert {"epsoutside", "rownext"} <= set(c.wrong) <= set(R.LN_WRONG) and ({"firstchunk", "gbchunk"} <= set(c.wrong)) == (H > 512)
    var = c.x.var(1)
    fam = {f: np.arange(c.n)[i::6] for i, f in enumerate(R.FAMILIES)}
    if eps > 1e-8:
        assert (var[fam["c"]] > eps / 4).all() and (var[fam["c"]] < 4 * eps).all(), "family (c): a variance of the order of eps"
    else:
        assert (var[fam["c"]] > eps / 16).all() and (var[fam["c"]] < 16 * eps).all()
    assert (var[fam["d"]] == 0).all() and (c.x[fam["f"]] == 0).all() and (c.x[fam["e"]].max(1) > 2.9e4).all()
    # a constant row whose H c is exact (H a power of two) and an all-zero row give round(beta), bit for bit
    want = np.broadcast_to(R.rne(c.b.astype(np.float64), c.out), (len(fam["f"]), H))
    assert np.array_equal(got[fam["f"]], want)
    if H & (H - 1) == 0:
        assert np.array_equal(got[fam["d"]], np.broadcast_to(want[0], (len(fam["d"]), H)))
    # the divisor H - 1: named where it shows, invisible where nothing cancels against beta from H = 64 (bf16) / 512 (fp16) up
    if R.hminus1_invisible(c.out, H):
        n_out = int((np.abs(c.hminus1 - c.y64)[c.nocancel] > 2 * c.bound[c.nocancel]).sum())
        print(f"  H - 1 divisor outside the bound where |y| >= |y - b|: {n_out} of {int(c.nocancel.sum())} elements")
        assert n_out == 0 and "hminus1" not in c.wrong
    else:
        assert "hminus1" in c.wrong
    # the one-pass variance: named where a row can show it, inside the bound on every element where it is not
    _onepass(c, named=dtname == "f16" and H <= 56)


def _onepass(c, named):
    n_out = R.outside(c.onepass, c.y64, c.bound)
    print(f"  one-pass variance: outside the bound on {n_out} elements ({'named' if 'onepass' in c.wrong else 'not named'})")
    assert ("onepass" in c.wrong) == named and (n_out > 0) == named


@pytest.mark.parametrize("H", R.H_LN)
def test_layernorm_fp32_layouts(H):
    """The fp32-output layouts (f32_path.hip, x3_path.hip, f16c_path.hip) on fp32 rows: u_out = 0, so every wrong reference, H - 1
    included, is outside at every width they take."""
    for layout in ("stride64", "float4"):
        if (layout == "stride64" and H % 64) or (layout == "float4" and H % 128):
            continue
        for eps in R.EPS:
            c = R.ln_case(H, "f32", eps, layout=layout)
            assert "hminus1" in c.wrong and ("onepass" in c.wrong or H > 768)
            _onepass(c, named="onepass" in c.wrong)
            _check(f"LayerNorm fp32 {layout} H {H} eps {eps}", c, c.emulate())


@pytest.mark.parametrize("path", list(R.EMBED_PATHS))
def test_embedding_layernorm_restatement(path):
    dtname, layout, out, hiddens, n_rows = R.EMBED_PATHS[path]
    for H in hiddens:
        for n in n_rows:
            for no_types in (False, True):
                c = R.embed_case(H, dtname, n, layout=layout, out=out, no_types=no_types)
                _check(f"embedding + LayerNorm{path} H {H} n_rows {n} type_ids {'NULL' if no_types else 'given'}", c, c.emulate())
                assert set(R.EMB_WRONG) - ({"type0"} if no_types else set()) <= set(c.wrong)
                assert len(c.zero_rows) >= (0 if no_types else 1), "an all-zero sum"
                assert len(np.unique(c.x, axis=0)) >= 32, "rows must not be copies of one another (16 words x 16 positions x 2 types)"
                assert (c.ids < 0).any() and (c.ids >= R.VOCAB).any() and (c.ps < 0).any() and (c.ps >= R.MAX_POS).any()
                assert (c.ts < 0).any() and (c.ts >= R.TYPE_VOCAB).any() and 0 in c.ids and R.VOCAB - 1 in c.ids
                assert "rownext" in c.wrong
                if out == "f32":
                    assert "hminus1" in c.wrong and ("onepass" in c.wrong or H > 768)
                    _onepass(c, named="onepass" in c.wrong)
                else:
                    _onepass(c, named=False)
                    assert c.exact16.sum() >= 3, "rows whose fp32 sum is exact in 16 bits (the bit-equality with tt_layernorm_*)"


# ---- GELU fits ------------------------------------------------------------------------------------------------------------------------
def test_gelu_fits_meet_their_claims_over_the_sweep():
    v32 = R.sweep_values()
    v = v32.astype(np.float64)
    ref = R.gelu64(v)
    corr = R.gelu_correction(v)
    for name, fn, rel_claim in (("gelu_erf2", R.gelu_erf2_f32, R.GELU_REL), ("gelu_erfc", R.gelu_erfc_f32, R.GELU_ERFC_REL)):
        got = fn(v32).astype(np.float64)
        err = np.abs(got - ref)
        fin = np.isfinite(err)
        tail = (v <= 0) & (corr > 1e-30)
        # gelu_erf2's claim comes with the 4 u |v| the issue grants it; gelu_erfc's is relative to the correction term outright
        slack = 4 * R.U * np.abs(v) if name == "gelu_erf2" else 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(tail, (err - slack) / corr, 0.0)
        print(f"\n{name}: max abs error {err[fin & (np.abs(v) < 1e3)].max():.3e}; max error / correction term on v <= 0"
              f"{' (less 4 u |v|)' if name == 'gelu_erf2' else ''}: {rel.max():.3e} at v = {v[np.argmax(rel)]:.4f}; "
              f"gelu(-0) = {got[np.flatnonzero((v == 0) & np.signbit(v))[0]]}")
        if name == "gelu_erfc":
            for lo, hi in ((-3, 0), (-6, -3), (-9, -6), (-12, -9)):
                print(f"  error / correction term on [{lo}, {hi}]: {rel[(v >= lo) & (v <= hi)].max():.2e}")
        assert fin.all()
        assert rel.max() <= rel_claim and (name == "gelu_erfc" or err[np.abs(v) < 1e3].max() <= R.GELU_ABS)
    with np.errstate(invalid="ignore", over="ignore"):
        print(f"  gelu_erf2(+inf, -inf, nan) = {R.gelu_erf2_f32(np.asarray([np.inf, -np.inf, np.nan], dtype=np.float32))}")
        assert np.isnan(R.gelu_erf2_f32(np.asarray([np.inf], dtype=np.float32)))[0], "inf 2^(-inf): the restatement says NaN"


@pytest.mark.parametrize("out", R.LN_TYPES)
@pytest.mark.parametrize("epi", [R.EPI_GELU, R.EPI_TANH])
def test_epilogue_sweep_restatement(epi, out):
    c = R.sweep_case(epi, out)
    got = c.emulate()
    names = ["tanhgelu", "roundacc"] if epi == R.EPI_GELU else []
    _check(f"epilogue sweep epi {epi} {out}", c, got, names)
    if epi == R.EPI_TANH and out == "bf16":
        _tanh_roundacc(c, f"sweep {out}")


def _tanh_roundacc(c, what):
    """|v| (1 - tanh^2 v) <= |tanh v|: the accumulator rounded before the tanh moves the result by at most one output rounding, never
    two bounds -- and a kernel that does it leaves the bound all the same, because its two roundings add."""
    w = c.wrong["roundacc"]
    out = c.out if hasattr(c, "out") else c.base.dtname
    n_out = R.outside(w, c.y64, c.bound)
    r = R.ratio(R.rne(w, out), c.y64, c.bound)
    print(f"  {what}: accumulator rounded before tanh: {n_out} elements two bounds away; as a kernel's output, error / bound = {r:.3f}")
    assert n_out == 0 and (r > 1.0 or what.startswith("sweep") or c.base.K > 192)


# ---- GEMM -----------------------------------------------------------------------------------------------------------------------------
GEMM_PARAMS = [(k, s) for k, shapes in R.GEMM_SHAPES.items() for s in shapes]


@pytest.mark.parametrize("dtname", R.LN_TYPES)
@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
@pytest.mark.parametrize("kernel,shape", GEMM_PARAMS, ids=[f"{k}-{m}x{n}x{kk}" for k, (m, n, kk) in GEMM_PARAMS])
def test_gemm_restatement_within_bound_wrong_references_outside(kernel, shape, family, dtname):
    M, N, K = shape
    base = R.gemm_base(family, dtname, M, N, K)
    for epi in R.gemm_epis(kernel):
        assert R.gemm_kernel(M, N, K, epi, R.MI355X_CUS) == kernel, "the shape no longer picks the intended kernel"
        c = R.gemm_checks(base, epi, R.gemm_f32(base, epi), _check)
        if epi == R.EPI_TANH and family == "gauss":
            _tanh_roundacc(c, f"GEMM {M}x{N}x{K} {dtname} gauss tanh")
    for k, (m, n, kk) in R.SWEEP_SHAPES.items():
        assert all(R.gemm_kernel(m, n, kk, e, R.MI355X_CUS) == k for e in ((R.EPI_GELU,) if k == "persistent" else (R.EPI_GELU, R.EPI_TANH))), k
    if kernel == "onetile":
        assert R.gemm_kernel(4096, 2048, 192, R.EPI_RES, R.MI355X_CUS) == "twostage", "an odd K-step count: the residual falls back"
        assert R.gemm_kernel(4096, 2048, 192, R.EPI_BIAS, R.MI355X_CUS) == "onetile"
