"""CPU: the helper of tests/test_tail_gpu.py (tests/tail_refs.py) on the inputs the GPU tests use.

* An fp32 numpy restatement of each kernel's arithmetic (sequential fp32 accumulation in the kernel's order, the wave's butterfly)
  stays within the bound of the fp64 reference: the bounds are not too tight before a GPU is involved.
* Every named wrong reference lies outside the bound (further than twice the bound from the fp64 result) on at least one element of
  every parametrised case.
* The divisor ``len + 1`` is invisible behind an L2 normalisation (tail_refs' docstring) and outside the bound in ModernBERT's head.

Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

import tail_refs as T

POOL_TYPES = ["bf16", "f16", "f32"]


def _check(what, case, got, ref=None, bound=None, wrong=None):
    ref = (case.y64 if hasattr(case, "y64") else case.logit64) if ref is None else ref
    bound = case.bound if bound is None else bound
    wrong = case.wrong if wrong is None else wrong
    r = T.ratio(got, ref, bound)
    bites = {k: T.outside(v, ref, bound) for k, v in wrong.items()}
    print(f"\n{what}: max error / bound = {r:.4f}; elements on which a wrong reference is outside the bound {bites}")
    assert np.isfinite(np.asarray(got)).all()
    assert r <= 1.0, what
    assert all(v > 0 for v in bites.values()), f"{what}: a wrong reference is inside the bound on these inputs: {bites}"
    return r


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("dtname", POOL_TYPES)
@pytest.mark.parametrize("H", T.H_ROW)
def test_pooling_restatements_within_bound_wrong_references_outside(H, dtname, pad):
    x = T.pool_inputs(H, dtname, pad, 100 + H + pad)
    assert x.n == 257 and x.starts[T.EMPTY] > 0 and x.lens[T.EMPTY] == 0 and set(T.MEAN_LENS) <= set(x.lens.tolist())
    assert 0 in x.rows and x.n_rows - 1 in x.rows and len(set(x.rows.tolist())) < len(x.rows) and (np.diff(x.rows) < 0).any()
    cases = [T.cls_case(x, f32=dtname == "f32"), T.mean_case(x)] + ([T.last_case(x)] if dtname != "f32" else [])
    for c in cases:
        got = c.emulate()
        _check(f"{c.kind} pooling H {H} {dtname} ld H+{pad}", c, got)
        for n in T.N_SEQ:                                    # every prefix the GPU test runs has every wrong reference outside
            bites = {k: T.outside(v[:n], c.y64[:n], c.bound[:n]) for k, v in c.wrong.items()}
            assert all(bites.values()), (c.kind, n, bites)
    mean, last = cases[1], cases[-1]
    assert (mean.y64[T.EMPTY] == 0).all() and (mean.y64[T.ZEROS] == 0).all() and (mean.emulate()[[T.EMPTY, T.ZEROS]] == 0).all()
    if dtname != "f32":
        assert (last.y64[T.EMPTY] == 0).all() and (last.y64[T.ZEROS] == 0).all()
    # the bound is operand-driven: the sequence whose rows nearly cancel has a bound far above the others'
    rel = (mean.bound.sum(1) / np.maximum(np.abs(mean.y64).sum(1), 1e-300))
    print(f"  mean bound / |y|: cancelling sequence {rel[T.CANCEL]:.2e}, length-65 sequence {rel[4]:.2e}")
    assert rel[T.CANCEL] > 20 * rel[4]
    # a divisor of len + 1 gives the same unit vector
    assert T.outside(mean.invisible, mean.y64, mean.bound) == 0 and T.ratio(mean.invisible, mean.y64, mean.bound) < 1e-3


@pytest.mark.parametrize("dtname", POOL_TYPES)
def test_mean_pooling_of_8192_rows(dtname):
    x = T.pool_inputs(1024, dtname, 8, 7, long=True)
    assert 8192 in x.lens.tolist() and x.n == 12
    c = T.mean_case(x)
    _check(f"mean pooling of 8192 rows {dtname}", c, c.emulate())
    b = x.lens.tolist().index(8192)
    assert all(T.outside(v[b], c.y64[b], c.bound[b]) for v in c.wrong.values()), "the long sequence alone shows every wrong reference"


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("dtname", ["bf16", "f16"])
@pytest.mark.parametrize("H", T.H_ROW)
def test_score_head_restatement(H, dtname, pad):
    c = T.score_case(H, dtname, pad, 200 + H)
    got = c.emulate()
    _check(f"score head H {H} {dtname} ld H+{pad}", c, got)
    first = np.abs(c.logit64[:8])
    print(f"  |logits| of the constructed rows {first.round(3).tolist()}")
    assert (first[:2] < 0.1).all() and (first[2:4] > 10).all() and (first[2:4] < 40).all() and (first[4:] > 90).all()
    for n in T.N_SEQ:
        assert all(T.outside(v[:n], c.logit64[:n], c.bound[:n]) for v in c.wrong.values()), n
    _sigmoid(got)


def _sigmoid(logits):
    s = T.sigmoid_f32(logits)
    err = float(np.abs(s.astype(np.float64) - T.sigmoid64(np.asarray(logits, dtype=np.float32))).max())
    print(f"  sigmoid: max |score - sigmoid64(logit)| = {err / T.U:.2f} u")
    assert np.isfinite(s).all() and (s >= 0).all() and (s <= 1).all() and err <= 4 * T.U


def test_sigmoid_restatement_at_the_extremes():
    _sigmoid(np.asarray([0.0, 1e-3, -1e-3, 20.0, -20.0, 88.0, -88.0, 95.0, -95.0, 104.0, -104.0, 300.0, -300.0, 1e30, -1e30], dtype=np.float32))


@pytest.mark.parametrize("n_seq", T.N_SEQ_RERANK)
@pytest.mark.parametrize("dtname", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("H", T.H_HEAD)
def test_rerank_head_restatement(H, dtname, n_seq):
    c = T.rerank_case(H, dtname, n_seq, 300 + H + n_seq)
    assert c.n_pad % 128 == 0 and c.n_pad - n_seq < 128 and (n_seq < 2 or (c.rows[0] == c.n_rows - 1 and c.rows[1] == 0))
    tight = T.rerank_tight(c, T.host_gemm)
    got = T.head_out_f32(c, tight.t)
    _check(f"rerank head (against its GEMM) H {H} {dtname} n_seq {n_seq}", tight, got)
    _check(f"rerank head (end to end) H {H} {dtname} n_seq {n_seq}", c, got)
    assert (tight.t[n_seq:] == 0).all() or (c.bd != 0).all()      # (padded rows: tanh(bias), never read by the head)


@pytest.mark.parametrize("dtname", ["bf16", "f16"])
@pytest.mark.parametrize("H", T.H_HEAD)
@pytest.mark.parametrize("model,pooling", [("deberta", 0), ("modernbert", 0), ("modernbert", 1)])
def test_pooled_head_restatement(model, pooling, H, dtname):
    c = T.pooled_head_case(model, H, dtname, pooling, 400 + H)
    assert {1, 65, 300} <= set(c.lens.tolist())
    _check(f"{model} head pooling {pooling} H {H} {dtname}", c, c.emulate())
    want = {"nottransposed", "lastinput", "lastoutputs"} | ({"nobias", "secondtoken"} if model == "deberta" else {"nonorm", "otherpool"})
    want |= {"divisor"} if pooling else {"secondtoken"}
    assert set(c.wrong) == want
