"""GPU: BGE-M3's multi-vector head (csrc/multivec.hip, tensor_truth_amd/multivec.py).

* ``tt_multivec_project[_f16|_f32]`` against fp64 on the element-rounded operands: tests/test_colbert_gpu.py's derivation with the
  bias term added.  ``y_k = sum_h W_kh x_h + b_k`` in fp32 (exact products of 16-bit values, any order, one more addition):
  ``|dy_k| <= (H + 1) u (a_k + |b_k|)``, ``a_k = sum_h |W_kh x_h|``, ``u = 2^-24`` -- ``(H + 2) u (...)`` for ``_f32``, whose fp32
  products are rounded too.  The norm in fp32: relative ``(dim + 4) u`` on top of ``|dy|_2 / n``.  One division, one rounding to the
  output type (unit roundoff e: 2^-8 bf16, 2^-11 fp16 with its 2^-25 subnormal half-step):
      |dv_k| <= dy_k / n + |v_k| (|dy|_2 / n + (dim + 8) u) + e |v_k| + e_abs,
  evaluated with the fp64 values, times (1 + 2^-10) for the second-order terms.
* ``tt_maxsim_wide[_f16]`` against fp64 (a float64 matmul on the device: an independent implementation).  Products of two 16-bit
  values are exact in fp32, a dot product of ``dim`` terms in any order is within ``dim u A``, ``A = max_ij sum_k |q_ik d_jk|``;
  the maximum carries that; the sum of ``q_len`` maxima adds ``q_len u`` per term: ``q_len (dim + q_len) u A`` for the sum and, divided
  by q_len with one more rounding, ``(dim + q_len + 1) u A`` for the mean -- computed from the operands, not measured.
* ``tt_m3_mix`` within ``6 u (|w_d dense| + |w_l lex| + |w_m mv|) / sum w`` of fp64.
* The fixture (tests/golden/make_m3_multivec_golden.py) through ``M3MultiVectorEncoder``, ``MultiVectorStore`` and
  ``HipM3AllRerank``: vectors, mv and all within 2 e_<type> of fp64 (DESIGN.md 4.8's factor for a second 16-bit implementation, e the
  same torch modules' own error in that type), every listed defect outside, the fp64 top-5 order, stored == encoded-in-call.

Every figure is printed before it is asserted.
"""
import math
import os

import numpy as np
import pytest
import torch

from test_modernbert_gpu import DTYPES, EPS, U, _ratio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M3 = os.path.join(GOLDEN, "m3_mv_l2")
FACTOR = 2.0
Q_LENS = [1, 15, 16, 17, 33, 128, 129, 512]
D_LENS = [0, 1, 15, 16, 17, 33, 180, 513, 2049, 8192]            # ascending: a query takes a prefix of them
_DT = list(DTYPES.values())
_IDS = list(DTYPES)


def _allowed_docs(q_len):
    """How many of D_LENS a query of q_len vectors is paired with: the 8192-row document with short queries only, the 512-row query
    with documents of up to 513 rows."""
    return len(D_LENS) if q_len <= 33 else (len(D_LENS) - 1 if q_len < 512 else len(D_LENS) - 2)


def _packed(lens, dim, dt, dev, gen):
    lens = np.asarray(lens, dtype=np.int32)
    starts = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(lens[:-1], out=starts[1:])
    v = torch.randn(max(int(lens.sum()), 1), dim, generator=gen, device=dev)
    return torch.nn.functional.normalize(v, dim=-1).to(dt), starts, lens


class _Reference:
    """fp64 scores (sum and mean) and their bounds for pairs of one set of queries and documents, each pair computed once."""

    def __init__(self, q, qs, ql, d, ds, dl):
        self.q, self.qs, self.ql, self.d, self.ds, self.dl = q.double(), qs, ql, d.double(), ds, dl
        self.dim = q.shape[1]
        self.cache = {}

    def pair(self, a, doc):
        if (a, doc) not in self.cache:
            n = int(self.ql[a])
            if self.dl[doc] == 0:
                self.cache[(a, doc)] = (0.0, 0.0, 0.0, 0.0)
            else:
                Q = self.q[self.qs[a]:self.qs[a] + n]
                D = self.d[self.ds[doc]:self.ds[doc] + self.dl[doc]]
                s = float((Q @ D.T).max(-1).values.sum())
                A = float((Q.abs() @ D.abs().T).max())
                self.cache[(a, doc)] = (s, n * (self.dim + n) * U * A, s / n, (self.dim + n + 1) * U * A)
        return self.cache[(a, doc)]

    def table(self, cand, mean):
        want = torch.zeros(cand.shape, dtype=torch.float64)
        bound = torch.zeros(cand.shape, dtype=torch.float64)
        for a in range(cand.shape[0]):
            for c in range(cand.shape[1]):
                if cand[a, c] < 0:
                    want[a, c] = -math.inf
                else:
                    r = self.pair(a, int(cand[a, c]))
                    want[a, c], bound[a, c] = (r[2], r[3]) if mean else (r[0], r[1])
        return want, bound


def _check_scores(got, want, bound, what):
    got = got.double().cpu()
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), f"{what}: a negative candidate must score -inf"
    err = (got[~inf] - want[~inf]).abs()
    ratio = _ratio(err, bound[~inf]) if err.numel() else 0.0
    print(f"\n{what}: max error / bound = {ratio:.3f} (max abs error {err.max().item() if err.numel() else 0:.3g})")
    assert ratio <= 1.0, f"{what}: error {ratio:.3g} x its bound"


# ---- MaxSim -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("n_q", [1, 3])
@pytest.mark.parametrize("dim", [128, 384, 1024])
def test_maxsim_wide_matches_fp64(dev, built_lib, dim, n_q, mean, dt):
    from tensor_truth_amd import multivec

    gen = torch.Generator(device=dev).manual_seed(100 + dim + n_q)
    d, ds, dl = _packed(D_LENS, dim, dt, dev, gen)
    groups = [[n] for n in Q_LENS] if n_q == 1 else [[1, 15, 16], [17, 33, 128], [129, 512, 16]]
    rng = np.random.default_rng(dim + n_q)
    for qlens in groups:
        q, qs, ql = _packed(qlens, dim, dt, dev, gen)
        ref = _Reference(q, qs, ql, d, ds, dl)
        allowed = [_allowed_docs(n) for n in qlens]
        # the documents every query of the group may take, in order: the NULL form
        n_c = min(allowed)
        got = multivec.maxsim_wide(q, qs.astype(np.int32), ql, d, ds, dl, n_cand=n_c, mean=bool(mean))
        cand = np.tile(np.arange(n_c, dtype=np.int32), (n_q, 1))
        _check_scores(got, *ref.table(cand, mean), f"maxsim_wide dim {dim} q_len {qlens} mean {mean} NULL {dt}")
        assert (got[:, 0] == 0).all(), "a document of length 0 scores 0"
        # candidate lists with repeats and with -1
        cand = np.stack([rng.integers(-1, allowed[a], 13) for a in range(n_q)]).astype(np.int32)
        cand[:, 3] = cand[:, 2]
        cand[0, 0] = -1
        cand[:, 5] = np.asarray(allowed) - 1                                   # (the longest document the query may take)
        got_c = multivec.maxsim_wide(q, qs.astype(np.int32), ql, d, ds, dl, cand=cand, mean=bool(mean))
        _check_scores(got_c, *ref.table(cand, mean), f"maxsim_wide dim {dim} q_len {qlens} mean {mean} lists {dt}")
        # a score does not depend on the list it travels in
        flat, listed = got.cpu(), got_c.cpu()
        for a in range(n_q):
            for c in range(cand.shape[1]):
                if 0 <= cand[a, c] < n_c:
                    assert listed[a, c].item() == flat[a, cand[a, c]].item()


@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("dim", [128, 1024])
def test_maxsim_wide_negative_maxima_and_document_ends(dev, built_lib, dim, dt):
    """Two constructed cases a wrong kernel fails: a maximum that is negative (a running maximum started at 0 returns 0), and a
    neighbour in the store whose first row is a query row (reading one row past d_len finds a perfect match)."""
    from tensor_truth_amd import multivec

    gen = torch.Generator(device=dev).manual_seed(7)
    q, qs, ql = _packed([17], dim, dt, dev, gen)
    neg = (-q[5]).repeat(16, 1)
    body, _, _ = _packed([15], dim, dt, dev, gen)
    nxt = torch.cat([q[9:10], _packed([7], dim, dt, dev, gen)[0]])
    d = torch.cat([neg, body, nxt]).contiguous()
    ds, dl = np.array([0, 16, 31], dtype=np.int64), np.array([16, 15, 8], dtype=np.int32)
    cand = np.arange(3, dtype=np.int32)[None]
    for mean in (0, 1):
        got = multivec.maxsim_wide(q, qs.astype(np.int32), ql, d, ds, dl, mean=bool(mean)).cpu()
        want, bound = _Reference(q, qs, ql, d, ds, dl).table(cand, mean)
        _check_scores(got, want, bound, f"maxsim_wide constructed dim {dim} mean {mean} {dt}")
        div = 17 if mean else 1
        Q, D0 = q.double(), neg.double()
        from_zero = float((Q @ D0.T).max(-1).values.clamp_min(0).sum()) / div
        assert float((Q[5] @ D0.T).max()) < -0.9 and abs(from_zero - want[0, 0]) > 100 * bound[0, 0]
        assert abs(got[0, 0].item() - from_zero) > bound[0, 0]
        past, _ = _Reference(q, qs, ql, d, ds, np.array([16, 16, 8], dtype=np.int32)).table(cand, mean)
        assert abs(past[0, 1] - want[0, 1]) > 100 * bound[0, 1] and abs(got[0, 1].item() - past[0, 1]) > bound[0, 1]


@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("dim", [128, 1024])
def test_maxsim_wide_finds_a_winner_wherever_it_stands(dev, built_lib, dim, dt):
    """Row j_i of the document IS query vector i, for j_i at 0, 15, 16, d_len - 1 and on both sides of every multiple of 64 (the
    rows a workgroup takes per step, multivec.DOC_STEP): every token's maximum is its own squared norm, about 1, and a row the
    kernel skips leaves a random row's maximum instead -- far outside the bound."""
    from tensor_truth_amd import multivec

    assert multivec.DOC_STEP == 64
    gen = torch.Generator(device=dev).manual_seed(23 + dim)
    for d_len in (2049, 8192):
        at = sorted({0, 15, 16, d_len - 1} | {j for m in range(64, d_len, 64) for j in (m - 1, m)})
        assert len(at) <= 512
        q, qs, ql = _packed([len(at)], dim, dt, dev, gen)
        d, ds, dl = _packed([d_len], dim, dt, dev, gen)
        d[torch.as_tensor(at, device=dev)] = q
        cand = np.zeros((1, 1), dtype=np.int32)
        ref = _Reference(q, qs, ql, d, ds, dl)
        Q, D = q.double(), d.double()
        own = (Q * Q).sum(-1)
        assert ((Q @ D.T).max(-1).values - own).abs().max().item() < 1e-12, "every token's maximum is its own row"
        others = D.clone()
        others[torch.as_tensor(at, device=dev)] = 0
        drop = float((own - (Q @ others.T).max(-1).values).min())               # what skipping one placed row costs at least
        for mean in (0, 1):
            got = multivec.maxsim_wide(q, qs.astype(np.int32), ql, d, ds, dl, mean=bool(mean))
            want, bound = ref.table(cand, mean)
            _check_scores(got, want, bound, f"maxsim_wide winners d_len {d_len} dim {dim} mean {mean} {dt}")
            cost = drop / (len(at) if mean else 1)
            print(f"  a skipped row costs at least {cost:.3g}: {cost / bound[0, 0].item():.3g} bounds")
            # (a kernel that skips one placed row is at least cost - bound from fp64: outside the bound iff cost > 2 bounds)
            assert cost > 2 * bound[0, 0].item()


@pytest.mark.parametrize("dt", _DT, ids=_IDS)
def test_mean_is_the_sum_divided_once_and_a_pair_scores_the_same_everywhere(dev, built_lib, dt):
    from tensor_truth_amd import multivec

    dim = 384
    gen = torch.Generator(device=dev).manual_seed(11)
    q, qs, ql = _packed([33, 5, 129], dim, dt, dev, gen)
    d, ds, dl = _packed([180, 33, 513, 1, 64, 2049], dim, dt, dev, gen)
    qs32 = qs.astype(np.int32)
    total = multivec.maxsim_wide(q, qs32, ql, d, ds, dl).cpu()
    mean = multivec.maxsim_wide(q, qs32, ql, d, ds, dl, mean=True).cpu()
    exact = total.double() / torch.as_tensor(ql, dtype=torch.float64)[:, None]
    off = ((mean.double() - exact).abs() / exact.abs()).max().item()
    print(f"\nmean against sum / q_len {dt}: relative difference {off:.3g} (one rounding: {U:.3g})")
    assert off <= U
    for batch, flag in ((total, False), (mean, True)):
        for a in range(3):
            for c in range(6):
                alone = multivec.maxsim_wide(q, qs32[a:a + 1], ql[a:a + 1], d, ds[c:c + 1], dl[c:c + 1], mean=flag)
                assert alone.item() == batch[a, c].item()
        # the same documents at other offsets of a store (in reverse order behind 3 filler rows), the queries behind one filler row
        order = [5, 4, 3, 2, 1, 0]
        d2 = torch.cat([torch.ones(3, dim, dtype=dt, device=dev)] + [d[ds[c]:ds[c] + dl[c]] for c in order]).contiguous()
        dl2 = dl[order]
        ds2 = 3 + np.concatenate([[0], np.cumsum(dl2[:-1])]).astype(np.int64)
        q2 = torch.cat([torch.ones(1, dim, dtype=dt, device=dev), q]).contiguous()
        moved = multivec.maxsim_wide(q2, (qs + 1).astype(np.int32), ql, d2, ds2, dl2, mean=flag).cpu()
        assert torch.equal(moved, batch[:, order])
        cand = np.asarray([[5, 0, 0, -1], [2, 2, 1, 3], [4, -1, 5, 5]], dtype=np.int32)
        listed = multivec.maxsim_wide(q, qs32, ql, d, ds, dl, cand=cand, mean=flag).cpu()
        for a in range(3):
            for c in range(4):
                assert listed[a, c].item() == (batch[a, cand[a, c]].item() if cand[a, c] >= 0 else -math.inf)


# ---- projection ---------------------------------------------------------------------------------------------------------------------
_PROJ_TYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}


@pytest.mark.parametrize("dt", list(_PROJ_TYPES.values()), ids=list(_PROJ_TYPES))
@pytest.mark.parametrize("dim", [128, 384, 1024])
@pytest.mark.parametrize("H", [128, 384, 1024])
def test_projection_matches_fp64(dev, built_lib, H, dim, dt):
    from tensor_truth_amd import multivec

    gen = torch.Generator(device=dev).manual_seed(H + dim)
    n_rows = 320
    hidden = torch.randn(n_rows, H, generator=gen, device=dev).to(dt)
    W = (torch.randn(dim, H, generator=gen, device=dev) * 0.05).to(dt)
    bias = (torch.randn(dim, generator=gen, device=dev) * 0.5).contiguous()
    out_dt = torch.float16 if dt == torch.float32 else dt
    e = EPS[out_dt]
    acc = (H + 2) if dt == torch.float32 else (H + 1)
    for n_out in (1, 17, 300):
        rows = torch.randperm(n_rows, generator=torch.Generator().manual_seed(n_out))[:n_out].numpy().astype(np.int32)
        if n_out > 1:
            rows[1] = n_rows + 5                                      # a row that does not exist gives zeros (no bias)
        if n_out > 2:
            rows[2] = -1
        got = multivec.project(hidden, W, bias, rows)
        assert got.shape == (n_out, dim) and got.dtype == out_dt
        live = torch.as_tensor((rows >= 0) & (rows < n_rows), device=dev)
        x = hidden[torch.as_tensor(np.clip(rows, 0, n_rows - 1).astype(np.int64), device=dev)].double()
        w, b = W.double(), bias.double()
        y = x @ w.T + b
        a = x.abs() @ w.abs().T + b.abs()
        n = y.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        v = y / n
        dy = acc * U * a
        bound = (dy / n + v.abs() * (dy.norm(dim=-1, keepdim=True) / n + (dim + 8) * U) + e["out"] * v.abs() + e["out_abs"]) \
            * (1 + 2.0 ** -10)
        err = (got.double() - v).abs()[live]
        ratio = _ratio(err, bound[live])
        print(f"\nprojection H {H} dim {dim} n_out {n_out} {dt}: max error / bound = {ratio:.3f} (max abs error {err.max().item():.3g})")
        assert ratio <= 1.0
        assert (got[~live].view(torch.int16) == 0).all()
        # dropping the bias is far outside the bound
        nob = x @ w.T
        nob = nob / nob.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        assert _ratio((got.double() - nob).abs()[live], bound[live]) > 100
        # a row's bits depend neither on where in the list it stands nor on what else is listed
        again = multivec.project(hidden, W, bias, rows[::-1].copy())
        assert torch.equal(again.flip(0), got)
        for i in {0, n_out - 1, n_out // 2}:
            assert torch.equal(multivec.project(hidden, W, bias, rows[i:i + 1])[0], got[i])
    # a strided hidden state (rows of a wider buffer) and a zero row
    wide = torch.zeros(n_rows, H + 64, dtype=dt, device=dev)
    wide[:, :H] = hidden
    assert torch.equal(multivec.project(wide[:, :H], W, bias, rows), got)
    zb = torch.zeros_like(bias)
    hidden[7] = 0
    assert (multivec.project(hidden, W, zb, np.asarray([7], dtype=np.int32)).view(torch.int16) == 0).all(), "y = 0 gives 0"


# ---- the three-way score -------------------------------------------------------------------------------------------------------------
def test_m3_mix_matches_fp64(dev, built_lib):
    from tensor_truth_amd import multivec

    gen = torch.Generator(device=dev).manual_seed(3)
    dense = torch.randn(7, 150, generator=gen, device=dev)
    lex = torch.randn(7, 150, generator=gen, device=dev).abs() * 20
    mv = torch.rand(7, 150, generator=gen, device=dev)
    lex[0, 3] = dense[1, 4] = mv[2, 5] = -math.inf
    inf = torch.zeros(7, 150, dtype=torch.bool)
    inf[0, 3] = inf[1, 4] = inf[2, 5] = True
    for ws in ((0.4, 0.2, 0.4), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.4, 0.2, 0), (3.0, 1e-3, 250.0)):
        got = multivec.m3_mix(dense, lex, mv, ws).cpu()
        assert torch.isneginf(got[inf]).all() and torch.isfinite(got[~inf]).all(), "-inf propagates, whatever its weight"
        wd, wl, wm = (float(np.float32(w)) for w in ws)                         # (the weights travel as fp32)
        d, l, m = (t.double().cpu()[~inf] for t in (dense, lex, mv))
        want = (wd * d + wl * l + wm * m) / (wd + wl + wm)
        bound = 6 * U * ((wd * d).abs() + (wl * l).abs() + (wm * m).abs()) / (wd + wl + wm)
        ratio = _ratio((got[~inf].double() - want).abs(), bound)
        print(f"\nm3_mix weights {ws}: max error / bound = {ratio:.3f}")
        assert ratio <= 1.0
    assert torch.equal(multivec.m3_mix(dense, lex, mv, (0, 0, 1)).cpu()[~inf], mv.cpu()[~inf]), "(0, 0, 1) returns mv bit for bit"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_refused_before_a_launch(dev, built_lib):
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    i = torch.zeros(8, dtype=torch.int32, device=dev)
    l = torch.zeros(8, dtype=torch.int64, device=dev)
    f = torch.zeros(1024, dtype=torch.float32, device=dev)
    b = torch.zeros(8, 1024, dtype=torch.bfloat16, device=dev)
    o = torch.zeros(8, 1024, dtype=torch.bfloat16, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731

    for sfx in ("", "_f16"):
        ms = getattr(lib, "tt_maxsim_wide" + sfx)
        for dim in (96, 0, 1152, -128, 160):
            assert ms(p(b), p(i), p(i), 1, p(b), p(l), p(i), None, 1, dim, 1, p(f), None) == -2
            assert f"dim={dim}".encode() in lib.tt_last_error()
        assert ms(p(b), p(i), p(i), -1, p(b), p(l), p(i), None, 1, 128, 0, p(f), None) == -1
        assert ms(p(b), p(i), p(i), 70000, p(b), p(l), p(i), None, 1, 128, 0, p(f), None) == -1
        assert ms(None, p(i), p(i), 1, p(b), p(l), p(i), None, 1, 128, 0, p(f), None) == -1
        assert ms(p(b), p(i), p(i), 1, p(b), p(l), None, None, 1, 128, 0, p(f), None) == -1
        assert ms(p(b), p(i), p(i), 1, p(b), p(l), p(i), None, 1, 128, 0, None, None) == -1
        assert b"null pointer" in lib.tt_last_error()
        assert ms(p(b), p(i), p(i), 0, p(b), p(l), p(i), None, 1, 128, 0, p(f), None) == 0      # nothing to do
    for name in ("tt_multivec_project", "tt_multivec_project_f16", "tt_multivec_project_f32"):
        pr = getattr(lib, name)
        src = f if name.endswith("_f32") else b
        for dim in (96, 0, 1152):
            assert pr(p(src), 8, 1024, 128, p(src), p(f), dim, p(i), 1, p(o), None) == -2 and f"dim={dim}".encode() in lib.tt_last_error()
        for H in (100, 0, 1152):
            assert pr(p(src), 8, 1024, H, p(src), p(f), 128, p(i), 1, p(o), None) == -2 and f"hidden={H}".encode() in lib.tt_last_error()
        assert pr(p(src), 8, 64, 128, p(src), p(f), 128, p(i), 1, p(o), None) == -1              # ld < H
        assert pr(p(src), 0, 1024, 128, p(src), p(f), 128, p(i), 1, p(o), None) == -1
        assert pr(None, 8, 1024, 128, p(src), p(f), 128, p(i), 1, p(o), None) == -1
        assert pr(p(src), 8, 1024, 128, p(src), None, 128, p(i), 1, p(o), None) == -1
        assert pr(p(src), 8, 1024, 128, p(src), p(f), 128, p(i), 1, None, None) == -1
        assert pr(p(src), 8, 1024, 128, p(src), p(f), 128, p(i), 0, p(o), None) == 0             # nothing to do
    mix = lib.tt_m3_mix
    for ws in ((0.0, 0.0, 0.0), (-1.0, 1.0, 1.0), (1.0, 1.0, -0.5), (float("nan"), 1.0, 1.0), (float("inf"), 1.0, 1.0)):
        assert mix(p(f), p(f), p(f), 8, *ws, p(f), None) == -1 and b"tt_m3_mix" in lib.tt_last_error()
    assert mix(None, p(f), p(f), 8, 0.4, 0.2, 0.4, p(f), None) == -1
    assert mix(p(f), p(f), p(f), -1, 0.4, 0.2, 0.4, p(f), None) == -1
    torch.cuda.synchronize(dev)


# ---- the fixture --------------------------------------------------------------------------------------------------------------------
PRECISIONS = {"bf16": "bf16", "fp16": "fp16", "reference": "fp16"}      # precision -> the type whose e bounds it


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(GOLDEN, "m3_mv_l2_expected.npz"))


@pytest.fixture(scope="module")
def embedders(dev, built_lib):
    from tensor_truth_amd.embedding import HipHuggingFaceEmbedding

    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = HipHuggingFaceEmbedding(model_name=M3, device="cuda:0", model_kwargs={"precision": precision})
        return cache[precision]

    return get


def _texts(z):
    n_q = int(z["n_queries"])
    texts = [str(t) for t in z["texts"]]
    return texts[:n_q], texts[n_q:]


def _listed_defects(z, key):
    only16 = {str(d) for d in z["defects_fp16_only"]}
    return [str(d) for d in z["defects"] if key == "fp16" or str(d) not in only16]


def _nodes(passages):
    from tensor_truth_amd.schema import NodeWithScore, TextNode

    return [NodeWithScore(node=TextNode(text=t, id_=f"p{i}"), score=0.0) for i, t in enumerate(passages)]


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_fixture_vectors_and_scores_within_2e_of_fp64(dev, built_lib, expected, embedders, precision):
    from tensor_truth_amd import lexical, multivec

    z, key = expected, PRECISIONS[precision]
    emb = embedders(precision)
    queries, passages = _texts(z)
    n_q, n_d = len(queries), len(passages)
    before = emb.get_text_embedding_batch(passages[:5] + queries[:1])
    enc = multivec.M3MultiVectorEncoder(emb)
    assert enc.dim == 128 and enc.mv_w.dtype == emb._encoder.path.hidden and enc.mv_b.dtype == torch.float32
    want_dt = torch.bfloat16 if precision == "bf16" else torch.float16
    q_dense, q_lw, q_tv = enc.encode(queries, is_query=True)
    d_dense, d_lw, d_tv = enc.encode(passages, is_query=False)
    assert q_tv.vectors.dtype == want_dt and d_tv.vectors.dtype == want_dt
    assert emb.get_text_embedding_batch(passages[:5] + queries[:1]) == before, "the embedder's own output changed"
    # the lexical and dense parts are M3Encoder's bits
    plain = lexical.M3Encoder(emb)
    pq_dense, pq_lw = plain.encode(queries, is_query=True)
    pd_dense, pd_lw = plain.encode(passages, is_query=False)
    assert torch.equal(pq_dense, q_dense) and torch.equal(pd_dense, d_dense)
    assert pq_lw.as_dicts() == q_lw.as_dicts() and pd_lw.as_dicts() == d_lw.as_dicts()
    # len - 1 vectors per text; token ids give what the strings give, in any batch
    lens = z["lens"].astype(np.int64)
    assert q_tv.lens.tolist() == (lens[:n_q] - 1).tolist() and d_tv.lens.tolist() == (lens[n_q:] - 1).tolist()
    off = np.concatenate([[0], np.cumsum(lens)])
    seqs = [z["ids"][off[i]:off[i + 1]].tolist() for i in range(len(lens))]
    d2, lw2, tv2 = enc.encode(seqs[n_q + 3:n_q + 9], is_query=False)
    lo, hi = int(d_tv.starts[3]), int(d_tv.starts[9])
    assert torch.equal(d2, d_dense[3:9]) and lw2.as_dicts() == d_lw.as_dicts()[3:9] and torch.equal(tv2.vectors, d_tv.vectors[lo:hi])
    _, _, tv1 = enc.encode(passages[7:8], is_query=False)
    assert torch.equal(tv1.vectors, d_tv.vectors[int(d_tv.starts[7]):int(d_tv.starts[8])]), "alone or in a batch: the same bits"

    e = {q: float(z[f"e_{q}_{key}"]) for q in ("vec", "mv", "all")}
    vec = torch.cat([q_tv.vectors, d_tv.vectors]).double().cpu().numpy()
    store = multivec.MultiVectorStore(128, want_dt, dev, capacity_tokens=16, capacity_docs=2)          # (grows by doubling)
    store.add(list(range(n_d)), d_tv.vectors, d_tv.lens)
    assert store.nbytes >= 2 * 128 * int(d_tv.lens.sum()) + 12 * n_d and len(store) == n_d
    every = np.tile(np.arange(n_d, dtype=np.int32), (n_q, 1))
    mv_t = store.score(q_tv, every, mean=True)
    total = store.score(q_tv, every).double().cpu().numpy()
    lstore = lexical.LexicalStore(128, dev)
    lstore.add(list(range(n_d)), d_lw, d_dense)
    lex_t, dense_t, _ = lstore.score(q_lw, every, dense=q_dense, hybrid_weights=(1, 1))
    w = tuple(float(v) for v in z["m3_weights"])
    all_t = multivec.m3_mix(dense_t, lex_t, mv_t, w)
    got = {"vec": vec, "mv": mv_t.double().cpu().numpy(), "all": all_t.double().cpu().numpy()}
    err = {q: float(np.abs(got[q] - z[q]).max()) for q in got}
    print(f"\nfixture {precision}: max |hip - fp64| {err}; 2 e_{key} " + str({q: FACTOR * v for q, v in e.items()}))
    for q in got:
        assert err[q] <= FACTOR * e[q], f"{q}: {err[q]:.5g} > 2 e = {FACTOR * e[q]:.5g}"
    assert np.abs(total / (lens[:n_q, None] - 1) - got["mv"]).max() <= 2 * U * 1.0, "the mean is the sum over the vector count"
    for dn in _listed_defects(z, key):
        d = np.load(os.path.join(GOLDEN, f"m3_mv_l2_defect_{dn}.npz"))
        gap = {q: float(np.abs(got[q] - d[q]).max()) for q in d.files}
        print(f"  defect {dn}: max |hip - defect| {gap}")
        for q, g in gap.items():
            assert g > FACTOR * e[q], f"defect {dn}: {q} is within 2 e of the implementation"
    assert (np.argsort(-got["all"], 1)[:, :5] == np.argsort(-z["all"], 1)[:, :5]).all(), "the fp64 top-5 order"


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_fixture_postprocessor_and_stores(dev, built_lib, expected, embedders, precision):
    from tensor_truth_amd import lexical, multivec
    from tensor_truth_amd.schema import QueryBundle

    z, key = expected, PRECISIONS[precision]
    queries, passages = _texts(z)
    emb = embedders(precision)
    w = tuple(float(v) for v in z["m3_weights"])
    make = lambda weights, top_n=5: multivec.HipM3AllRerank(model=M3, top_n=top_n, model_kwargs={"m3_weights": weights, "embedder": emb})  # noqa: E731
    with pytest.raises(ValueError, match="m3_weights"):
        multivec.HipM3AllRerank(model=M3, model_kwargs={"embedder": emb})
    stored, fresh, mixed = make(w, 24), make(w, 24), make(w)
    assert stored.index_nodes(_nodes(passages)) == 24 and mixed.index_nodes(_nodes(passages)[::2]) == 12
    assert len(list(stored.model.parameters())) > 10 and stored.vectors.nbytes > 0 and len(stored.vectors) == 24 and len(stored.store) == 24
    e_all = float(z[f"e_all_{key}"])
    worst = 0.0
    for qi, q in enumerate(queries):
        ranked = stored.postprocess_nodes(_nodes(passages), QueryBundle(query_str=q))
        assert [n.score for n in ranked] == sorted((n.score for n in ranked), reverse=True) and isinstance(ranked[0].score, float)
        a = {n.node.id_: n.score for n in ranked}
        b = {n.node.id_: n.score for n in fresh.postprocess_nodes(_nodes(passages), query_str=q)}
        assert a == b, "a stored node and one encoded in the call score different bits"
        top = mixed.postprocess_nodes(_nodes(passages), QueryBundle(query_str=q))
        assert len(top) == 5 and [n.node.id_ for n in top] == [f"p{i}" for i in np.argsort(-z["all"][qi])[:5]], "the fp64 top-5 order"
        assert [n.score for n in top] == [a[n.node.id_] for n in top]
        worst = max(worst, max(abs(a[f"p{i}"] - z["all"][qi, i]) for i in range(24)))
    print(f"\npostprocessor {precision}: max |all - fp64| {worst:.4g}; 2 e_all_{key} {FACTOR * e_all:.4g}")
    assert worst <= FACTOR * e_all
    assert stored.stats == {"queries": 4, "stored": 96, "encoded": 0} and fresh.stats == {"queries": 4, "stored": 0, "encoded": 96}
    assert mixed.stats == {"queries": 4, "stored": 48, "encoded": 48}
    pred = fresh.predict([(queries[1], passages[6]), (queries[1], passages[7]), (queries[2], passages[6])])
    rr = fresh.rerank(queries[1], passages[6:9], top_n=2)
    assert [r["index"] for r in rr] == [0, 1] and rr[0]["relevance_score"] == pred[0] and pred[2] < pred[1] < pred[0]

    # (w_d, w_l, 0): the hybrid scores of HipM3HybridRerank on the same texts, within the mix bound
    two = make((w[0], w[1], 0), 24)
    hyb = lexical.HipM3HybridRerank(model=M3, top_n=24, model_kwargs={"hybrid_weights": (w[0], w[1]), "embedder": emb})
    two.index_nodes(_nodes(passages))
    hyb.index_nodes(_nodes(passages))
    ratio = 0.0
    for q in queries:
        a = {n.node.id_: n.score for n in two.postprocess_nodes(_nodes(passages), query_str=q)}
        h = {n.node.id_: n.score for n in hyb.postprocess_nodes(_nodes(passages), query_str=q)}
        q_dense, q_lw = hyb.encoder.encode([q], is_query=True)
        lex, dense, _ = hyb.store.score(q_lw, np.arange(24, dtype=np.int32)[None], dense=q_dense, hybrid_weights=(w[0], w[1]))
        lex, dense = lex[0].double().cpu().numpy(), dense[0].double().cpu().numpy()
        wd, wl = float(np.float32(w[0])), float(np.float32(w[1]))
        bound = 6 * U * (np.abs(wd * dense) + np.abs(wl * lex)) / (wd + wl)
        ratio = max(ratio, max(abs(a[f"p{i}"] - h[f"p{i}"]) / bound[i] for i in range(24)))
    print(f"  (w_d, w_l, 0) against the hybrid score: max difference / mix bound = {ratio:.3f}")
    assert ratio <= 1.0

    # a removed node is never returned
    best = stored.postprocess_nodes(_nodes(passages), query_str=queries[0])[0].node.id_
    assert stored.remove_node(best) and not stored.remove_node(best) and len(stored.vectors) == 23 and len(stored.store) == 23
    others = [n for n in _nodes(passages) if n.node.id_ != best]
    again = stored.postprocess_nodes(others, query_str=queries[0])
    assert len(again) == 23 and best not in [n.node.id_ for n in again]
    q_dense, q_lw, q_tv = stored.encoder.encode(queries[:1], is_query=True)
    assert np.isneginf(stored.store.score(q_lw, [[int(best[1:])]])[0].cpu().numpy()).all(), "a removed document scores -inf"
    assert stored.vectors.lookup([best])[0] == -1
