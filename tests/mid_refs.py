"""fp64 references, bounds, deliberately wrong references and fp32 restatements of the kernels every model family runs between the
embedding tables and the pooling: LayerNorm and embedding + LayerNorm (rowops.hip and its fp32, split-plane and f16c siblings) and
the epilogues of the 16-bit GEMM kernels (gemm.hip).  Shared by tests/test_rowops_gpu.py, tests/test_gemm_edges_gpu.py (the kernels)
and tests/test_mid_refs_host.py (the restatements: the bounds are not too tight, the wrong references are outside them).

Vocabulary and shape follow tests/tail_refs.py: operands exact in their type, fp64 references, ``U = 2^-24``; a *case* is a namespace
with ``y64``, ``bound`` and ``wrong`` (named fp64 results of the operation done subtly wrong, each only on the cases it is named
for); ``ratio``, ``outside`` and ``teeth`` are tail_refs' own.  ``U_OUT`` is the unit roundoff of the output: 2^-8 (bf16), 2^-11
(fp16), 0 (fp32: its rounding is one of the ``c u`` below); ``TINY`` is the absolute floor: fp16 results below 2^-14 round on the
grid of 2^-24, and an fp32 or bf16 result below 2^-126 may be flushed to zero.

LayerNorm, ``y = (x - mu) / sqrt(var + eps) g + b``, first order in u, for ANY order of the two sums (n terms carry at most
(n - 1) u of the sum of their magnitudes).  With e_i the error the row arrives with (0 for tt_layernorm_*; the two additions of the
embedding sum, ``u (|w + p| + |x|)``: 2 u |x| unless the type row cancels the first sum), m1 = mean |x|, d = x - mu:

* ``dmu = (H + 1) u m1 + mean e``                     H - 1 additions, the division by H, and what the row brings
* ``dd_i = dmu + e_i + u |d_i|``                       the subtraction
* ``dvar = (H + 3) u var + 2 mean(|d_i| (dmu + e_i))``  rounded squares, H - 1 additions, the division, ``+ eps``; d moved by dmu + e
* ``rho = dvar / (2 (var + eps)) + 4 u``               rstd, relative: the root halves it; rsqrtf or 1 / sqrtf within 2 ulp
* ``|y - y64| <= |g_i| rstd (dd_i + |d_i| rho) + 3 u (|y64_i| + |b_i|) + U_OUT |y64_i| + TINY``
                                                     two products and the addition of b (fused or not), then the output's rounding

16-bit GEMM, ``C = epi(A W^T + bias [, residual])``, fp32 accumulation in any order:  ``ev = (K + 1) u (sum_k |a_k w_k| + |bias|)``
on the pre-activation v; then

* bias (0), ReLU (7):  ``ev + U_OUT |ref|``
* residual (2):        ``ev + u |ref| + U_OUT |ref|``
* tanh (3):            ``ev + 8 u |ref| + U_OUT |ref|``       (Lipschitz 1; tanhf within 4 ulp of fp32)
* GELU (1):            ``1.13 ev + g(v) + U_OUT |ref|``; g is the claim in gemm.hip's comment on gelu_erf2: ``GELU_ABS`` absolute,
  and for v <= 0 also ``GELU_REL |v| Phi(-|v|) + 4 u |v|`` (the smaller of the two), relative to the correction term.

What no bound of this kind can see, asserted as such by the host test:
* the divisor H - 1 scales y - b by ``1 + 1 / (2 H)``: where nothing cancels against b (``|y| >= |y - b|``) that is within twice the
  output's rounding from H = 64 (bf16) and H = 512 (fp16) up.  The divisor is held where it shows: bf16 at H = 8 and 56, fp16 up to
  384, the fp32 outputs at every width -- one code path, ``/ (float)H``, at every width.
* the one-pass variance E[x^2] - mean^2 is off by u (mean / sigma)^2 / 2 on rstd, the any-order bound allows (H + 1) u mean / sigma:
  it shows only in rows with mean / sigma beyond 4 (H + 1) -- and below 1 / ((H + 1) u), where the bound says nothing at all.  A bf16 row (8 bits) never gets there behind its output's rounding, an
  fp16 row (11 bits) up to H = 56; the fp32 rows of family (b) do up to H = 768 (the window closes at
  (H + 1)^2 = 2^24 / 16; at H = 1024 it depends on the rows).  It is named there, and asserted to be inside the bound on every 16-bit
  case where it is not named.
* ReLU commutes with a monotone rounding: the accumulator rounded to the output type first gives the same bits.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import tail_refs as T
from tail_refs import F32, U, f64, outside, ratio, teeth, wave_dot  # noqa: F401  (the GPU tests take them from here)

U_OUT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}
TINY = {"bf16": 2.0 ** -126, "f16": 2.0 ** -25, "f32": 2.0 ** -126}
DTYPES = T.DTYPES
H_LN = [8, 56, 128, 384, 512, 520, 768, 1024]   # one lane; seven lanes; ...; exactly 64 chunks; only lane 0 has a second; serving
N_ROWS = [1, 4, 5, 257]
EPS = [1e-5, 1e-12]
FAMILIES = "abcdef"                              # row r of a LayerNorm case belongs to family FAMILIES[r % 6]
EPI_BIAS, EPI_GELU, EPI_RES, EPI_TANH, EPI_RELU = 0, 1, 2, 3, 7
GELU_LIPSCHITZ = 1.13
GELU_ABS, GELU_REL = 1e-5, 7.5e-5                # the claims in gemm.hip's comment on gelu_erf2
GELU_ERFC_REL = 1e-5                             # ... and on gelu_erfc (the fit alone: 1.2e-7; evaluated in fp32: the comment)


def rne(x, dtname):
    """fp64 -> the nearest value of the type, ties to even, as fp64 (no double rounding through fp32).  fp16 saturates at +-65504
    as the kernels' stores do."""
    x = np.asarray(x, dtype=np.float64)
    p, emin = {"bf16": (8, -125), "f16": (11, -13), "f32": (24, -125)}[dtname]
    _, e = np.frexp(x)
    e = np.maximum(e, emin)
    q = np.ldexp(np.rint(np.ldexp(x, p - e)), e - p)
    if dtname == "f16":
        q = np.clip(q, -65504.0, 65504.0)
    return np.where(np.isfinite(x), q, x)


def to_type(x64, dtname):
    """fp64 values that are exact in the type -> a torch tensor of the type."""
    t = torch.from_numpy(np.ascontiguousarray(rne(x64, dtname))).to(DTYPES[dtname])
    assert np.array_equal(f64(t), rne(x64, dtname), equal_nan=True)
    return t


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------
def ln64(x, g, b, eps, variant=None):
    """LayerNorm in fp64, or one of its wrong forms."""
    H = x.shape[1]
    xs = x
    if variant == "rownext":                                 # the neighbouring row's statistics
        xs = np.roll(x, -1, axis=0)
    mu = xs[:, :512].mean(1, keepdims=True) * (min(H, 512) / H) if variant == "firstchunk" else xs.mean(1, keepdims=True)
    if variant == "onepass":                                 # E[x^2] - mean^2 in fp32
        x32 = xs.astype(F32)
        m32 = (x32.sum(1, keepdims=True, dtype=F32) / F32(H)).astype(F32)
        var = ((x32 * x32).sum(1, keepdims=True, dtype=F32) / F32(H) - m32 * m32).astype(F32).astype(np.float64)
        var = np.maximum(var, 0.0)
        mu = m32.astype(np.float64)
    else:
        var = ((xs - mu) ** 2).sum(1, keepdims=True) / (H - 1 if variant == "hminus1" else H)
    rstd = 1.0 / (np.sqrt(var) + eps) if variant == "epsoutside" else 1.0 / np.sqrt(var + eps)
    if variant == "gbchunk" and H > 512:                     # gamma and beta of the second chunk read at the first chunk's index
        g, b = g.copy(), b.copy()
        g[512:], b[512:] = g[:H - 512], b[:H - 512]
    return (x - mu) * rstd * g + b


def ln_bound(x, g, b, eps, out, e_in=None):
    """The bound of the module docstring -> (y64, bound)."""
    H = x.shape[1]
    e = np.zeros_like(x) if e_in is None else e_in
    mu = x.mean(1, keepdims=True)
    d = x - mu
    var = (d * d).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = d * rstd * g + b
    dmu = (H + 1) * U * np.abs(x).mean(1, keepdims=True) + e.mean(1, keepdims=True)
    dd = dmu + e + U * np.abs(d)
    dvar = (H + 3) * U * var + 2 * (np.abs(d) * (dmu + e)).mean(1, keepdims=True)
    rho = dvar / (2 * (var + eps)) + 4 * U
    bound = np.abs(g) * rstd * (dd + np.abs(d) * rho) + 3 * U * (np.abs(y) + np.abs(b)) + U_OUT[out] * np.abs(y) + TINY[out]
    return y, bound


LN_WRONG = ["hminus1", "epsoutside", "onepass", "firstchunk", "gbchunk", "rownext"]


def ln_rows(H, dtname, eps, n, seed):
    """n rows, exact in the type, row r of family FAMILIES[r % 6]:
    (a) Gaussian, 3 sigma + 0.5;  (b) a large mean with a small spread: 64 + {0, +-0.5, +-1} (fp16: 32 + multiples of 2^-5; fp32: of 2^-10);
    (c) a variance of the order of eps: s (1 - j 2^-8), j in {0, 1, 2} (var = 2/3 2^-16 s^2 = 1.0e-5 s^2), s = 1 at eps 1e-5 and
    2^-12 at eps 1e-12 (var 6e-13);  (d) a constant row, 3 or -0.75 (H c exact);  (e) one outlier of 3e4 among +-1;  (f) zeros."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, H))
    for r in range(n):
        fam = FAMILIES[r % 6]
        if fam == "a":
            x[r] = 3.0 * rng.standard_normal(H) + 0.5
        elif fam == "b":
            x[r] = 64 + rng.integers(-2, 3, H) * 0.5 if dtname == "bf16" else 32 + rng.integers(-8, 9, H) * 2.0 ** (-5 if dtname == "f16" else -10)
        elif fam == "c":
            x[r] = (1.0 if eps > 1e-8 else 2.0 ** -12) * (1 - rng.integers(0, 3, H) * 2.0 ** -8)
        elif fam == "d":
            x[r] = 3.0 if (r // 6) % 2 == 0 else -0.75
        elif fam == "e":
            x[r] = rng.integers(0, 2, H) * 2.0 - 1.0
            x[r, int(rng.integers(0, H))] = 3.0e4
    return rne(x, dtname)


def ln_params(H, seed):
    """gamma, beta fp32 [H]: every element its own value (a chunk read at another's index is another number), beta never 0."""
    rng = np.random.default_rng(seed + 1)
    g = (1.0 + 0.2 * rng.standard_normal(H)).astype(F32)
    b = (0.3 * rng.standard_normal(H)).astype(F32)
    b = np.where(np.abs(b) < 1e-3, F32(0.25), b).astype(F32)
    return g, b


def _ln_named(H, out, layout):
    """The wrong references named for a LayerNorm case (each must bite on at least one of its rows)."""
    names = ["epsoutside", "rownext"]
    if out == "f32" or (out == "f16" and H <= 384) or (out == "bf16" and H <= 56):
        names.append("hminus1")
    if (out == "f32" and H <= 768) or (out == "f16" and H <= 56):           # (the module docstring on what a 16-bit row cannot show)
        names.append("onepass")
    if H > 512:
        names += ["firstchunk", "gbchunk"]
    return names


def _marginal_onepass(wrong, x, g64, b64, eps, H, out, y64, bound):
    """fp32 rows beyond H = 768: the window of the module docstring is all but closed, and whether the one-pass variance leaves the
    bound depends on the rows; it is named on the cases whose rows show it (tests/test_mid_refs_host.py prints which)."""
    if out == "f32" and H > 768:
        w = ln64(x, g64, b64, eps, "onepass")
        if outside(w, y64, bound):
            wrong["onepass"] = w


@functools.lru_cache(maxsize=4)
def ln_case(H, dtname, eps, n=257, layout="chunk8", out=None):
    """tt_layernorm_* on n rows of ``ln_rows``.  ``dtname``: the input's type; ``out``: the output's (the input's by default)."""
    out = out or dtname
    x = ln_rows(H, dtname, eps, n, 1000 + H)
    g, b = ln_params(H, H)
    g64, b64 = g.astype(np.float64), b.astype(np.float64)
    y64, bound = ln_bound(x, g64, b64, eps, out)
    wrong = {k: ln64(x, g64, b64, eps, k) for k in _ln_named(H, out, layout)}
    nocancel = np.abs(y64) >= np.abs(y64 - b64)
    _marginal_onepass(wrong, x, g64, b64, eps, H, out, y64, bound)
    return SimpleNamespace(H=H, dtname=dtname, out=out, eps=eps, n=n, x=x, g=g, b=b, y64=y64, bound=bound, wrong=wrong, layout=layout,
                           hminus1=ln64(x, g64, b64, eps, "hminus1"), nocancel=nocancel, onepass=ln64(x, g64, b64, eps, "onepass"),
                           emulate=lambda: ln_f32(x, g, b, eps, layout, out))


def hminus1_invisible(out, H):
    return (out == "bf16" and H >= 64) or (out == "f16" and H >= 512)


# ---- fp32 restatements of the four lane layouts --------------------------------------------------------------------------------------
def _butterfly(acc):
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, np.arange(64) ^ off]).astype(F32)
    return acc[:, 0]


def _fma(a, b, c):
    return (a.astype(np.float64) * b + c).astype(F32)


def _float4_stats(x, H):
    """x3_path.hip / f16c_path.hip: lane l holds the float4 at 256 c + 4 l (the lanes below (H - 256 c) / 4 in a partial last chunk);
    ``s += (x + y) + (z + w)``, then ``v += (a a + b b) + (d d + e e)`` on the centred values, products fused into the pair's sum."""
    R = x.shape[0]
    xz = np.concatenate([x, np.zeros((R, 1024 + 4 - H), dtype=F32)], 1).astype(F32)
    nc = (H + 255) // 256
    q = xz[:, :1024].reshape(R, 4, 64, 4)[:, :nc]            # [R][c][lane][4]
    s = np.zeros((R, 64), dtype=F32)
    for c in range(nc):
        s = (s + ((q[:, c, :, 0] + q[:, c, :, 1]).astype(F32) + (q[:, c, :, 2] + q[:, c, :, 3]).astype(F32)).astype(F32)).astype(F32)
    mean = (_butterfly(s) / F32(H)).astype(F32)
    live = (256 * np.arange(nc)[:, None, None] + 4 * np.arange(64)[None, :, None] + np.arange(4)[None, None, :]) < H
    d = np.where(live[None], (q - mean[:, None, None, None]).astype(F32), F32(0))
    v = np.zeros((R, 64), dtype=F32)
    for c in range(nc):
        ab = _fma(d[:, c, :, 0], d[:, c, :, 0], (d[:, c, :, 1] * d[:, c, :, 1]).astype(F32))
        de = _fma(d[:, c, :, 2], d[:, c, :, 2], (d[:, c, :, 3] * d[:, c, :, 3]).astype(F32))
        v = (v + (ab + de).astype(F32)).astype(F32)
    return mean, _butterfly(v)


def ln_f32(x, g, b, eps, layout, out):
    """The LayerNorm kernels in fp32 numpy, in each layout's own order, the xor butterfly 32 .. 1 between the lanes:
    ``chunk8``   rowops.hip: lane l owns the 8-element chunks l and l + 64; plain sum, the squares rounded before the addition
                 (mul_then_add), rsqrtf;
    ``stride64`` f32_path.hip: lane l owns the elements l + 64 c; the squares fused into the sum; 1 / sqrtf;
    ``float4``   x3_path.hip and f16c_path.hip (H a multiple of 256 there): see ``_float4_stats``; 1 / sqrtf.
    The last product is fused with the addition of beta in all of them."""
    x = np.asarray(x, dtype=F32)
    R, H = x.shape
    ones = np.ones((R, H), dtype=F32)
    if layout == "float4":
        mean, vs = _float4_stats(x, H)
    else:
        mean = (wave_dot(x, ones, layout, fused=False) / F32(H)).astype(F32)
        d = (x - mean[:, None]).astype(F32)
        vs = wave_dot(d, d, layout, fused=layout == "stride64")
    rstd = (F32(1) / np.sqrt((vs / F32(H)).astype(F32) + F32(eps), dtype=F32)).astype(F32)
    t = ((x - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
    y = _fma(t, g.astype(F32), b.astype(F32))
    return rne(y.astype(np.float64), out)


# ---- embedding + LayerNorm ------------------------------------------------------------------------------------------------------------
VOCAB, MAX_POS, TYPE_VOCAB = 16, 16, 2
EMB_WRONG = ["posnext", "type0", "idclamp0", "notype"]


def embed_tables(H, dtname, seed):
    """word [16][H], pos [16][H], type [2][H], exact in the type, so that word[i] + pos[p] + type[t] lands in a row family by the word
    row: i % 4 == 0: (a) Gaussian; 1: (b) a large mean (word 64 / 32; position rows p % 4 == 1 the small spread: halves, and for the fp32 tables
    multiples of 2^-10 as in ``ln_rows``, so that a one-pass variance shows); 2: (c) 1 - j 2^-8 with a position
    row of 0 / -2^-8 (the type rows are 0 / 2^-8 and 0 / -2^-8 throughout); 3: word = -(pos[i] + type[1]) exactly (multiples of 2^-6) plus multiples of 1/4, none for i = 3: (id 3, position 3, type 1) is
    (f), the all-zero sum, and (id i, position i, type 1) a sum that is exact in 16 bits.  Position and type rows differ per row; the last word row (the clamp's target) is a Gaussian one of its own."""
    rng = np.random.default_rng(seed)
    word = np.zeros((VOCAB, H))
    pos = rne(0.25 * rng.standard_normal((MAX_POS, H)), dtname)
    typ = rng.integers(0, 2, (TYPE_VOCAB, H)) * np.asarray([[1.0], [-1.0]]) * 2.0 ** -8
    grid = 2.0 ** -8
    for p in range(MAX_POS):
        if p % 4 == 1:
            pos[p] = rng.integers(-2, 3, H) * 0.5 if dtname != "f32" else rng.integers(-8, 9, H) * 2.0 ** -10
        if p % 4 == 2:
            pos[p] = -rng.integers(0, 2, H) * grid
        if p % 4 == 3:
            pos[p] = rng.integers(-16, 17, H) * 2.0 ** -6
    for i in range(VOCAB):
        if i % 4 == 0:
            word[i] = 3.0 * rng.standard_normal(H) + 0.5
        elif i % 4 == 1:
            word[i] = 64.0 if dtname == "bf16" else 32.0
        elif i % 4 == 2:
            word[i] = 1 - rng.integers(0, 2, H) * grid
        else:
            word[i] = -(pos[i] + typ[1]) + (rng.integers(-1, 2, H) * 0.25 if i > 3 else 0.0)
    word[VOCAB - 1] = 2.0 * rng.standard_normal(H) - 0.25
    return rne(word, dtname), pos, typ


def embed_ids(n_rows, seed):
    """ids, pos, types [n_rows] int32 with the edges first: the first and the last id; ids -1 and vocab, positions -1 and max_pos,
    types -1 and type_vocab (each clamps to the nearer end); the all-zero sum (3, 3, 1); then every family at its own position."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, VOCAB, n_rows)
    pos = rng.integers(0, MAX_POS, n_rows)
    typ = rng.integers(0, TYPE_VOCAB, n_rows)
    edge = [(0, 0, 0), (VOCAB - 1, MAX_POS - 1, 1), (-1, 5, 1), (VOCAB, 6, 0), (4, -1, 1), (8, MAX_POS, 1), (12, 7, -1), (1, 9, TYPE_VOCAB),
            (3, 3, 1), (7, 7, 1), (11, 11, 1), (2, 2, 0), (6, 6, 1), (1, 1, 1), (5, 13, 0), (-7, -7, -7), (99, 99, 99), (2, 2, 1), (10, 10, 1)]
    for r, (i, p, t) in enumerate(edge):
        ids[r], pos[r], typ[r] = i, p, t
    pos[2::4] = ids[2::4]                                    # (the zero family needs its own position; family (c) its grid row)
    sel = (ids % 4 == 2) & (ids >= 0) & (ids < VOCAB)
    pos[sel] = 2 + 4 * (pos[sel] % 4)
    sel = (ids % 4 == 1) & (ids >= 0) & (ids < VOCAB)
    pos[sel] = 1 + 4 * (pos[sel] % 4)
    return ids.astype(np.int32), pos.astype(np.int32), typ.astype(np.int32)


def _clamp(v, n, low=False):
    return np.where(v < 0, 0, np.where(v >= n, 0 if low else n - 1, v))


@functools.lru_cache(maxsize=4)
def embed_case(H, dtname, n_rows, layout="chunk8", out=None, no_types=False, eps=1e-5):
    """Embedding + LayerNorm through ``tt_encoder_forward*`` with ``layers = 0``: x = (word[id] + pos[p]) + type[t], then ``ln_bound``
    with the two additions' ``u (|w + p| + |x|)``.  ``no_types``: type_ids = NULL reads type row 0."""
    out = out or dtname
    word, pos, typ = embed_tables(H, dtname, 50 + H)
    ids, ps, ts = embed_ids(n_rows, 60 + H + n_rows)
    g, b = ln_params(H, H + 7)
    g64, b64 = g.astype(np.float64), b.astype(np.float64)

    def rows(variant=None):
        i = _clamp(ids, VOCAB, low=variant == "idclamp0")
        p = _clamp(ps + (variant == "posnext"), MAX_POS)
        t = _clamp(np.zeros_like(ts) if (no_types or variant == "type0") else ts, TYPE_VOCAB)
        wp = word[i] + pos[p]
        return wp, wp + (0.0 if variant == "notype" else typ[t])

    wp, x = rows()
    y64, bound = ln_bound(x, g64, b64, eps, out, e_in=U * (np.abs(wp) + np.abs(x)))
    names = ["posnext", "idclamp0", "notype"] + ([] if no_types else ["type0"])
    wrong = {k: ln64(rows(k)[1], g64, b64, eps) for k in names}
    wrong.update({k: ln64(x, g64, b64, eps, k) for k in _ln_named(H, out, layout)})
    _marginal_onepass(wrong, x, g64, b64, eps, H, out, y64, bound)
    exact16 = (rne(x, dtname) == x).all(1) if dtname != "f32" else np.zeros(n_rows, dtype=bool)

    def emulate():
        x32 = ((word[_clamp(ids, VOCAB)].astype(F32) + pos[_clamp(ps, MAX_POS)].astype(F32)).astype(F32)
               + typ[_clamp(np.zeros_like(ts) if no_types else ts, TYPE_VOCAB)].astype(F32)).astype(F32)
        return ln_f32(x32, g, b, eps, layout, out)

    return SimpleNamespace(H=H, dtname=dtname, out=out, n=n_rows, eps=eps, word=word, pos=pos, typ=typ, ids=ids, ps=ps, ts=ts, g=g, b=b,
                           x=x, y64=y64, bound=bound, wrong=wrong, exact16=exact16, no_types=no_types, layout=layout, emulate=emulate,
                           zero_rows=np.flatnonzero((x == 0).all(1)), onepass=ln64(x, g64, b64, eps, "onepass"))


# ---- GELU -----------------------------------------------------------------------------------------------------------------------------
def _phi64(v):
    """Phi(v), accurate in the lower tail (erfc)."""
    return 0.5 * torch.special.erfc(torch.from_numpy(-np.asarray(v, dtype=np.float64) / np.sqrt(2.0))).numpy()


def gelu64(v):
    """0.5 v (1 + erf(v / sqrt 2)) = max(v, 0) - |v| Phi(-|v|), accurate relative to the correction term."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        corr = np.where(np.isinf(v), 0.0, np.abs(v) * _phi64(-np.abs(v)))
    return np.maximum(v, 0.0) - corr


def gelu_tanh64(v):
    return 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * v ** 3)))


def gelu_correction(v):
    return np.abs(v) * _phi64(-np.abs(v))


def gelu_own_error(v):
    """What gemm.hip's comment on gelu_erf2 claims, as a bound on |gelu_erf2(v) - gelu64(v)|."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tail = GELU_REL * gelu_correction(v) + 4 * U * np.abs(v)
    return np.where(v <= 0, np.minimum(GELU_ABS, tail), GELU_ABS)


_Q = [-9.697845371e-07, 4.016999810e-05, -7.211678312e-04, 7.490924560e-03, -5.142170191e-02, -4.614778757e-01, -1.149914980e+00,
      -1.000091195e+00]


def gelu_erf2_f32(x):
    """gemm.hip's gelu_erf2 in fp32: the degree-7 Horner form of log2 Phi(-u) with fused steps, exp2, ``max(x, 0) - u e`` fused.
    (numpy's exp2 stands in for v_exp_f32: 1 ulp.)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        u = np.abs(x)
        q = _fma(u, F32(_Q[0]), F32(_Q[1]))
        for c in _Q[2:]:
            q = _fma(q, u, F32(c))
        e = np.exp2(q).astype(F32)
        return _fma(-u, e, np.maximum(x, F32(0)))


_P = [0.17087277, -0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368, -1.26551223]


def gelu_erfc_f32(x):
    """gemm.hip's gelu_erfc in fp32: t = 1 / (1 + z / 2), erfc(z) = t exp(-z^2 + P(t)), ``max(x, 0) - |x| / 2 erfc``."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        ax = np.abs(x)
        z = (ax * F32(0.70710678118654752)).astype(F32)
        t = (F32(1) / _fma(F32(0.5) * np.ones_like(z), z, F32(1))).astype(F32)
        p = np.full_like(t, F32(_P[0]))
        for c in _P[1:]:
            p = _fma(p, t, F32(c))
        arg = (_fma(-z, z, p) * F32(1.4426950408889634)).astype(F32)
        e = (t * np.exp2(arg).astype(F32)).astype(F32)
        return _fma(-(F32(0.5) * ax).astype(F32), e, np.maximum(x, F32(0)))


def sweep_values():
    """The pre-activations of the epilogue sweep, fp32: every bf16 value in [-12, 12] (both zeros among them), a grid of 2^-6 on
    [-10, 10], +-1e-40, +-1e30, +-3e38, and 193 values on [-4, -1] that are 0.45 ulp of fp16 off that grid (exact in neither 16-bit
    type: an accumulator rounded before the GELU shows there, where ``ev`` is 0); padded with zeros to a multiple of 8192 columns."""
    pos = (np.arange(0x0000, 0x4141, dtype=np.uint32) << 16).view(F32)
    assert pos[-1] == 12.0
    grid = (np.arange(-640, 641) * 2.0 ** -6).astype(F32)
    special = np.asarray([1e-40, -1e-40, 1e30, -1e30, 3e38, -3e38], dtype=F32)
    tail = -(np.arange(64, 257) * 2.0 ** -6)                 # [-4, -1]: 0.45 of an fp16 ulp (2^-10 below 2, 2^-9 above) off the grid
    off = (tail - 0.45 * np.where(tail > -2, 2.0 ** -10, 2.0 ** -9)).astype(F32)
    v = np.concatenate([pos, -pos, grid, special, off])
    return np.concatenate([v, np.zeros(-len(v) % 8192, dtype=F32)])


# ---- GEMM -----------------------------------------------------------------------------------------------------------------------------
GEMM_WRONG = {EPI_BIAS: ["lastkstep", "last32", "biascol"],
              EPI_GELU: ["roundacc", "tanhgelu", "lastkstep", "last32", "biascol"],
              EPI_RES: ["roundacc", "lastkstep", "last32", "biascol", "resrow"],
              EPI_TANH: ["roundacc", "lastkstep", "last32", "biascol"],
              EPI_RELU: ["norelu", "lastkstep", "last32", "biascol"]}


def gemm_named(family, out, K, epi):
    """The wrong references named for a GEMM case.  What is left out, and why:
    * ``lastkstep`` needs a K-step before the last one;
    * the accumulator rounded before the tanh is never two bounds away (tests/test_mid_refs_host.py, ``_tanh_roundacc``), before the
      ReLU it gives the same bits, and in the integer family every result is judged by its bits (the residual epilogue's is there);
    * ``ev`` grows as (K + 1) sqrt(K) u: at K = 320 it passes the 4e-4 by which the tanh form of the GELU differs from the erf form,
      and the 2^-8 |v| gelu'(v) of a bf16-rounded accumulator; at fp16's 2^-11 that rounding is below ``ev`` from K = 32 on.  Both are
      held by the epilogue sweep, where ``ev`` is 0 (in fp16 by its values off the fp16 grid);
    * in the cancelling family v is 2^-10 of the products' mass, so ``ev`` is most of every bound: what is held there is the
      kernel, a dropped K-step and (up to K = 192) a dropped ReLU."""
    names = [k for k in GEMM_WRONG[epi] if not (k == "lastkstep" and K <= 64)]
    if family == "int":
        return ["roundacc"] if epi == EPI_RES else []
    if epi in (EPI_TANH,):
        names.remove("roundacc")
    if epi == EPI_GELU and (K > 192 or out == "f16"):
        names.remove("roundacc")
    if epi == EPI_GELU and K > 192:
        names.remove("tanhgelu")
    if family == "cancel":
        names = [k for k in names if k in ("lastkstep", "last32") or (k == "norelu" and K <= 192)]
    return names


def epi64(v, epi, res=None, tanh_gelu=False):
    if epi == EPI_GELU:
        return gelu_tanh64(v) if tanh_gelu else gelu64(v)
    if epi == EPI_RES:
        return v + res
    if epi == EPI_TANH:
        return np.tanh(v)
    if epi == EPI_RELU:
        return np.maximum(v, 0.0)
    return v


def epi_bound(v, ev, ref, epi, out):
    """The bound of the module docstring from the pre-activation v, its error bound ev and the fp64 result."""
    a = np.abs(ref)
    if epi == EPI_GELU:
        e = GELU_LIPSCHITZ * ev + gelu_own_error(v)
    elif epi == EPI_RES:
        e = ev + U * a
    elif epi == EPI_TANH:
        e = ev + 8 * U * a
    else:
        e = ev
    return e + U_OUT[out] * a + TINY[out]


def gemm_operands(family, dtname, M, N, K, seed):
    """A [M][K], W [N][K], residual [M][N] (exact in the type), bias fp32 [N], as fp64 arrays.
    ``int``:    A in {-1, 0, 1}, W integer in [-8, 8], bias an integer plus a multiple of 2^-4 (even columns small, odd columns beyond
                +-1024, where neither type holds sixteenths), the residual a multiple of 2^-8 below 1: every partial sum is exact in fp32.
    ``cancel``: columns k, k + K / 2 of W equal and of A opposite, so every pair of products cancels exactly; one pair left 2^-8 short.
    ``gauss``:  today's tests: A ~ N(0, 1), W ~ N(0, 1 / K), bias ~ 0.1 N(0, 1), residual ~ N(0, 1)."""
    rng = np.random.default_rng(seed)
    if family == "int":
        a = rng.integers(-1, 2, (M, K)).astype(np.float64)
        w = rng.integers(-8, 9, (N, K)).astype(np.float64)
        a[0, :], w[0, :] = 1.0, np.where(w[0] == 0, 3.0, w[0])          # every k carries a non-zero product
        big = (np.arange(N) % 2) * rng.choice([-1, 1], N) * rng.integers(1024, 1500, N)
        bias = big + rng.integers(-3, 4, N) + rng.integers(-15, 16, N) * 2.0 ** -4
        res = rng.integers(-255, 256, (M, N)) * 2.0 ** -8
    elif family == "cancel":
        a = rne(rng.standard_normal((M, K)), dtname)
        w = rne(rng.standard_normal((N, K)) / np.sqrt(K), dtname)
        a[:, K // 2:], w[:, K // 2:] = -a[:, :K // 2], w[:, :K // 2]
        a[:, 0], a[:, K // 2] = 1.0, -(1 - 2.0 ** -8)
        w[:, K // 2] = w[:, 0] = rne(np.clip(w[:, 0], -1 / np.sqrt(K), 1 / np.sqrt(K)), dtname)
        bias = np.zeros(N)
        res = rne(0.01 * rng.standard_normal((M, N)), dtname)
    else:
        a = rne(rng.standard_normal((M, K)), dtname)
        w = rne(rng.standard_normal((N, K)) / np.sqrt(K), dtname)
        bias = 0.1 * rng.standard_normal(N)
        res = rne(rng.standard_normal((M, N)), dtname)
    return a, w, bias.astype(F32).astype(np.float64), res


@functools.lru_cache(maxsize=1)      # (the largest is 1 GB of fp64 arrays; a test asks for its operands once or twice)
def gemm_base(family, dtname, M, N, K, seed=0):
    """Operands, the fp64 pre-activation v, ``ev`` and what the wrong references need, once per shape."""
    a, w, bias, res = gemm_operands(family, dtname, M, N, K, 7000 + seed + M + N + K)
    prod = a @ w.T
    mass = np.abs(a) @ np.abs(w).T
    v = prod + bias
    ev = (K + 1) * U * (mass + np.abs(bias))
    last64 = a[:, K - 64:] @ w[:, K - 64:].T if K > 64 else None
    last32 = a[:, K - 32:] @ w[:, K - 32:].T
    return SimpleNamespace(family=family, dtname=dtname, M=M, N=N, K=K, a=a, w=w, bias=bias, res=res, prod=prod, mass=mass, v=v, ev=ev,
                           last64=last64, last32=last32)


def gemm_case(base, epi, names=None):
    """One epilogue on a ``gemm_base``: y64, bound, the wrong references named for it (``names`` narrows them)."""
    out, v, res = base.dtname, base.v, base.res
    fin = lambda pre, **kw: rne_sat(epi64(pre, epi, res, **kw), out)  # noqa: E731
    y64 = fin(v)
    bound = epi_bound(v, base.ev, y64, epi, out)
    wrong = {}
    for k in GEMM_WRONG[epi] if names is None else names:
        if k == "roundacc":
            wrong[k] = fin(rne(v, out))
        elif k == "tanhgelu":
            wrong[k] = fin(v, tanh_gelu=True)
        elif k == "lastkstep" and base.last64 is not None:
            wrong[k] = fin(v - base.last64)
        elif k == "last32":
            wrong[k] = fin(v - base.last32)
        elif k == "biascol":
            wrong[k] = fin(base.prod + np.roll(base.bias, -4))
        elif k == "resrow":
            wrong[k] = rne_sat(v + np.roll(res, -1, axis=0), out)
        elif k == "norelu":
            wrong[k] = v
    return SimpleNamespace(base=base, epi=epi, y64=y64, bound=bound, wrong=wrong, emulate=lambda: gemm_f32(base, epi))


def rne_sat(y, out):
    """The fp16 stores saturate at +-65504: so does the reference (the bound is that of the unsaturated value)."""
    return np.clip(y, -65504.0, 65504.0) if out == "f16" else y


def gemm_f32(base, epi):
    """The 16-bit GEMM in fp32 numpy: an fp32 product (whatever order the BLAS takes), the bias, the epilogue in fp32 -- gelu_erf2's
    restatement, tanhf, fmaxf, the residual's addition -- and the output's rounding."""
    acc = (base.a.astype(F32) @ base.w.astype(F32).T).astype(F32)
    v = (acc + base.bias.astype(F32)).astype(F32)
    if epi == EPI_GELU:
        v = gelu_erf2_f32(v)
    elif epi == EPI_TANH:
        v = np.tanh(v).astype(F32)
    elif epi == EPI_RELU:
        v = np.maximum(v, F32(0))
    elif epi == EPI_RES:
        v = (v + base.res.astype(F32)).astype(F32)
    return rne(v.astype(np.float64), base.dtname)


def sweep_case(epi, out, restate=gelu_erf2_f32):
    """W = 0: the pre-activation is bias[n] exactly (ev = 0) -> the values, y64, the epilogue's own bound."""
    v32 = sweep_values()
    v = v32.astype(np.float64)
    with np.errstate(over="ignore"):
        y64 = rne_sat(epi64(v, epi), out)
        bound = epi_bound(v, 0.0, y64, epi, out)
    wrong = {"roundacc": rne_sat(epi64(rne(v, out), epi), out)}
    if epi == EPI_GELU:
        wrong["tanhgelu"] = rne_sat(gelu_tanh64(np.clip(v, -1e9, 1e9)), out)

    def emulate():
        y = restate(v32) if epi == EPI_GELU else np.tanh(v32).astype(F32)
        return rne(y.astype(np.float64), out)

    return SimpleNamespace(v32=v32, v=v, y64=y64, bound=bound, wrong=wrong, emulate=emulate, epi=epi, out=out)


# ---- which kernel the launcher picks (gemm.hip: tt_gemm_launch, launch<EPI>) ---------------------------------------------------------
def gemm_kernel(M, N, K, epi, cus):
    """'skinny' | 'staged' | 'twostage' | 'onetile' | 'persistent' | None (refused), by the rule in gemm.hip for the 16-bit operands
    of tt_gemm_bf16 / tt_gemm_f16 (lda = K, ldc = ldr = N)."""
    if 0 < M <= 256 and M % 64 == 0 and N % 16 == 0 and K % 32 == 0 and K > 0:
        return "skinny"
    if M % 128 or N % 128 or K % 64 or K <= 0:
        return None
    small_grid = (M // 256) * (N // 256) < 128
    if not small_grid and M % 256 == 0 and N % 256 == 0 and N % 8 == 0 and (epi != EPI_RES or (K // 64) % 2 == 0):
        mt, nt = M // 256, N // 256
        sn = min(4, nt)
        while 32 % sn:
            sn -= 1
        sm = 32 // sn
        blocks = (-(-mt // sm)) * (-(-nt // sn)) * 32
        blocks = (blocks + 7) // 8 * 8
        cus8 = cus // 8 * 8
        if epi == EPI_GELU and (K // 64) % 2 == 0 and K // 64 >= 2 and blocks > cus8 and cus8 >= 8:
            return "persistent"
        return "onetile"
    return "staged" if (M // 128) * (N // 128) <= cus else "twostage"


def gemm_checks(base, epi, got, check):
    """What both the restatement and the kernel are held to on one (operands, epilogue)."""
    family, out, K = base.family, base.dtname, base.K
    what = f"GEMM {base.M}x{base.N}x{K} {out} {family} epi {epi}"
    if family == "int":
        c = gemm_case(base, epi, names=tuple(gemm_named(family, out, K, epi)))
        exact = base.v + (base.res if epi == EPI_RES else 0.0)
        assert (np.abs(base.prod).max() + np.abs(base.bias).max() + 1) * 2 ** 8 < 2 ** 24, "every partial sum exact in fp32"
        assert (np.abs(base.a).sum(0) > 0).all() and (np.abs(base.w).sum(0) > 0).all(), "every k carries a non-zero product"
        inexact = float((rne(base.v, out) != base.v).mean())
        assert inexact >= 0.25, f"acc + bias representable too often ({inexact:.2f}): double rounding has nothing to bite on"
        r = ratio(got, c.y64, c.bound)
        print(f"\n{what}: max error / bound = {r:.4f}; acc + bias not representable on {inexact:.2f} of the elements")
        assert r <= 1.0, what
        if epi in (EPI_BIAS, EPI_RES, EPI_RELU):
            want = rne(rne_sat(np.maximum(exact, 0.0) if epi == EPI_RELU else exact, out), out)
            diff = int((got != want).sum())
            print(f"  elements that are not the single correct rounding of the exact value: {diff}")
            assert diff == 0, what
            if epi == EPI_RES:
                twice = int((rne(c.wrong["roundacc"], out) != want).sum())
                print(f"  elements on which a doubly rounded result has other bits: {twice}")
                assert twice > 0
        return c
    names = gemm_named(family, out, K, epi)
    c = gemm_case(base, epi, names=tuple(names + (["roundacc"] if epi == EPI_TANH else [])))
    if family == "cancel":
        rel = np.abs(base.prod) / np.maximum(base.mass, 1e-300)
        assert rel.max() <= 2.0 ** -10, f"cancelling rows: |sum a w| / sum |a w| = {rel.max():.2e}"
    check(what, c, got, names)
    if epi == EPI_RELU:
        relu_first = np.maximum(rne(base.v, out), 0.0)
        assert np.array_equal(rne(relu_first, out), rne(c.y64, out)), "ReLU commutes with the rounding: the same bits"
    return c


# ---- the cases the GPU tests run (tests/test_mid_refs_host.py walks the same lists) --------------------------------------------------
LN_TYPES = ["bf16", "f16"]
# the five forwards with layers = 0: (name suffix, table type, lane layout, output type, hidden sizes, n_rows)
EMBED_PATHS = {"": ("bf16", "chunk8", "bf16", [128, 384, 640, 1024], [64, 128]),
               "_f16": ("f16", "chunk8", "f16", [128, 384, 640, 1024], [64, 128]),
               "_f32": ("f32", "stride64", "f32", [128, 384, 640, 1024], [64, 128]),
               "_x3": ("f32", "float4", "f32", [128, 384, 640, 1024], [64, 128]),
               "_f16c": ("f32", "float4", "f32", [256, 1024], [256])}      # (that path takes hidden and n_rows in multiples of 256 only)
# shapes for the 256 CUs of an MI355X, smallest first: kernel -> [(M, N, K)]
GEMM_SHAPES = {"skinny": [(64, 16, 32), (64, 16, 96), (256, 48, 32), (256, 48, 96)],
               "staged": [(384, 128, 64), (384, 128, 128), (384, 128, 192), (384, 128, 320)],        # ring depths 1, 2, 3, 5
               "twostage": [(4224, 1024, 64), (4224, 1024, 192)],                                    # 264 tiles of 128^2
               "onetile": [(4096, 2048, 128)],                                                       # 128 tiles of 256^2
               "persistent": [(8448, 2048, 128)]}                                                    # 264 tiles > 256 CUs, GELU
GEMM_FAMILIES = ["int", "cancel", "gauss"]
GEMM_EPIS = [EPI_BIAS, EPI_GELU, EPI_RES, EPI_TANH, EPI_RELU]
SWEEP_SHAPES = {"skinny": (64, 8192, 32), "staged": (384, 8192, 64), "onetile": (2048, 8192, 128), "persistent": (2304, 8192, 128)}
MI355X_CUS = 256


def gemm_epis(kernel):
    return [EPI_GELU] if kernel == "persistent" else GEMM_EPIS
