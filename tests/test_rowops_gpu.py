"""GPU: LayerNorm and embedding + LayerNorm -- the kernels every model family runs between the embedding tables and the pooling --
against fp64 through the C ABI, on operands that are exactly representable in their type, under the first-order bound tests/mid_refs.py
derives from the operands with ``u = 2^-24`` (tests/test_mid_refs_host.py holds fp32 restatements of every lane layout to the same
bounds on the same inputs, without a GPU).

* ``tt_layernorm_bf16``, ``tt_layernorm_f16``, ``tt_layernorm_bf16_fp8`` (its bf16 output, bit-equal to tt_layernorm_bf16's): widths
  8 .. 1024 with every chunk pattern of the one-wave-per-row kernel; 1, 4, 5 and 257 rows; eps 1e-5 and 1e-12; rows that are Gaussian,
  of a large mean and a small spread, of a variance of the order of eps, constant, with one outlier of 3e4, all zero; every other
  row poisoned; eight guard rows behind the output, in the same allocation as the input; the refusals.
* ``tt_encoder_forward`` / ``_f16`` / ``_f32`` / ``_x3`` / ``_f16c`` with ``layers = 0``: the embedding sum and its LayerNorm alone,
  with ids, positions and types beyond either end of their tables, ``type_ids = NULL``, an all-zero sum, and, for the 16-bit
  paths, rows whose sum is exact in 16 bits bit-equal to ``tt_layernorm_*`` of that sum.

For every kernel a set of named wrong references (the divisor H - 1, eps outside the root, a one-pass variance, the second chunk
left out of the mean, gamma and beta of another chunk, the neighbouring row's statistics; position p + 1, type row 0, the id clamped
to the wrong end, the type table left out) lies outside the bound, and further than the bound from what the kernel gave.  Every figure
is printed before it is asserted.
"""
import ctypes

import numpy as np
import pytest
import torch

import mid_refs as R

pytestmark = pytest.mark.gpu

FILL = -7.0
GUARD = 8
LN_ENTRY = {"bf16": "tt_layernorm_bf16", "f16": "tt_layernorm_f16"}
BIG = {"bf16": 3.0e38, "f16": 65504.0}          # the largest poison a row of the type can hold


def _lib():
    from tensor_truth_amd import _lib as L

    return L.load_library()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _verdict(what, case, got, rows=None):
    """Print and assert: the kernel within the bound; every wrong reference outside it, and further than the bound from the kernel."""
    sl = slice(None) if rows is None else rows
    ref, bound = case.y64[sl], case.bound[sl]
    got = np.asarray(got, dtype=np.float64)
    r = R.ratio(got, ref, bound)
    bites = {k: R.outside(v[sl], ref, bound) for k, v in case.wrong.items()}
    apart = {k: int((np.abs(got - v[sl]) > bound).sum()) for k, v in case.wrong.items()}
    print(f"\n{what}: max error / bound = {r:.4f}; elements with a wrong reference outside the bound {bites}, apart from the kernel {apart}")
    assert np.isfinite(got).all(), what
    assert r <= 1.0, what
    assert all(bites.values()) and all(apart.values()), f"{what}: a wrong reference is inside the bound"
    return r


class _Arena:
    """Input rows, output rows and GUARD sentinel rows behind them in ONE allocation: nothing the kernel could touch is foreign."""

    def __init__(self, dev, x_t, rows, H):
        self.rows, self.H = rows, H
        self.buf = torch.full(((2 * rows + GUARD) * H,), FILL, dtype=x_t.dtype, device=dev)
        self.buf[:rows * H] = x_t[:rows, :H].reshape(-1).to(dev)
        self.inp = self.buf[:rows * H]
        self.out = self.buf[rows * H:2 * rows * H].view(rows, H)
        self.guard = self.buf[2 * rows * H:]

    def result(self):
        torch.cuda.synchronize()
        assert (self.guard.float() == FILL).all(), "the guard rows behind the output were written"
        return self.out.cpu()


def _layernorm(lib, dev, name, x_t, g_d, b_d, rows, H, eps):
    a = _Arena(dev, x_t, max(rows, 1), H)
    if name.endswith("_fp8"):
        q8 = torch.zeros(max(rows, 1) * H, dtype=torch.uint8, device=dev)
        q8s = torch.zeros(max(rows, 1), dtype=torch.float32, device=dev)
        rc = getattr(lib, name)(a.inp.data_ptr(), a.out.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), rows, H, eps, q8.data_ptr(), q8s.data_ptr(),
                                _stream(dev))
    else:
        rc = getattr(lib, name)(a.inp.data_ptr(), a.out.data_ptr(), g_d.data_ptr(), b_d.data_ptr(), rows, H, eps, _stream(dev))
    return rc, a


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("eps", R.EPS)
@pytest.mark.parametrize("dtname", R.LN_TYPES)
@pytest.mark.parametrize("H", R.H_LN)
def test_layernorm_matches_fp64(dev, built_lib, H, dtname, eps):
    lib = _lib()
    c = R.ln_case(H, dtname, eps)
    x_t = R.to_type(c.x, dtname)
    g_d, b_d = torch.from_numpy(c.g).to(dev), torch.from_numpy(c.b).to(dev)
    name = LN_ENTRY[dtname]
    rc, a = _layernorm(lib, dev, name, x_t, g_d, b_d, c.n, H, eps)
    assert rc == 0, (rc, lib.tt_last_error())
    full = a.result()
    _verdict(f"{name} H {H} eps {eps} rows {c.n}", c, full.double().numpy())
    # an all-zero row, and a constant row whose H c is exact in fp32 (H a power of two), give round(beta) bit for bit
    want = R.to_type(c.b.astype(np.float64), dtname)
    fam = {f: list(range(i, c.n, 6)) for i, f in enumerate(R.FAMILIES)}
    assert all(_bits(full[r]).equal(_bits(want)) for r in fam["f"]), "an all-zero row must give round(beta)"
    if H & (H - 1) == 0:
        assert all(_bits(full[r]).equal(_bits(want)) for r in fam["d"]), "a constant row must give round(beta)"
    # 1 row (one wave), 4 (a full workgroup), 5 (one wave more): the bits of the 257-row launch
    for n in R.N_ROWS[:-1]:
        rc, a = _layernorm(lib, dev, name, x_t, g_d, b_d, n, H, eps)
        assert rc == 0 and _bits(a.result()).equal(_bits(full[:n])), f"{n} rows give other bits than the first {n} of {c.n}"
    if dtname == "bf16":
        rc, a = _layernorm(lib, dev, "tt_layernorm_bf16_fp8", x_t, g_d, b_d, c.n, H, eps)
        assert rc == 0 and _bits(a.result()).equal(_bits(full)), "tt_layernorm_bf16_fp8's bf16 output is not tt_layernorm_bf16's"
    # row isolation: every other row replaced by NaN, then by the largest finite value: the clean rows keep their bits
    for poison in (float("nan"), BIG[dtname]):
        y_t = x_t.clone()
        y_t[1::2] = poison
        rc, a = _layernorm(lib, dev, name, y_t, g_d, b_d, c.n, H, eps)
        got = a.result()
        assert rc == 0 and _bits(got[0::2]).equal(_bits(full[0::2])), f"rows next to rows of {poison} changed"
        assert poison == poison or torch.isnan(got[1::2].float()).all(), "a row of NaN must come out as NaN"


@pytest.mark.parametrize("name", ["tt_layernorm_bf16", "tt_layernorm_f16", "tt_layernorm_bf16_fp8"])
def test_layernorm_refusals_come_before_a_launch(dev, built_lib, name):
    lib = _lib()
    dt = torch.float16 if name.endswith("f16") else torch.bfloat16
    g_d, b_d = torch.ones(1040, device=dev), torch.zeros(1040, device=dev)
    x_t = torch.ones(4, 1040, dtype=dt)
    for H in (4, 12, 1032):
        rc, a = _layernorm(lib, dev, name, x_t, g_d, b_d, 4, H, 1e-5)
        assert rc == -2 and lib.tt_last_error(), (name, H, rc)
        assert (a.result().float() == FILL).all(), "a refused call wrote"
    rc, a = _layernorm(lib, dev, name, x_t, g_d, b_d, 0, 128, 1e-5)
    assert rc == 0 and (a.result().float() == FILL).all(), "rows = 0 returns 0 and writes nothing"


# ---- embedding + LayerNorm: the five forwards with layers = 0 -----------------------------------------------------------------------------
def _forward_entry(path):
    from tensor_truth_amd.encoder import _EncW
    from tensor_truth_amd.encoder_f16c import _EncWC
    from tensor_truth_amd.encoder_f32 import _EncWF
    from tensor_truth_amd.encoder_x3 import _EncWX

    return {"": (_EncW, "tt_encoder_workspace_bytes"), "_f16": (_EncW, "tt_encoder_workspace_bytes_f16"),
            "_f32": (_EncWF, "tt_encoder_f32_workspace_bytes"), "_x3": (_EncWX, "tt_encoder_x3_workspace_bytes"),
            "_f16c": (_EncWC, "tt_encoder_f16c_workspace_bytes")}[path]


def _embed_forward(lib, dev, path, c, no_types):
    """tt_encoder_forward<path> with layers = 0 on a case's tables and ids -> hidden_out [n][H] (CPU), GUARD rows behind it checked."""
    Struct, ws_name = _forward_entry(path)
    dtname, H, n = c.dtname, c.H, c.n
    keep = [R.to_type(t, dtname).to(dev) for t in (c.word, c.pos, c.typ)] + [torch.from_numpy(c.g).to(dev), torch.from_numpy(c.b).to(dev)]
    w = Struct(hidden=H, layers=0, heads=H // 64, ffn=4 * H, vocab=R.VOCAB, max_pos=R.MAX_POS, type_vocab=R.TYPE_VOCAB, ln_eps=c.eps,
               word_emb=keep[0].data_ptr(), pos_emb=keep[1].data_ptr(), type_emb=keep[2].data_ptr(), emb_ln_g=keep[3].data_ptr(),
               emb_ln_b=keep[4].data_ptr())
    ids, ps, ts = (torch.from_numpy(v).to(dev) for v in (c.ids, c.ps, c.ts))
    start, length = torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1,), n, dtype=torch.int32, device=dev)
    need = getattr(lib, ws_name)(ctypes.byref(w), n)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
    out = torch.full((n + GUARD, H), FILL, dtype=R.DTYPES[c.out], device=dev)
    rc = getattr(lib, "tt_encoder_forward" + path)(ctypes.byref(w), ids.data_ptr(), ps.data_ptr(), None if no_types else ts.data_ptr(),
                                                   start.data_ptr(), length.data_ptr(), 1, n, n, out.data_ptr(), ws.data_ptr(), need, _stream(dev))
    assert rc == 0, (path, rc, lib.tt_last_error())
    torch.cuda.synchronize()
    assert (out[n:].float() == FILL).all(), "the guard rows behind hidden_out were written"
    return out[:n].cpu()


@pytest.mark.parametrize("path", list(R.EMBED_PATHS))
def test_embedding_layernorm_matches_fp64(dev, built_lib, path):
    lib = _lib()
    dtname, layout, out, hiddens, n_rows = R.EMBED_PATHS[path]
    for H in hiddens:
        for n in n_rows:
            for no_types in (False, True):
                c = R.embed_case(H, dtname, n, layout=layout, out=out, no_types=no_types)
                got = _embed_forward(lib, dev, path, c, no_types)
                _verdict(f"tt_encoder_forward{path} layers 0, H {H} n_rows {n} type_ids {'NULL' if no_types else 'given'}", c, got.double().numpy())
                if len(c.zero_rows):                         # the all-zero sum: round(beta)
                    want = R.rne(c.b.astype(np.float64), out)
                    assert all(np.array_equal(got[r].double().numpy(), want) for r in c.zero_rows), "an all-zero sum must give round(beta)"
                if path in ("", "_f16"):
                    # where the fp32 sum is exact in 16 bits: the bits of tt_layernorm_* on that sum
                    rows = np.flatnonzero(c.exact16)
                    assert len(rows) >= 3
                    g_d, b_d = torch.from_numpy(c.g).to(dev), torch.from_numpy(c.b).to(dev)
                    rc, a = _layernorm(lib, dev, LN_ENTRY[dtname], R.to_type(c.x[rows], dtname), g_d, b_d, len(rows), H, c.eps)
                    assert rc == 0 and _bits(a.result()).equal(_bits(got[rows])), "embedding + LayerNorm and tt_layernorm_* of the same sum differ"
