"""GPU: the two SPLADE kernels through the C ABI (csrc/splade.hip), on random operands, against fp64 from the same 16-bit values.

* ``tt_splade_pool[_f16]``, ``activation`` 0.  A product of two 16-bit operands is exact in fp32; the MFMA chain adds H of them into
  an fp32 accumulator and the bias is added last: ``|out - out64| <= (H + 2) u (sum_k |t_k E_k| + |bias|)`` with ``u = 2^-24`` for a
  row, and ``|max a - max b| <= max |a - b|``, so a column is held to the largest bound among its sequence's rows.  Sequence lengths
  0, 1, 2, 63, 64, 65, 127, 128, 129 and 300 are packed into one batch at unaligned start rows (a sequence starts in the middle of a
  64-row pass and reaches into the next one or two), one sequence is cut by ``n_rows`` and one has a negative start; ``ld > H`` and
  ``ldo > Vp`` with sentinels in the padding columns.
* Max placement: the maximum of a column is planted in the first row, the last row, and on either side of each 64-row boundary of a
  130-row sequence whose every logit is negative (a maximum that starts at 0 instead of -inf shows); the fp64 reference without the
  planted row must lie outside the bound.
* Bit-identity: every sequence alone, at two other start rows and another row stride, gives the bits it gives in the batch.
* ``activation`` 1 is compared with fp64 ``log1p(max(0, .))`` of the kernel's OWN ``activation`` 0 output read back, so the activation
  alone is measured.  tests/test_tail_gpu.py grants the device's transcendental in its sigmoid heads ``4 u`` absolute on results of
  magnitude <= 1; log1p's results grow past 1, so the same slack is taken relative above 1: ``4 u max(1, |ref|)``.
* The refusals (H 96, Vp 600, max_len 0 and 8193, n_seq 65536) and confinement (a NaN row changes its own sequence only).
* ``tt_sparse_compact`` against numpy, exactly: ids, weight bits, counts and the trailing (-1, 0) slots.

Every figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16}
SEQ_LENS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 300]
SENTINEL = -7.0
UNSUPPORTED = -2


def _lib():
    from tensor_truth_amd import _lib as L

    return L.load_library()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _pool(dev, dt, t, E, bias, starts, lens, activation, ldo=None, max_len=None, n_rows=None):
    """t [rows][ld] (a CPU tensor whose first H columns are the operand), E [Vp][H], bias [Vp] -> (rc, out [n_seq][ldo] CPU)."""
    lib = _lib()
    H, Vp = E.shape[1], E.shape[0]
    ldo = Vp if ldo is None else ldo
    td, Ed, bd = t.to(dev), E.to(dev).contiguous(), bias.to(dev)
    out = torch.full((len(lens), ldo), SENTINEL, dtype=torch.float32, device=dev)
    name = "tt_splade_pool" + ("_f16" if dt == torch.float16 else "")
    max_len = max(1, int(max(lens))) if max_len is None else max_len
    st, sl = _i32(starts, dev), _i32(lens, dev)        # (held in names: a temporary's memory is reused by the next allocation)
    rc = getattr(lib, name)(td.data_ptr(), t.shape[0] if n_rows is None else n_rows, t.shape[1], H, Ed.data_ptr(), bd.data_ptr(), Vp,
                            st.data_ptr(), sl.data_ptr(), len(lens), max_len, activation, out.data_ptr(), ldo, _stream(dev))
    torch.cuda.synchronize()
    return rc, out.cpu()


def _batch(H, Vp, dt, seed):
    """The packed batch of the module docstring -> (t [n_rows][H + 8] with sentinels in the padding columns, E, bias, starts, lens)."""
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    starts, row = [], 3
    for n in SEQ_LENS:
        starts.append(row)
        row += n + int(rng.integers(0, 6))
    n_rows = row + 30
    starts += [n_rows - 10, -5]                      # cut by n_rows after 10 of its 40 rows; a negative start: no rows
    lens = SEQ_LENS + [40, 20]
    t = torch.full((n_rows, H + 8), 3.0e4, dtype=dt)
    t[:, :H] = torch.randn(n_rows, H, generator=gen).to(dt)
    E = (torch.randn(Vp, H, generator=gen) * 0.1).to(dt)
    bias = torch.randn(Vp, generator=gen).to(torch.float32)
    return t, E, bias, np.asarray(starts), np.asarray(lens)


def _reference(t, E, bias, starts, lens, H, drop=None):
    """fp64 -> (ref [n_seq][Vp], bound [n_seq][Vp]); a sequence with no rows: (-inf, 0).  ``drop``: a row (relative to the sequence's
    first) left out of every maximum -- a wrong reference."""
    t64, E64, b64 = t[:, :H].double(), E.double(), bias.double()
    logits = t64 @ E64.T
    mass = t64.abs() @ E64.abs().T
    n_rows = t.shape[0]
    ref = np.full((len(lens), E.shape[0]), -np.inf)
    bound = np.zeros_like(ref)
    for b, (s, n) in enumerate(zip(starts.tolist(), lens.tolist())):
        rows = [r for r in range(s, s + n) if 0 <= r < n_rows and (drop is None or r - s != drop)] if s >= 0 else []
        if not rows:
            continue
        ref[b] = (logits[rows].max(0).values + b64).numpy()
        bound[b] = ((H + 2) * U * (mass[rows].max(0).values + b64.abs())).numpy()
    return ref, bound


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("Vp", [128, 640])
@pytest.mark.parametrize("H", [128, 1024])
def test_pool_matches_fp64_and_is_batch_invariant(dev, built_lib, H, Vp, dt):
    t, E, bias, starts, lens = _batch(H, Vp, dt, 7000 + H + Vp)
    ref, bound = _reference(t, E, bias, starts, lens, H)
    rc, out = _pool(dev, dt, t, E, bias, starts, lens, 0, ldo=Vp + 3)
    assert rc == 0
    got = out[:, :Vp].double().numpy()
    assert (out[:, Vp:] == SENTINEL).all(), "columns past Vp were written"
    empty = np.isinf(ref[:, 0])
    assert empty.tolist() == [n == 0 or s < 0 for s, n in zip(starts, lens)]
    assert (got[empty] == -np.inf).all(), "a sequence with no rows must give -inf under activation 0"
    ratio = float((np.abs(got[~empty] - ref[~empty]) / bound[~empty]).max())
    print(f"\ntt_splade_pool H {H} Vp {Vp} {dt}: max error / bound = {ratio:.3f} over {int((~empty).sum())} sequences")
    assert np.isfinite(got[~empty]).all() and ratio <= 1.0

    # activation 1 on the kernel's own activation-0 output
    rc, out1 = _pool(dev, dt, t, E, bias, starts, lens, 1, ldo=Vp + 3)
    assert rc == 0
    got1 = out1[:, :Vp].double().numpy()
    want1 = np.log1p(np.maximum(got, 0.0))             # (-inf -> 0)
    slack = 4 * U * np.maximum(1.0, np.abs(want1))
    r1 = float((np.abs(got1 - want1) / slack).max())
    print(f"  activation 1: max |out - log1p(max(0, out0))| / (4 u max(1, |ref|)) = {r1:.3f}; "
          f"in ulp of the result: {float((np.abs(got1 - want1)[want1 > 0] / np.spacing(want1[want1 > 0].astype(np.float32))).max()):.2f}")
    assert r1 <= 1.0
    assert (got1[got <= 0] == 0).all() and (got1[empty] == 0).all()
    assert (got > 0).any() and (got <= 0).any(), "the test's own inputs: both signs are needed"

    # every sequence alone, at other start rows and another row stride: identical bits
    bits = out[:, :Vp].contiguous().view(torch.int32)
    n_rows = t.shape[0]
    for b, (s, n) in enumerate(zip(starts.tolist(), lens.tolist())):
        if s < 0:
            continue
        n_in = max(0, min(n, n_rows - s))              # (the sequence that n_rows cuts keeps the rows inside)
        for shift in (5, 77):
            t1 = torch.zeros(shift + n_in + 9, H, dtype=dt)
            t1[shift:shift + n_in] = t[s:s + n_in, :H]
            rc, o1 = _pool(dev, dt, t1, E, bias, [shift], [n_in], 0, max_len=max(1, n_in))
            assert rc == 0
            assert torch.equal(o1.view(torch.int32)[0], bits[b]), f"sequence {b} (length {n}) alone at row {shift}: other bits"


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_pool_max_placement(dev, built_lib, dt):
    H, Vp, n, s = 128, 128, 130, 7
    planted = [0, 129, 63, 64, 127, 128]               # first row, last row, either side of both pass boundaries
    rng = np.random.default_rng(55)
    t = torch.from_numpy(rng.uniform(0.5, 1.0, (s + n + 4, H))).to(dt)
    E = torch.from_numpy(-rng.uniform(0.05, 0.1, (Vp, H))).to(dt)
    t[:, :len(planted)] = 0
    E[:, :len(planted)] = 0
    for j, p in enumerate(planted):                    # column v belongs to planted row planted[v % 6]
        t[s + p, j] = 1.0
        E[j::len(planted), j] = 4.0
    bias = torch.zeros(Vp)
    starts, lens = np.asarray([s]), np.asarray([n])
    ref, bound = _reference(t, E, bias, starts, lens, H)
    where = (t[s:s + n].double() @ E.double().T).argmax(0).numpy()
    assert where.tolist() == [planted[v % len(planted)] for v in range(Vp)], "the test's own inputs: the maxima are not where planted"
    assert (ref < 0).all(), "the test's own inputs: every logit must be negative"
    rc, out = _pool(dev, dt, t, E, bias, starts, lens, 0)
    assert rc == 0
    got = out.double().numpy()
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"\nmax placement {dt}: max error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    for j, p in enumerate(planted):
        wrong, _ = _reference(t, E, bias, starts, lens, H, drop=p)
        cols = np.arange(j, Vp, len(planted))
        assert (np.abs(wrong[0, cols] - ref[0, cols]) > bound[0, cols]).all(), f"the reference without row {p} is inside the bound"
        assert (np.abs(got[0, cols] - wrong[0, cols]) > bound[0, cols]).all(), f"the kernel is within the bound of a maximum without row {p}"


def test_pool_refusals(dev, built_lib):
    dt = torch.bfloat16
    t = torch.zeros(64, 1024, dtype=dt)
    bias = torch.zeros(1024)

    def rc_of(H=128, Vp=128, max_len=8, n_seq=1):
        lib = _lib()
        td, Ed, bd = t.to(dev), torch.zeros(1024, 1024, dtype=dt, device=dev), bias.to(dev)
        st, sl = _i32([0], dev), _i32([8], dev)
        out = torch.zeros(1024, dtype=torch.float32, device=dev)
        return lib.tt_splade_pool(td.data_ptr(), 64, 1024, H, Ed.data_ptr(), bd.data_ptr(), Vp, st.data_ptr(), sl.data_ptr(), n_seq, max_len,
                                  0, out.data_ptr(), 1024, _stream(dev))

    assert rc_of() == 0
    for kw in (dict(H=96), dict(Vp=600), dict(max_len=0), dict(max_len=8193), dict(n_seq=65536), dict(H=1152), dict(Vp=65664)):
        assert rc_of(**kw) == UNSUPPORTED, kw
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
def test_pool_nan_row_stays_in_its_sequence(dev, built_lib, dt):
    H, Vp = 128, 640
    t, E, bias, starts, lens = _batch(H, Vp, dt, 99)
    _, clean = _pool(dev, dt, t, E, bias, starts, lens, 1)
    b = SEQ_LENS.index(65)
    dirty = t.clone()
    dirty[starts[b] + 64, :H] = float("nan")
    _, got = _pool(dev, dt, dirty, E, bias, starts, lens, 1)
    others = [i for i in range(len(lens)) if i != b]
    assert torch.equal(got[others].view(torch.int32), clean[others].view(torch.int32)), "a NaN row changed another sequence"


# ---- tt_sparse_compact ---------------------------------------------------------------------------------------------------------------
def _compact_reference(row, V, max_terms):
    ids = np.flatnonzero(row[:V] > 0)                  # (NaN > 0 is false; a denormal is > 0)
    if len(ids) > max_terms:
        order = np.lexsort((ids, -row[ids].astype(np.float64)))      # weight descending, then id ascending
        ids = np.sort(ids[order[:max_terms]])
    return ids.astype(np.int32), row[ids]


def _compact_rows(V, ldw, max_terms, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for count in sorted({0, 1, min(max_terms, V), min(max_terms + 1, V)}):
        row = -rng.random(ldw).astype(np.float32)
        row[rng.choice(V, count, replace=False)] = rng.uniform(0.1, 3.0, count).astype(np.float32)
        rows.append(row)
    # ties at the cut: positive values from a set of four, on more than max_terms ids where the vocabulary has that many
    row = np.zeros(ldw, dtype=np.float32)
    many = min(V, max_terms + max(3, max_terms // 2))
    row[rng.choice(V, many, replace=False)] = rng.choice(np.asarray([0.25, 0.5, 1.0, 2.0], dtype=np.float32), many)
    rows.append(row)
    # NaN, -0.0, denormals (positive ones are kept), +inf and negatives, everywhere
    row = rng.choice(np.asarray([np.nan, -0.0, 0.0, 1e-42, -1e-42, 1e-39, np.inf, -np.inf, -1.0, 0.75], dtype=np.float32), ldw)
    rows.append(row)
    w = np.stack(rows)
    w[:, V:] = 5.0                                      # positive values in the padding ids: never emitted
    return w


@pytest.mark.parametrize("max_terms", [1, 512, 8192])
@pytest.mark.parametrize("V,ldw", [(1, 8), (600, 640), (65536, 65536)])
def test_sparse_compact_matches_numpy(dev, built_lib, V, ldw, max_terms):
    from tensor_truth_amd import splade

    w = _compact_rows(V, ldw, max_terms, 31 * V + max_terms)
    terms, weights, nnz = splade.sparse_compact(torch.from_numpy(w).to(dev), V, max_terms)
    torch.cuda.synchronize()
    terms, weights, nnz = terms.cpu().numpy(), weights.cpu().numpy(), nnz.cpu().numpy()
    counts = []
    for b, row in enumerate(w):
        ids, vals = _compact_reference(row, V, max_terms)
        k = len(ids)
        counts.append(k)
        assert int(nnz[b]) == k, f"row {b}: nnz {int(nnz[b])}, numpy keeps {k}"
        assert np.array_equal(terms[b, :k], ids), f"row {b}: other ids"
        assert np.array_equal(weights[b, :k].view(np.int32), vals.view(np.int32)), f"row {b}: other weight bits"
        assert (np.diff(terms[b, :k]) > 0).all() and (terms[b, :k] < V).all()
        assert (terms[b, k:] == -1).all() and (weights[b, k:].view(np.int32) == 0).all(), f"row {b}: slots past nnz must hold (-1, 0)"
    print(f"\ntt_sparse_compact V {V} max_terms {max_terms}: kept {counts}")
    assert counts[0] == 0 and max(counts) == min(V, max_terms)


def test_sparse_compact_refusals(dev, built_lib):
    lib = _lib()
    w = torch.zeros(2, 640, device=dev)
    t = torch.zeros(2, 8192, dtype=torch.int32, device=dev)
    x = torch.zeros(2, 8192, device=dev)
    n = torch.zeros(2, dtype=torch.int32, device=dev)
    call = lambda V, mt: lib.tt_sparse_compact(w.data_ptr(), 640, V, 2, mt, t.data_ptr(), x.data_ptr(), n.data_ptr(), _stream(dev))  # noqa: E731
    assert call(600, 8) == 0
    for V, mt in ((0, 8), (65537, 8), (600, 0), (600, 8193)):
        assert call(V, mt) == UNSUPPORTED, (V, mt)
    torch.cuda.synchronize()
