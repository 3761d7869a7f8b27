"""The fp8 shadow prefilter (csrc/shadow.hip, ``tt_scan_topk_shadow``) where its bound is tight.

The contract is EXACT: every true top-k row satisfies ``q.d + ||q|| be >= thr`` and the result is bit-identical to ``tt_scan_topk``.
Random unit rows never come near that bound (``q.e`` ~ 0.001 against ~ 0.04), so the tests here construct the rows on which it holds
with equality, run every compiled width, shards whose row count is no multiple of 16, rows behind ``n_rows``, special values, large
norms, the overflow flag and the C ABI's refusals.  Small shards are reached as tests/test_pipeline_gpu.py reaches them
(``ScanShadow.MIN_ROWS`` patched to the C ABI's own floor, 8193)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = (128, 256, 384, 512, 640, 768, 896, 1024)
SIZES = (8193, 8200, 12_345, 32_768)       # one more than the floor, 8 mod 16, odd, a full sample
FLOOR = 8193
SENTINEL = 0xA5


def _align(x, a):
    return (x + a - 1) // a * a


def _bits(t):
    return t.contiguous().view(torch.int32)


def _e4m3(x):
    """The shadow's definition on the CPU: e4m3(clamp(256 x, +-448)), round to nearest even (NaN stays NaN)."""
    return (x.float() * 256.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def _layout(cap, dim):
    """The shadow block restated: bytes [cap][D]; be at align_up(cap D, 256); dn behind align_up(round_up(cap, 16) 4, 256)."""
    r16 = _align(cap, 16)
    off_be = _align(cap * dim, 256)
    off_dn = off_be + _align(r16 * 4, 256)
    return off_be, off_dn, off_dn + _align(r16 * 4, 256)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _lib():
    from tensor_truth_amd import _lib as L

    return L.load_library()


def _build_block(x, cap, ranges):
    """A sentinel-filled shadow block of capacity ``cap`` with the row ranges built in the order given -> its bytes on the host."""
    lib = _lib()
    dim = x.shape[1]
    total = lib.tt_scan_shadow_bytes(cap, dim)
    assert total == _layout(cap, dim)[2], (total, _layout(cap, dim))
    raw = torch.full((total + 256,), SENTINEL, dtype=torch.uint8, device=x.device)
    ptr = _align(raw.data_ptr(), 256)
    for lo, hi in ranges:
        rc = lib.tt_scan_shadow_build(x.data_ptr(), dim, lo, hi, ptr, cap, _stream(x.device))
        assert rc == 0, lib.tt_last_error()
    torch.cuda.synchronize()
    off = ptr - raw.data_ptr()
    return raw[off:off + total].cpu()


# ---- 1. tt_scan_shadow_build against the CPU ---------------------------------------------------------------------------------------------
def _build_rows(dim):
    """Rows of every kind the build kernel can meet; the first ceil(65536 / dim) rows hold every bf16 bit pattern."""
    g = torch.Generator().manual_seed(1000 + dim)
    every = torch.arange(_align(65536, dim), dtype=torch.int32).to(torch.int16).view(torch.bfloat16).view(-1, dim)     # (wraps behind 0xFFFF)
    blocks = [every]
    r = torch.randn(300, dim, generator=g)
    blocks.append((r / r.norm(dim=1, keepdim=True)).to(torch.bfloat16))                    # random unit rows
    blocks.append((torch.randn(200, dim, generator=g) * 3.0).to(torch.bfloat16))           # many elements beyond +-1.75: saturate to +-448
    blocks.append((torch.randn(200, dim, generator=g) * 2.0 ** -20).to(torch.bfloat16))    # most elements below 2^-18: flush to 0
    sub = torch.randint(1, 128, (100, dim), generator=g, dtype=torch.int32)                # bf16 subnormals of both signs
    sub = sub | (torch.randint(0, 2, (100, dim), generator=g, dtype=torch.int32) << 15)
    blocks.append(sub.to(torch.int16).view(torch.bfloat16))
    z = torch.zeros(4, dim)
    z[1] = -0.0
    z[2, ::2] = -0.0
    z[3, 1::3] = -0.0
    blocks.append(z.to(torch.bfloat16))                                                    # +-0
    inf = (torch.randn(6, dim, generator=g) * 0.1)
    inf[0, 3] = float("inf")
    inf[1, dim - 1] = float("-inf")
    inf[2, 0] = float("inf")
    inf[2, 77] = float("-inf")
    inf[3] = float("inf")
    inf[4] = float("-inf")
    inf[5, 64:96] = float("inf")
    blocks.append(inf.to(torch.bfloat16))                                                  # +-inf
    nan = (torch.randn(3, dim, generator=g) * 0.1)
    nan[0] = float("nan")
    nan[1, 5] = float("nan")
    nan[2, dim - 1] = float("nan")
    nan[2, 9] = float("inf")
    blocks.append(nan.to(torch.bfloat16))                                                  # NaN rows (a tombstone is all-NaN)
    ex = (torch.randn(300, dim, generator=g) * 256.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() / 256.0
    blocks.append(ex.to(torch.bfloat16))                                                   # e4m3-exact rows: nothing is rounded away
    edge = torch.tensor([1.75, -1.75, 1.7578125, 1.875, 2.0 ** -18, -(2.0 ** -18), 1.5 * 2.0 ** -18, 2.0 ** -17, 3 * 2.0 ** -18,
                         31 / 2048, 33 / 2048, 0.0068359375, 100.0, -100.0, 2.0 ** -19, 2.0 ** -30])
    blocks.append(edge.repeat(2, dim // 16 * 2)[:, :dim].to(torch.bfloat16))               # ties, the saturation edge, the flush edge
    blocks.append((torch.randn(4099, dim, generator=g) * 0.05).to(torch.bfloat16))         # enough rows for a split behind 4099
    return torch.cat(blocks).contiguous()


@pytest.mark.parametrize("dim", DIMS)
def test_shadow_build_matches_the_cpu_definition(dev, built_lib, dim):
    """``tt_scan_shadow_build``: bytes = e4m3(clamp(256 x, +-448)) bit for bit over EVERY bf16 value and rows of every kind; ``be`` and
    ``dn`` are upper bounds of ||x - d|| and ||d|| (fp64) and at most 1.001 x + 2e-9 above them (the kernel's x 1.0005 + 1e-9 and an fp32
    sum of <= 1024 squares); inf rows bound nothing (be = inf), NaN rows are NaN; a block built in pieces split at rows that are no
    multiples of 4 or 16 equals the block built at once, and nothing outside the built rows is written."""
    lib = _lib()
    x = _build_rows(dim)
    n = x.shape[0]
    cap = n + 37
    off_be, off_dn, total = _layout(cap, dim)
    assert lib.tt_scan_shadow_bytes(cap, dim) == total and lib.tt_scan_shadow_bytes(n, dim) == _layout(n, dim)[2]
    xd = x.to(dev)
    whole = _build_block(xd, cap, [(0, n)])
    got = whole[: n * dim].view(n, dim)
    want8 = _e4m3(x)
    want = want8.view(torch.uint8)
    isnan = x.isnan()
    wrong = (got != want) & ~isnan
    print(f"\nshadow build dim {dim}: {n} rows, {int(wrong.sum())} bytes differ from the CPU's e4m3, {int(isnan.sum())} NaN elements "
          f"with the bytes {sorted(hex(b) for b in got[isnan].unique().tolist())}")
    assert bool(((got & 0x7F) == 0x7F)[isnan].all()), "a NaN element's shadow byte is not e4m3's NaN"
    assert not bool(wrong.any()), (x[wrong][:8], got[wrong][:8], want[wrong][:8])
    # the bounds, in fp64
    d = want8.double() / 256.0
    e = x.double() - d
    ne, nd = e.norm(dim=1), d.norm(dim=1)
    be = whole[off_be: off_be + 4 * n].view(torch.float32).double()
    dn = whole[off_dn: off_dn + 4 * n].view(torch.float32).double()
    has_nan = isnan.any(dim=1)
    has_inf = x.isinf().any(dim=1) & ~has_nan
    finite = ~has_nan & ~has_inf
    moderate = finite & (x.float().abs().amax(dim=1) < 1e15)          # (beyond that an fp32 sum of squares overflows: be = inf, still a bound)
    assert bool(be[has_nan].isnan().all()) and bool(dn[has_nan].isnan().all())
    assert bool((be[has_inf] == float("inf")).all()) and bool((dn[has_inf] >= nd[has_inf]).all()) and bool(dn[has_inf].isfinite().all())
    lo_be, lo_dn = (be - ne)[finite].min(), (dn - nd)[finite].min()
    hi_be = (be - (1.001 * ne + 2e-9))[moderate].max()
    hi_dn = (dn - (1.001 * nd + 2e-9))[moderate].max()
    ratio = (be / ne)[moderate & (ne > 1e-6)]
    print(f"  min (be - ||e||) {float(lo_be):.3e}, min (dn - ||d||) {float(lo_dn):.3e}; max (be - 1.001 ||e|| - 2e-9) {float(hi_be):.3e}, "
          f"max (dn - 1.001 ||d|| - 2e-9) {float(hi_dn):.3e}; be / ||e|| in [{float(ratio.min()):.6f}, {float(ratio.max()):.6f}]")
    assert lo_be >= 0 and lo_dn >= 0, "be / dn must be rounded UP"
    assert hi_be <= 0 and hi_dn <= 0
    # built in pieces: the same block, byte for byte (be and dn included)
    for cuts in ([0, 4099, n], [0, 1, 4099, 4102, n - 5, n]):
        pieces = _build_block(xd, cap, list(zip(cuts, cuts[1:])))
        assert torch.equal(pieces, whole), cuts
    reverse = _build_block(xd, cap, [(4099, n), (0, 4099)])
    assert torch.equal(reverse, whole)
    # only the built rows are written
    lo, hi = 5, n - 3
    part = _build_block(xd, cap, [(lo, hi)])
    touched = torch.zeros(total, dtype=torch.bool)
    touched[lo * dim: hi * dim] = True
    touched[off_be + 4 * lo: off_be + 4 * hi] = True
    touched[off_dn + 4 * lo: off_dn + 4 * hi] = True
    assert bool((part[~touched] == SENTINEL).all()), "bytes outside the built range were written"
    assert torch.equal(part[touched], whole[touched])
    assert bool((whole[n * dim: off_be] == SENTINEL).all()) and bool((whole[off_be + 4 * n: off_dn] == SENTINEL).all())
    assert bool((whole[off_dn + 4 * n:] == SENTINEL).all())


# ---- 2. rows on which the Cauchy-Schwarz bound holds with equality ---------------------------------------------------------------------
# Per coordinate j_i in {0..3} and a sign s_i; u_i = s_i 2^j_i.  Query q = u / 8; row(m) = m u / 2048:
#   m = 33 (tight):  256 c_i = 4.125 2^j_i rounds DOWN to 4 2^j_i, so e = c - d = u / 2048 is parallel to q: q.c - q.d = ||q|| ||e||
#   m = 31 (decoy):  256 c_i = 3.875 2^j_i rounds UP (tie to even) to the SAME byte; its true score is 31/33 of the tight row's
#   m in STRONG:     larger scores (36 .. 48: e4m3-exact; 66: twice the tight row)
# Everything is bf16-exact, every product q_i c_i is a multiple of 2^-14 and every sum of them stays below 2^10, so fp32 accumulates
# them exactly in ANY order: thr and the scores do not depend on the MFMA's order.
TIGHT, DECOY, STRONG = 33, 31, (66, 36, 40, 44, 48)
N_DECOYS = 33


def _exact_in_fp32(q, rows, lsb_log2, what):
    prod = q.unsqueeze(0) * rows
    scaled = prod * 2.0 ** -lsb_log2
    assert torch.equal(scaled, scaled.round()), f"{what}: a product is no multiple of 2^{lsb_log2}"
    top = float(prod.abs().sum(dim=1).max())
    assert top < 2.0 ** (lsb_log2 + 24), f"{what}: sum |products| {top} does not fit fp32 at an lsb of 2^{lsb_log2}"
    return top


class _TightShard:
    """``n`` x ``dim`` bf16 rows on the device with, per query t, the tight row at ``tight_rows[t]`` as the k-th best, k - 1 stronger
    rows in 32-row groups of their own (so the sample's k-th best group maximum, thr, IS the tight row's score), N_DECOYS decoys and
    random rows of norm 1/2 everywhere else.  Every condition that gives the test its teeth is asserted here, in fp64 on the CPU."""

    def __init__(self, dev, dim, n, k, tight_rows, seed):
        self.dim, self.n, self.k, self.nq = dim, n, k, len(tight_rows)
        nq = self.nq
        g = torch.Generator().manual_seed(seed)
        j = torch.randint(0, 4, (nq, dim), generator=g)
        sg = torch.randint(0, 2, (nq, dim), generator=g) * 2 - 1
        self.u = (sg * 2.0 ** j).double()
        self.q = self.u / 8.0
        assert len(set(tight_rows)) == nq and all(0 <= r < n for r in tight_rows)
        self.tight = list(tight_rows)
        used = set(tight_rows)
        n_groups = (n + 31) // 32
        self.strong, self.decoys = [], []
        for t in range(nq):
            groups = {self.tight[t] // 32}
            strong = []
            for grp in torch.randperm(n_groups, generator=g).tolist():
                if len(strong) == k - 1:
                    break
                if grp in groups:
                    continue
                for o in range(32):
                    r = grp * 32 + (5 * len(strong) + 11 * t + 3 + o) % 32
                    if r < n and r not in used:
                        used.add(r)
                        groups.add(grp)
                        strong.append((r, STRONG[len(strong) % len(STRONG)]))
                        break
            assert len(strong) == k - 1
            self.strong.append(strong)
            near = [self.tight[t] + o for o in (1, -1, 2, -2, 3, -3, 17, -17)]
            decoys = []
            for r in near + torch.randperm(n, generator=g)[: 4 * N_DECOYS].tolist():
                if len(decoys) < N_DECOYS and 0 <= r < n and r not in used:
                    used.add(r)
                    decoys.append(r)
            assert len(decoys) == N_DECOYS >= 32
            self.decoys.append(decoys)
        idx, val, owner = [], [], []
        for t in range(nq):
            for r, m in [(self.tight[t], TIGHT)] + self.strong[t] + [(r, DECOY) for r in self.decoys[t]]:
                idx.append(r)
                val.append(self.u[t] * (m / 2048.0))
                owner.append(t)
        self.special_idx = torch.tensor(idx)
        special = torch.stack(val)
        owner = torch.tensor(owner)
        assert torch.equal(special.to(torch.bfloat16).double(), special) and torch.equal(self.q.to(torch.bfloat16).double(), self.q)
        self.thr, self.tightness, self.expect_idx, self.expect_s = [], [], [], []
        for t in range(nq):
            self._teeth(t)
            foreign = (special[owner != t] @ self.q[t])
            if foreign.numel():
                assert float(foreign.max()) < 0.8 * self.thr[t], (t, float(foreign.max()), self.thr[t])
        # the shard: random rows of norm 1/2 (scores ~ N(0, (||q|| / 2)^2 / D): far below), the special rows written over them
        gd = torch.Generator(device=dev).manual_seed(seed)
        c = torch.randn(n, dim, device=dev, generator=gd)
        c = (c * (0.5 / c.norm(dim=1, keepdim=True))).to(torch.bfloat16)
        c[self.special_idx.to(dev)] = special.to(torch.bfloat16).to(dev)
        self.c = c.contiguous()
        self.queries = self.q.to(torch.bfloat16).to(dev).contiguous()
        scores = self.c.double() @ self.q.to(dev).t()
        scores[self.special_idx.to(dev)] = float("-inf")
        self.filler_max = scores.amax(dim=0).cpu()
        for t in range(nq):
            assert float(self.filler_max[t]) < 0.5 * self.thr[t], (t, float(self.filler_max[t]), self.thr[t])

    def _teeth(self, t):
        q, u, k = self.q[t], self.u[t], self.k
        c = u * (TIGHT / 2048.0)
        d = _e4m3(c).double() / 256.0
        e = c - d
        thr = float(q @ c)
        s8 = float(q @ d)
        qe = float(q.norm() * e.norm())
        assert torch.equal(d, u * (32 / 2048.0)), "the tight row no longer rounds down to 4 2^j"
        assert s8 + 1e-4 < thr, "a kernel WITHOUT the bound would keep the row: no teeth"
        assert s8 + 0.99 * qe + 1e-4 < thr, "a bound 1 % too small would keep the row: no teeth"
        assert s8 + 0.99 * 1.0011 * qe + 1e-4 < thr, "... also with the kernel's own x 1.0005 on ||q|| and on be"
        assert s8 + qe >= thr - 1e-9 * thr, "the true bound does not hold: the construction is wrong"
        self.tightness.append((thr - s8) / qe)
        assert abs(self.tightness[-1] - 1.0) < 1e-12
        c2 = u * (DECOY / 2048.0)
        d2 = _e4m3(c2).double() / 256.0
        assert torch.equal(d2, d), "the decoy no longer rounds up to the tight row's shadow bytes"
        assert float(q @ d2) >= s8 and float(q @ c2) < thr and float((c2 - d2).norm()) == float(e.norm())
        mults = sorted(set(m for _, m in self.strong[t]))
        rows = torch.stack([u * (m / 2048.0) for m in [TIGHT, DECOY] + mults]) if mults else torch.stack([c, c2])
        assert all(float(q @ (u * (m / 2048.0))) > thr for m in mults)
        top = _exact_in_fp32(q, rows, -14, "bf16 pass")
        _exact_in_fp32(q, _e4m3(rows).double(), -4, "shadow pass")
        assert top < 2.0 ** 10
        self.thr.append(thr)
        order = sorted(self.strong[t], key=lambda rm: (-rm[1], rm[0])) + [(self.tight[t], TIGHT)]
        self.expect_idx.append([r for r, _ in order])
        self.expect_s.append([float(q @ (u * (m / 2048.0))) for _, m in order])


def _search_tight(tscan, shard, split, idx_base=0, expect=True, dense=True):
    """The shard through the shadow (built over [0, split), then extended), through the plain scan and the dense path: the same bits."""
    c, queries, k, n, nq = shard.c, shard.queries, shard.k, shard.n, shard.nq
    sh = tscan.ScanShadow(c[:split], cap_rows=n)
    assert sh.rows == split and not sh.serves(n, nq, k)
    sh.extend(c, n)
    assert sh.dim == shard.dim and sh.serves(n, nq, k), "the call below would not take the shadow path"
    got_s, got_i, flag = tscan.scan_topk(c, queries, k, idx_base=idx_base, return_flag=True, shadow=sh)
    want_s, want_i, flag0 = tscan.scan_topk(c, queries, k, idx_base=idx_base, return_flag=True)
    ex_s, ex_i = tscan.scan_topk(c, queries, k, idx_base=idx_base, exact_dense=True) if dense else (None, None)
    torch.cuda.synchronize()
    tag = (shard.dim, n, k, nq, shard.tight, split, idx_base)
    assert flag == 0 and flag0 == 0, (tag, flag, flag0)
    if expect:
        exp_i = torch.tensor(shard.expect_idx, dtype=torch.int32) + idx_base
        exp_s = torch.tensor(shard.expect_s, dtype=torch.float32)
        assert torch.equal(want_i.cpu(), exp_i) and torch.equal(_bits(want_s.cpu()), _bits(exp_s)), ("plain scan vs fp64", tag)
        for t in range(nq):
            assert int(got_i[t, k - 1]) == shard.tight[t] + idx_base, ("the tight row is not the k-th hit", tag, t, got_i[t].tolist()[-4:])
            assert not set(got_i[t].tolist()) & set(r + idx_base for r in shard.decoys[t]), ("a decoy was returned", tag, t)
    assert torch.equal(got_i, want_i) and torch.equal(_bits(got_s), _bits(want_s)), ("shadow vs plain scan", tag)
    if dense:
        assert torch.equal(got_i, ex_i) and torch.equal(_bits(got_s), _bits(ex_s)), ("shadow vs dense path", tag)
    return got_s, got_i


@pytest.mark.parametrize("k", (1, 10, 64))
@pytest.mark.parametrize("dim", DIMS)
def test_shadow_keeps_the_row_whose_bound_holds_with_equality(dev, built_lib, monkeypatch, dim, k):
    """The k-th best row loses exactly ||q|| ||e|| to the shadow's rounding, and its score IS thr: a filter without the ``||q|| be``
    term, or with one 1 % too small, drops it (asserted in fp64 before anything runs); decoys with the same shadow bytes and a lower
    true score survive pass 1, so a kernel that ranked survivors by their shadow scores would return them.  Every width; every shard
    size with the tight row at row 0, at a 16-row group's edge (15, 16), at n - 1 (a partial tail group) and at the first row
    appended by ``extend``; 1, 2 and 4 queries, each with its own sign pattern and its own tight row."""
    from tensor_truth_amd import scan as tscan

    monkeypatch.setattr(tscan.ScanShadow, "MIN_ROWS", FLOOR)
    worst, runs = 0.0, 0
    for ni, n in enumerate(SIZES):
        split = (n // 2) | 1                   # odd: no multiple of 4 or 16
        places = [0, 15, 16, n - 1, split]
        for pi in range(len(places)):
            nq = (1, 2, 4)[(ni + pi) % 3]
            tight_rows = [places[(pi + t) % len(places)] for t in range(nq)]
            shard = _TightShard(dev, dim, n, k, tight_rows, seed=dim * 1000 + k * 10 + ni * 5 + pi)
            _search_tight(tscan, shard, split, idx_base=(0, 7)[pi % 2])
            worst = max(worst, max(abs(x - 1.0) for x in shard.tightness))
            runs += 1
    print(f"\ntight rows dim {dim} k {k}: {runs} shards, |tightness - 1| <= {worst:.1e}, last thr {shard.thr}, "
          f"filler max {[round(float(v), 3) for v in shard.filler_max]}")


def test_shadow_keeps_the_tight_row_at_k_1024(dev, built_lib, monkeypatch):
    """The same construction at the largest k: 131 072 x 128 (the floor 128 k), 1023 stronger rows in groups of their own."""
    from tensor_truth_amd import scan as tscan

    monkeypatch.setattr(tscan.ScanShadow, "MIN_ROWS", FLOOR)
    n = 131_072
    split = (n // 2) | 1
    shard = _TightShard(dev, 128, n, 1024, [split], seed=1024)
    _search_tight(tscan, shard, split)
    print(f"\ntight row k 1024: thr {shard.thr[0]}, tightness {shard.tightness[0]}, filler max {float(shard.filler_max[0]):.3f}")


# ---- 3. rows behind n_rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_shadow_never_returns_rows_behind_n_rows(dev, built_lib, monkeypatch, dim):
    """The matrix and its shadow hold 37 more rows than the search covers, and those rows are copies of the query -- the best match
    there could be, also inside the last 16-row group.  Nothing at or behind ``n_rows`` comes back; the result is the plain scan's."""
    from tensor_truth_amd import scan as tscan

    monkeypatch.setattr(tscan.ScanShadow, "MIN_ROWS", FLOOR)
    g = torch.Generator(device=dev).manual_seed(300 + dim)
    k = 10
    for n in (8193, 8200, 12_345):
        cap = n + 37
        mat = torch.randn(cap, dim, device=dev, generator=g)
        mat = (mat / mat.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        q = torch.randn(2, dim, device=dev, generator=g)
        q = (q / q.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()
        mat[n:] = q[0]
        mat[n + 1:: 2] = q[1]
        mat = mat.contiguous()
        sh = tscan.ScanShadow(mat)
        assert sh.rows == cap == sh.cap_rows and sh.serves(n, 2, k)
        for base in (0, 1_000_000):
            got_s, got_i, flag = tscan.scan_topk(mat[:n], q, k, idx_base=base, return_flag=True, shadow=sh)
            want_s, want_i, flag0 = tscan.scan_topk(mat[:n], q, k, idx_base=base, return_flag=True)
            torch.cuda.synchronize()
            print(f"\nrows behind n_rows: dim {dim} n {n} base {base}: max index {int(got_i.max()) - base}, best score {float(got_s.max()):.4f}")
            assert flag == 0 and flag0 == 0
            assert int(got_i.min()) >= base and int(got_i.max()) < base + n, "a row behind n_rows was returned"
            assert torch.equal(got_i, want_i) and torch.equal(_bits(got_s), _bits(want_s))


# ---- 4. special values in the search -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_shadow_search_with_tombstones_saturated_and_flushed_rows(dev, built_lib, monkeypatch, dim):
    """A NaN tombstone where the tight row would be is never returned; a row with one saturated element (3.0: its shadow says 1.75)
    that is the true best is returned; a row whose elements all lie below 2^-18 -- an all-zero shadow, the whole score in ``e`` --
    is returned when it is the k-th best.  All bit-identical to the plain scan."""
    from tensor_truth_amd import scan as tscan

    monkeypatch.setattr(tscan.ScanShadow, "MIN_ROWS", FLOOR)
    n, k = 8200, 10
    split = (n // 2) | 1
    # (a) tombstone in the tight row's place: the k-th hit is the first decoy instead
    shard = _TightShard(dev, dim, n, k, [n - 1], seed=4000 + dim)
    shard.c[n - 1] = float("nan")
    s, i = _search_tight(tscan, shard, split, expect=False, dense=False)
    first_decoy = min(shard.decoys[0])
    print(f"\nspecial values dim {dim}: tombstone at {n - 1}: hits {i[0].tolist()}")
    assert n - 1 not in i[0].tolist() and i[0].tolist() == shard.expect_idx[0][:-1] + [first_decoy]
    # (b) one saturated element in the true best row; with k = 1 thr is that row's own score
    shard = _TightShard(dev, dim, n, 1, [16], seed=4100 + dim)
    q, u = shard.q[0], shard.u[0]
    sat = u * (66 / 2048.0)
    sat[0] = 3.0 * torch.sign(u[0])
    assert torch.equal(sat.to(torch.bfloat16).double(), sat)
    d = _e4m3(sat).double() / 256.0
    assert abs(float(d[0])) == 1.75 and float(q @ d) + 1e-4 < float(q @ sat) and float(q @ sat) > shard.thr[0]
    _exact_in_fp32(q, sat.unsqueeze(0), -14, "saturated row")
    row = n - 3
    assert row not in shard.special_idx.tolist()
    shard.c[row] = sat.to(torch.bfloat16).to(dev)
    s, i = _search_tight(tscan, shard, split, expect=False)
    print(f"  saturated row {row}: hit {i[0].tolist()} score {float(s[0, 0])} (fp64 {float(q @ sat)}, from the shadow {float(q @ d)})")
    assert i[0].tolist() == [row] and float(s[0, 0]) == float(q @ sat)
    # (c) the flushed row: c = u 2^-22 (|c_i| <= 2^-19), q = 16 u, so q.c = sum 4^j 2^-18 is far above the filter's absolute slack;
    #     k - 1 stronger e4m3-exact rows u m 2^-17 in groups of their own; every other row is e4m3-exact with a score below -1 (or zero)
    k = 3
    g = torch.Generator().manual_seed(4200 + dim)
    u = ((torch.randint(0, 2, (dim,), generator=g) * 2 - 1) * 2.0 ** torch.randint(0, 4, (dim,), generator=g)).double()
    q = u * 16.0
    tiny = u * 2.0 ** -22
    rest = (torch.randn(n, dim, generator=g) * 32.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).double() / 256.0
    sc = rest @ q
    rest = rest * torch.where(sc > 0, -1.0, 1.0).unsqueeze(1)
    rest[(rest @ q) > -1.0] = 0.0
    tiny_row, strong_rows = n - 1, (40, 4100)
    rest[tiny_row] = tiny
    for m, r in enumerate(strong_rows):
        rest[r] = u * ((m + 1) * 2.0 ** -17)
    assert torch.equal(rest.to(torch.bfloat16).double(), rest) and torch.equal(q.to(torch.bfloat16).double(), q)
    assert float(tiny.abs().max()) < 2.0 ** -18 and not bool(_e4m3(tiny).double().any()), "the row's shadow is not all zeros"
    thr = float(q @ tiny)
    scores = rest @ q
    assert 1e-4 + 1e-5 < thr and abs(float(q.norm() * tiny.norm()) / thr - 1.0) < 1e-12       # without the bound the row is dropped
    assert sorted(scores.topk(k).indices.tolist()) == sorted([tiny_row, *strong_rows]) and float(scores.topk(k + 1).values[-1]) <= 0.0
    _exact_in_fp32(q, rest[[tiny_row, *strong_rows]], -18, "flushed row")
    c = rest.to(torch.bfloat16).to(dev).contiguous()
    qd = q.to(torch.bfloat16).to(dev).unsqueeze(0).contiguous()
    sh = tscan.ScanShadow(c)
    assert sh.serves(n, 1, k)
    got_s, got_i, flag = tscan.scan_topk(c, qd, k, return_flag=True, shadow=sh)
    want_s, want_i, flag0 = tscan.scan_topk(c, qd, k, return_flag=True)
    torch.cuda.synchronize()
    print(f"  flushed row {tiny_row}: hits {got_i[0].tolist()} scores {got_s[0].tolist()} (thr {thr}, ||q|| {float(q.norm()):.1f})")
    assert flag == 0 and flag0 == 0
    assert got_i[0].tolist() == [strong_rows[1], strong_rows[0], tiny_row] and float(got_s[0, 2]) == thr
    assert torch.equal(got_i, want_i) and torch.equal(_bits(got_s), _bits(want_s))


# ---- 5. large norms: the filter's rounding slack -------------------------------------------------------------------------------------------
LARGE_K = (1, 2, 5, 10, 33, 64)


@pytest.mark.parametrize("scale", (1.0, 1.0 / 32.0), ids=("norm30", "unit_control"))
def test_shadow_rounding_slack_at_large_norms(dev, built_lib, monkeypatch, scale):
    """e4m3-exact rows (be ~ 1e-9) of norm ~ 30 and un-normalised near-neighbour queries: scores ~ 900, where two fp32 evaluations of
    the same dot product in different K orders differ by more than an ABSOLUTE 1e-4.  At 8200 rows the sample is the whole shard, so
    for each of 4 queries x 6 values of k the k-th best row sits exactly on thr, and the shadow pass must keep it whatever its own
    accumulation order gives.  The control is the same shard at unit norm (x 1/32).

    Only k = 1 puts a row with a score of ||c||^2 ~ 900 on thr (the second best scores ~ 280, the rest ~ 90), so 32 more four-query
    calls at k = 1 follow.  With the filter's former absolute slack of 1e-4 the 24 cases passed (thr - q.d <= 3.3e-5 in fp64) and 10 of
    those 32 calls lost their best row (thr - q.d between -3.0e-4 and +2.8e-4 at ||q|| ||c|| up to 1007); the slack is now
    2 D 2^-23 ||q|| (dn + be) (shadow.hip)."""
    from tensor_truth_amd import scan as tscan

    monkeypatch.setattr(tscan.ScanShadow, "MIN_ROWS", FLOOR)
    dim, n = 1024, 8200
    g = torch.Generator().manual_seed(55)
    rows = (torch.randn(n, dim, generator=g) * 256.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() / 256.0
    pairs = [(17, 4000), (8199, 3), (2048, 2049), (5000, 123)]
    queries = torch.stack([rows[r] + 0.3 * rows[o] for r, o in pairs]) * scale
    rows = rows * scale
    assert torch.equal(rows.to(torch.bfloat16).float(), rows)
    c = rows.to(torch.bfloat16).to(dev).contiguous()
    q = queries.to(torch.bfloat16).to(dev).contiguous()
    sh = tscan.ScanShadow(c)
    q64, c64 = q.cpu().double(), c.cpu().double()
    d64 = _e4m3(c.cpu()).double() / 256.0
    be = float((c64 - d64).norm(dim=1).max())
    exact = q64 @ c64.t()                                       # [4, n], fp64
    shadow_exact = q64 @ d64.t()
    failures = []
    for k in LARGE_K:
        assert sh.serves(n, 4, k)
        got_s, got_i, flag = tscan.scan_topk(c, q, k, return_flag=True, shadow=sh)
        want_s, want_i, flag0 = tscan.scan_topk(c, q, k, return_flag=True)
        torch.cuda.synchronize()
        kth = want_i[:, k - 1].cpu().long()
        thr = want_s[:, k - 1].cpu().double()                   # the bf16 pass's fp32 score of the k-th row: the threshold
        ar = torch.arange(4)
        qc = q64.norm(dim=1) * c64[kth].norm(dim=1)
        above = thr - shadow_exact[ar, kth]                     # what the slack has to cover before the shadow pass's OWN rounding
        print(f"\nlarge norms x {scale:g} k {k}: ||q|| ||c|| {[round(float(v), 1) for v in qc]}, thr {[float(v) for v in thr]}, "
              f"thr - q.d (fp64) {[f'{float(v):.2e}' for v in above]}, thr - q.c (fp64) {[f'{float(v):.2e}' for v in thr - exact[ar, kth]]}, "
              f"2 D 2^-23 ||q|| ||c|| {[f'{float(v):.2e}' for v in 2 * dim * 2.0 ** -23 * qc]}, max be {be:.2e}, flags {flag} {flag0}")
        same = flag == 0 and flag0 == 0 and torch.equal(got_i, want_i) and torch.equal(_bits(got_s), _bits(want_s))
        if not same:
            failures.append((k, got_i.tolist(), want_i.tolist()))
    # beyond those 24: only k = 1 puts a row with a score of ||c||^2 on thr, so 128 more queries of the same make at k = 1
    top_qc, top_above, top_below = 0.0, float("-inf"), float("inf")
    for call in range(32):
        near = torch.randint(0, n, (4, 2), generator=g)
        qs = torch.stack([rows[r] + 0.3 * rows[o] for r, o in near.tolist()]).to(torch.bfloat16)
        qg = qs.to(dev).contiguous()
        got_s, got_i, flag = tscan.scan_topk(c, qg, 1, return_flag=True, shadow=sh)
        want_s, want_i, flag0 = tscan.scan_topk(c, qg, 1, return_flag=True)
        kth = want_i[:, 0].cpu().long()
        diff = want_s[:, 0].cpu().double() - (qs.double() * d64[kth]).sum(dim=1)
        top_qc = max(top_qc, float((qs.double().norm(dim=1) * c64[kth].norm(dim=1)).max()))
        top_above, top_below = max(top_above, float(diff.max())), min(top_below, float(diff.min()))
        if not (flag == 0 and flag0 == 0 and torch.equal(got_i, want_i) and torch.equal(_bits(got_s), _bits(want_s))):
            failures.append(("k = 1 sweep", call, got_i.tolist(), want_i.tolist()))
    print(f"\nlarge norms x {scale:g}: 128 more queries at k = 1: ||q|| ||c|| up to {top_qc:.1f}, thr - q.d (fp64) in [{top_below:.2e}, {top_above:.2e}], "
          f"{len(failures)} calls differ from the plain scan")
    assert not failures, failures


# ---- 6. overflow at a small shape ----------------------------------------------------------------------------------------------------------
def test_shadow_survivor_lists_overflow_at_a_small_shape(dev, built_lib, monkeypatch):
    """300 000 identical rows x 128: every row reaches thr, a wave's ~146 survivors exceed its list of 128, the status word is raised
    and the default call comes back through the exact fallback -- rows 0 .. k - 1 with the plain scan's score bits.  Distinct random
    rows of the same shape raise nothing."""
    from tensor_truth_amd import scan as tscan

    monkeypatch.setattr(tscan.ScanShadow, "MIN_ROWS", FLOOR)
    n, dim, k = 300_000, 128, 20
    g = torch.Generator(device=dev).manual_seed(6)
    row = torch.randn(1, dim, device=dev, generator=g)
    row = (row / row.norm()).to(torch.bfloat16).contiguous()
    c = row.repeat(n, 1).contiguous()
    sh = tscan.ScanShadow(c)
    assert sh.serves(n, 1, k)
    _, _, flagged = tscan.scan_topk(c, row, k, return_flag=True, shadow=sh)
    s, i = tscan.scan_topk(c, row, k, shadow=sh)
    want_s, want_i = tscan.scan_topk(c, row, k)
    torch.cuda.synchronize()
    print(f"\noverflow: identical rows flag {flagged}, hits {i[0].tolist()}")
    assert flagged != 0
    assert i[0].tolist() == list(range(k)) and torch.equal(i, want_i) and torch.equal(_bits(s), _bits(want_s))
    del c, sh
    c = torch.randn(n, dim, device=dev, generator=g)
    c = (c / c.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()
    sh = tscan.ScanShadow(c)
    s, i, flag = tscan.scan_topk(c, row, k, return_flag=True, shadow=sh)
    want_s, want_i, flag0 = tscan.scan_topk(c, row, k, return_flag=True)
    torch.cuda.synchronize()
    print(f"  distinct rows flag {flag}")
    assert flag == 0 and flag0 == 0 and torch.equal(i, want_i) and torch.equal(_bits(s), _bits(want_s))


# ---- 7. refusals, directly through the C ABI -----------------------------------------------------------------------------------------------
def test_shadow_c_abi_refuses_what_it_cannot_serve(dev, built_lib):
    """``tt_scan_topk_shadow`` returns its documented codes, with a message, for: 5 queries, 8192 rows, n_rows < 128 k, n_rows beyond the
    shadow's capacity, a misaligned shadow, a workspace one byte short (TT_E_WORKSPACE) and a width outside the kernel set; the two size
    queries return 0 for invalid inputs.  The same arguments without the defect are served."""
    lib = _lib()
    n, dim, k = 8200, 128, 10
    g = torch.Generator(device=dev).manual_seed(7)
    c = torch.randn(n, dim, device=dev, generator=g)
    c = (c / c.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()
    q = c[:5].clone().contiguous()
    sbytes = lib.tt_scan_shadow_bytes(n, dim)
    assert sbytes == _layout(n, dim)[2]
    raw = torch.zeros(sbytes + 512, dtype=torch.uint8, device=dev)
    sptr = _align(raw.data_ptr(), 256)
    st = _stream(dev)
    assert lib.tt_scan_shadow_build(c.data_ptr(), dim, 0, n, sptr, n, st) == 0
    need = max(lib.tt_scan_shadow_workspace_bytes(n, dim, 4, 65), lib.tt_scan_shadow_workspace_bytes(n, dim, 4, k))
    assert need > 0
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    wptr = _align(ws.data_ptr(), 256)
    out_s = torch.full((5, 65), -7.0, dtype=torch.float32, device=dev)
    out_i = torch.full((5, 65), -7, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def call(n_rows=n, dim_=dim, nq=1, k_=k, shadow=sptr, cap=n, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = need
        rc = lib.tt_scan_topk_shadow(c.data_ptr(), shadow, cap, n_rows, dim_, q.data_ptr(), nq, k_, 0, out_s.data_ptr(), out_i.data_ptr(),
                                     wptr, ws_bytes, flag.data_ptr(), st)
        return rc, (lib.tt_last_error() or b"").decode("utf-8", "replace")

    INVALID, WORKSPACE = -1, -3
    exact_need = lib.tt_scan_shadow_workspace_bytes(n, dim, 1, k)
    cases = [
        ("n_queries = 5", dict(nq=5), INVALID),
        ("n_rows = 8192", dict(n_rows=8192), INVALID),
        ("n_rows < 128 k", dict(k_=65), INVALID),
        ("n_rows > cap_rows", dict(cap=n - 1), INVALID),
        ("shadow not 256-aligned", dict(shadow=sptr + 16), INVALID),
        ("workspace one byte short", dict(ws_bytes=exact_need - 1), WORKSPACE),
        ("dim = 192", dict(dim_=192), INVALID),
    ]
    for what, kw, code in cases:
        rc, msg = call(**kw)
        print(f"\nrefusal {what}: rc {rc}, '{msg}'")
        assert rc == code and msg.strip(), (what, rc, msg)
    torch.cuda.synchronize()
    assert bool((out_s == -7.0).all()) and bool((out_i == -7).all()), "a refused call wrote results"
    rc, msg = call(ws_bytes=exact_need)
    assert rc == 0, msg
    want_s, want_i = torch.empty(1, k, dtype=torch.float32, device=dev), torch.empty(1, k, dtype=torch.int32, device=dev)
    pneed = lib.tt_scan_workspace_bytes(n, dim, 1, k)
    pws = torch.empty(pneed + 256, dtype=torch.uint8, device=dev)
    assert lib.tt_scan_topk(c.data_ptr(), n, dim, q.data_ptr(), 1, k, 0, want_s.data_ptr(), want_i.data_ptr(), _align(pws.data_ptr(), 256),
                            pneed, flag.data_ptr(), st) == 0
    torch.cuda.synchronize()
    got_s, got_i = out_s.view(-1)[:k], out_i.view(-1)[:k]
    assert int(got_i[0]) == 0 and torch.equal(got_i, want_i[0]) and torch.equal(_bits(got_s), _bits(want_s[0]))
    for args in ((0, dim, 1, k), (-1, dim, 1, k), (n, dim, 0, k), (n, dim, 5, k), (n, dim, 1, 0), (n, 192, 1, k), (n, 0, 1, k)):
        assert lib.tt_scan_shadow_workspace_bytes(*args) == 0, args
    for args in ((0, dim), (-5, dim), (n, 0), (n, 192), (n, 1152), (n, -128)):
        assert lib.tt_scan_shadow_bytes(*args) == 0, args
