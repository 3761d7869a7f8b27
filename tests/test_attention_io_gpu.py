"""GPU: the two ends of the 16-bit attention kernel (``tt_attention_varlen[_f16]``) -- what a store that writes whole rows through
LDS can get wrong: a row too many, the neighbouring head's columns, a row of another wave's block.

One batch, lengths 1, 31, 32, 33, 64, 127, 128, 129, 160, 257, 292 (a lone row; a 32-row block boundary; tail tiles with 1, 2 and 4
live waves; the launcher's eight-wave length class at 160), packed back to back with 1-7 gap rows, no start on the 8-row grid;
``ld_out`` larger than heads x width, ``ld_qk`` larger than the two column ranges, both column offsets non-zero.  ``ld_out`` = H + 8
keeps rows 16-byte aligned (the whole-row stores), H + 4 does not (the launcher's 8-byte stores): both are held to the same checks.
``ld_qk`` = 2 H + 64 keeps K rows a multiple of 128 bytes apart (the four-wave kernel of 64-wide heads, the one the rerank step
runs); 2 H + 24 does not, and the launcher then has to take the eight-wave kernel (the four-wave one's second K piece per wave
would be copied from the wrong columns).  A sequence alone is launched with its own length as max_len: 160 alone is the eight-wave
length class.

Judged against test_attention_parity_gpu.py's fp64 reference and bound.  That bound's terms for this kernel (its docstring's
symbols): Q.K products of 16-bit operands are exact in fp32 (D = 0); the probabilities reach the value product rounded to the
operand format, e_p = 2^-8 (bf16) / 2^-11 (fp16, + a_p = 2^-25 for its subnormals) + 2 u for v_exp_f32 -- the f16c entry's P
terms, the same kernel body; the output is one rounding to the format, e_out = 2^-8 / 2^-11 (+ 2^-25) + 2 u for the
normalisation -- the CLS 16-bit entries' output terms; one product per key (n_o = 1).
"""
import functools

import pytest
import torch

from test_attention_parity_gpu import U, _check, _lib_and_stream, _reference, _v8

pytestmark = pytest.mark.gpu

LENS = [1, 31, 32, 33, 64, 127, 128, 129, 160, 257, 292]
GUARD = 64                     # rows in front of and behind the output buffer, inside the same allocation
SENTINEL = 0x7BCD              # (as int16; never a value the kernel writes into a row it owns by accident: checked on the untouched elements only)
EPS = {
    torch.bfloat16: dict(p=2.0 ** -8 + 2 * U, p_abs=0.0, out=2.0 ** -8 + 2 * U, out_abs=0.0, n_o=1),
    torch.float16: dict(p=2.0 ** -11 + 2 * U, p_abs=2.0 ** -25, out=2.0 ** -11 + 2 * U, out_abs=2.0 ** -25, n_o=1),
}
# (ld_out - H, ld_qk - 2 H): 16-byte aligned output rows or not; K rows 128 bytes apart or not (the launcher keeps the four-wave
# 64-wide kernel to the former: its K copies' swizzle step needs it)
CASES = [(dt, dh, pad, ldq) for dt in (torch.bfloat16, torch.float16) for dh in (64, 32)
         for pad, ldq in ((8, 64), (4, 64)) + (((8, 24),) if dh == 64 else ())]
IDS = [f"{'bf16' if dt == torch.bfloat16 else 'fp16'}-2x{dh}-ld_out+{pad}-ld_qk+{ldq}" for dt, dh, pad, ldq in CASES]


def _starts():
    starts, row = [], 3
    for i, n in enumerate(LENS):
        starts.append(row)
        row += n + 1 + i % 7
        if row % 8 == 0:
            row += 1 if (i % 7) < 6 else -1          # (the gap stays within 1..7)
    assert all(s % 8 for s in starts)
    gaps = [starts[i + 1] - starts[i] - LENS[i] for i in range(len(LENS) - 1)]
    assert all(1 <= g <= 7 for g in gaps), gaps
    return starts, (row + 7) // 8 * 8


STARTS, T = _starts()


class Batch:
    """the operands of one (dtype, head width, ld_out padding) case, on the device"""

    def __init__(self, dev, dt, dh, pad, ldq):
        self.dev, self.dt, self.dh, self.heads = dev, dt, dh, 2
        H = self.H = self.heads * dh
        self.q_col0, self.k_col0, self.ld_qk, self.ld_out = 8, H + 16, 2 * H + ldq, H + pad
        g = torch.Generator(device=dev).manual_seed(1000 + dh)       # (one set of values, so one fp64 reference, per dtype and width)
        self.q, self.k, self.v = ((torch.randn(T, H, generator=g, device=dev) * s).to(dt) for s in (1.5, 1.5, 1.0))
        self.vt = _v8(self.v)

    def qk(self, q=None):
        x = torch.full((T, self.ld_qk), 3.0, dtype=self.dt, device=self.dev)      # (finite filler in the columns nobody may read)
        x[:, self.q_col0:self.q_col0 + self.H] = self.q if q is None else q
        x[:, self.k_col0:self.k_col0 + self.H] = self.k
        return x

    def run(self, starts=STARTS, lens=LENS, max_len=None, q=None, vt=None):
        """-> the whole allocation as int16 [GUARD + T + GUARD][ld_out]; the kernel gets the T rows in the middle"""
        _lib, lib, st = _lib_and_stream(self.dev)
        qk = self.qk(q)
        vt = self.vt if vt is None else vt
        alloc = torch.full((GUARD + T + GUARD, self.ld_out), SENTINEL, dtype=torch.int16, device=self.dev)
        ss = torch.tensor(starts, dtype=torch.int32, device=self.dev)
        sl = torch.tensor(lens, dtype=torch.int32, device=self.dev)
        fn = lib.tt_attention_varlen if self.dt == torch.bfloat16 else lib.tt_attention_varlen_f16
        rc = fn(qk.data_ptr(), self.ld_qk, self.q_col0, self.k_col0, vt.data_ptr(), 8 * self.H, alloc[GUARD:].data_ptr(), self.ld_out,
                ss.data_ptr(), sl.data_ptr(), len(lens), self.heads, self.dh, max_len or max(lens), st)
        _lib.check(rc, "tt_attention_varlen")
        torch.cuda.synchronize()
        return alloc

    def owned(self, starts=STARTS, lens=LENS):
        m = torch.zeros((GUARD + T + GUARD, self.ld_out), dtype=torch.bool, device=self.dev)
        for s, n in zip(starts, lens):
            m[GUARD + s:GUARD + s + n, : self.H] = True
        return m


@functools.lru_cache(maxsize=None)
def _base(dev, dt, dh, pad, ldq):
    """one batch and its output, shared by the tests of a case and left unchanged"""
    b = Batch(dev, dt, dh, pad, ldq)
    return b, b.run()


@functools.lru_cache(maxsize=None)
def _ref(dev, dt, dh):
    """the fp64 reference and bound of the batch's values: computed once per dtype and head width"""
    b = Batch(dev, dt, dh, 8, 64)
    return _reference(b.q.double(), b.k.double(), b.v.double(), STARTS, LENS, b.heads, dh, EPS[dt])


def _seq_rows(alloc, s, n, H):
    return alloc[GUARD + s:GUARD + s + n, :H]


@pytest.mark.parametrize("dt,dh,pad,ldq", CASES, ids=IDS)
def test_context_against_fp64_and_untouched_bytes(dev, built_lib, dt, dh, pad, ldq):
    b, alloc = _base(dev, dt, dh, pad, ldq)
    owned = b.owned()
    # every element the kernel must not write: gap rows, rows past the last sequence, the columns beyond heads x width, the guard rows
    assert bool((alloc[~owned] == SENTINEL).all()), "an element outside the sequences' rows and columns was written"
    got = torch.cat([_seq_rows(alloc, s, n, b.H) for s, n in zip(STARTS, LENS)]).contiguous().view(dt).double()
    want, bound = _ref(dev, dt, dh)
    ratio = _check(got, want, bound, f"{dt} 2x{dh} ld_out {b.ld_out} ld_qk {b.ld_qk}")
    print(f"\nerror / bound {ratio:.3f}")


@pytest.mark.parametrize("dt,dh,pad,ldq", CASES, ids=IDS)
def test_rows_do_not_depend_on_the_batch_or_the_wave_count(dev, built_lib, dt, dh, pad, ldq):
    b, alloc = _base(dev, dt, dh, pad, ldq)
    n_seq = len(LENS)
    for i, (s, n) in enumerate(zip(STARTS, LENS)):                 # alone
        one = b.run([s], [n])
        assert torch.equal(_seq_rows(one, s, n, b.H), _seq_rows(alloc, s, n, b.H)), f"sequence {i} (length {n}) alone differs from the batch"
        assert bool((one[~b.owned([s], [n])] == SENTINEL).all()), f"sequence {i} alone: an element outside its rows was written"
    for r in range(1, n_seq):                                       # every sequence at every position of the sequence list
        order = [(i + r) % n_seq for i in range(n_seq)]
        rot = b.run([STARTS[i] for i in order], [LENS[i] for i in order])
        assert torch.equal(rot, alloc), f"the batch listed from sequence {r} on differs"
    # max_len 292: ten 32-row blocks, the four-wave kernel; max_len 512: sixteen, the eight-wave one (64-wide heads)
    assert torch.equal(b.run(max_len=512), alloc), "the eight-wave launch differs from the four-wave one"


@pytest.mark.parametrize("dt,dh,pad,ldq", CASES, ids=IDS)
def test_adversarial_query_rows_leave_their_neighbours_alone(dev, built_lib, dt, dh, pad, ldq):
    b, alloc = _base(dev, dt, dh, pad, ldq)
    odd = torch.zeros(T, dtype=torch.bool, device=dev)
    for s, n in zip(STARTS, LENS):
        odd[s + 1:s + n:2] = True
    own = b.owned()
    clean = own.clone()
    clean[GUARD:GUARD + T][odd] = False
    for what, val in (("NaN", float("nan")), ("largest finite", torch.finfo(dt).max)):
        q = b.q.clone()
        q[odd] = val
        out = b.run(q=q)
        assert torch.equal(out[clean], alloc[clean]), f"{what} query rows changed a clean row"
        assert bool((out[~own] == SENTINEL).all()), f"{what} query rows: an element outside the sequences was written"
        if what == "NaN":              # a NaN query row's scores are all NaN: so is its context, in either format
            bad = torch.cat([_seq_rows(out, s, n, b.H)[1::2] for s, n in zip(STARTS, LENS)]).contiguous().view(dt)
            assert bool(torch.isnan(bad).all()), "a NaN query row did not come out as NaN"
    if dt == torch.float16:
        # the fp16 contract (common.h e_sat): finite results beyond the range saturate at +-65504, never infinity, and a NaN stays a NaN
        # -- values at the format's maximum on every key, so that a context's rounded sum can land past it
        v = b.v.clone()
        v[:, ::2] = 65504.0
        v[:, 1::2] = -65504.0
        q = b.q.clone()
        q[odd] = float("nan")
        out = b.run(q=q, vt=_v8(v))
        rows = torch.cat([_seq_rows(out, s, n, b.H) for s, n in zip(STARTS, LENS)]).contiguous().view(dt)
        sel = torch.cat([odd[s:s + n] for s, n in zip(STARTS, LENS)])
        assert bool(torch.isnan(rows[sel]).all()), "a NaN query row did not come out as NaN"
        # (the probabilities are rounded to fp16 for the value product and the row sum is not: a context of +-65504 values lands up
        #  to 2^-11 past 65504 -- infinity without the clamp -- or as far below it)
        fin = rows[~sel].float()
        assert bool(torch.isfinite(fin).all()), "a context of +-65504 values became infinite instead of saturating at +-65504"
        assert bool((fin.abs() >= 65504.0 * (1 - 2.0 ** -9)).all()) and bool((fin.abs() == 65504.0).any())
        assert bool((out[~own] == SENTINEL).all())
