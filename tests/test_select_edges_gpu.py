"""GPU: ``tt_topk_merge`` on select_kernel, the LDS sorting network that serves 64 < k <= 1024 (csrc/select.hip), bit for bit
against the numpy contract of tests/select_refs.py.

Every k whose padded size kpad is another power of two (128 ... 1024), below, at and above it; list lengths around every
threshold of the kernel: k itself, one and two sort groups, the prefilter's onset (2048 staged keys) and its admissibility bound
(ceil(m / 1024) * kpad <= 4096), one LDS chunk (room = 8192 - kpad staged keys) and its seams, several flushes with a partial
last one.  The query rows are the wave kernel's contract rows (tests/test_abi_sweeps_gpu.py) and what a long output needs:
index order alone, fewer live entries than k, live infinities, mismatched entries, the winners placed around the chunk seams,
the ends of the index range, and a tie class that the prefilter's threshold falls into (``select_refs.ROW_NAMES``).
tests/test_select_refs_host.py shows on the CPU that every one of these batches tells four wrong oracles from the right one.

The outputs sit between guard elements in one allocation: nothing may be written outside [q][k].  ``tt_topk_merge`` fixes the
output stride at k; strides other than k are exercised by tests/test_scan_ties_gpu.py (row-list scan with segments)."""
import numpy as np
import pytest
import torch

import select_refs as refs

pytestmark = pytest.mark.gpu

GUARD = 1024                       # elements in front of and behind each output
FILL_S = 0x7FC0BEEF                # a NaN pattern no selection produces
FILL_I = -77777


def _merge_guarded(dev, scores, idx, k):
    """tt_topk_merge through the C ABI on numpy [Q, M] inputs -> numpy (scores [Q, k], idx [Q, k]); the guards checked."""
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    q, m = scores.shape
    s_d = torch.from_numpy(np.ascontiguousarray(scores)).to(dev)
    i_d = torch.from_numpy(np.ascontiguousarray(idx)).to(dev)
    out_s = torch.full((2 * GUARD + q * k,), FILL_S, dtype=torch.int32, device=dev)
    out_i = torch.full((2 * GUARD + q * k,), FILL_I, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.tt_topk_merge(s_d.data_ptr(), i_d.data_ptr(), q, m, k, out_s[GUARD:].data_ptr(), out_i[GUARD:].data_ptr(),
                               torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "tt_topk_merge")
    torch.cuda.synchronize()
    hs, hi = out_s.cpu(), out_i.cpu()
    for name, h, fill in (("scores", hs, FILL_S), ("indices", hi, FILL_I)):
        assert (h[:GUARD] == fill).all() and (h[GUARD + q * k:] == fill).all(), f"a guard element of the {name} was written"
    body_s = hs[GUARD:GUARD + q * k]
    assert (body_s != FILL_S).all(), "an output element was left unwritten"
    return body_s.view(torch.float32).view(q, k).numpy(), hi[GUARD:GUARD + q * k].view(q, k).numpy()


def _first_difference(got_s, got_i, want_s, want_i, r):
    bad = np.nonzero((refs.canon_bits(got_s[r]) != refs.canon_bits(want_s[r])) | (got_i[r] != want_i[r]))[0]
    j = int(bad[0])
    lo, hi = max(j - 1, 0), j + 3
    return (f"{len(bad)} of {got_s.shape[1]} places differ, the first at {j}: got {list(zip(got_s[r, lo:hi].tolist(), got_i[r, lo:hi].tolist()))} "
            f"want {list(zip(want_s[r, lo:hi].tolist(), want_i[r, lo:hi].tolist()))}")


def _hold_to_contract(dev, s, ix, k, names, calls):
    want_s, want_i = refs.select_topk(s, ix, k)
    failures = []
    for lo, hi in calls:
        assert 7 <= hi - lo <= 9
        got_s, got_i = _merge_guarded(dev, s[lo:hi], ix[lo:hi], k)
        ok = refs.same_bits(got_s, got_i, want_s[lo:hi], want_i[lo:hi])
        for r in np.nonzero(~ok)[0]:
            failures.append(f"{names[lo + r]!r}: " + _first_difference(got_s, got_i, want_s[lo:hi], want_i[lo:hi], r))
    return failures


CASES = [(k, m) for k in refs.KS for m in refs.list_lengths(k)]


@pytest.mark.parametrize("k,m", CASES)
def test_lds_network_list_lengths(dev, built_lib, k, m):
    s, ix = refs.query_rows(k, m)
    failures = _hold_to_contract(dev, s, ix, k, refs.ROW_NAMES, refs.CALLS)
    print(f"\nk {k} (kpad {refs.kpad_of(k)}, room {refs.room_of(k)}) m {m}: {len(refs.ROW_NAMES) - len(failures)} of "
          f"{len(refs.ROW_NAMES)} query rows bit-exact")
    for f in failures:
        print("  " + f)
    assert not failures, (k, m, failures[0])


@pytest.mark.parametrize("m", refs.FALLBACK_LENGTHS)
def test_duplicate_pairs_defeat_the_prefilter(dev, built_lib, m):
    """More than 4096 equal keys at or above the prefilter's threshold (only a caller's index column can supply equal keys): the
    survivors do not fit, flush_staged has to run the network over everything staged -- the copies come first, as the contract says."""
    s, ix = refs.fallback_rows(m)
    failures = _hold_to_contract(dev, s, ix, refs.FALLBACK_K, refs.FALLBACK_NAMES, ((0, len(refs.FALLBACK_NAMES)),))
    print(f"\nduplicate pairs, k {refs.FALLBACK_K} m {m}: {len(refs.FALLBACK_NAMES) - len(failures)} of {len(refs.FALLBACK_NAMES)} "
          "query rows bit-exact")
    for f in failures:
        print("  " + f)
    assert not failures, (m, failures[0])


def test_wave_kernel_control_at_k_64(dev, built_lib):
    """The same query rows and the same oracle at k = 64, the largest k of select_wave_kernel: both kernels answer to one contract
    in one file (the wave kernel's own sweep: tests/test_abi_sweeps_gpu.py)."""
    k, m = 64, 5000
    s, ix = refs.query_rows(k, m)
    failures = _hold_to_contract(dev, s, ix, k, refs.ROW_NAMES, refs.CALLS)
    print(f"\ncontrol k {k} m {m}: {len(refs.ROW_NAMES) - len(failures)} of {len(refs.ROW_NAMES)} query rows bit-exact")
    for f in failures:
        print("  " + f)
    assert not failures, failures[0]
