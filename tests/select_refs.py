"""The selection contract of csrc/select.hip in plain numpy, the inputs that hold the LDS network (64 < k <= 1024) to it, and
deliberately WRONG oracles that those inputs must tell from the right one.

Contract (``tt_topk_merge`` and every scan's final selection; what ``make_key`` encodes):

* an entry (score, idx) is LIVE iff its score is not NaN and its idx is >= 0;
* live entries are ordered by score descending (-0 and +0 are one value), then idx ascending;
* the output is the first k live entries, then (-inf, -1).

Consequences pinned here: (-inf, idx >= 0) is live and ranks after every finite score; (+inf, idx >= 0) ranks first;
(finite, idx < 0) never ranks; duplicate (score, idx) pairs are all returned, next to each other; a returned zero equals the
oracle's zero whatever its sign (``same_bits`` compares them so).

No torch here: tests/test_select_refs_host.py runs on a machine without a GPU, tests/test_select_edges_gpu.py imports the same
inputs and the same oracle."""
import numpy as np

CHUNK = 8192            # composite keys select_kernel stages in LDS per round (csrc/select.hip kChunk)
PREFILTER_ONSET = 2048  # flush_staged prefilters from this many staged keys on ...
PREFILTER_KEYS = 4096   # ... while ceil(filled / 1024) * kpad stays at or below this (kAux2)
I32_MAX = 2 ** 31 - 1

KS = (65, 100, 128, 129, 256, 257, 512, 1000, 1024)


def kpad_of(k):
    p = 2
    while p < k:
        p *= 2
    return p


def room_of(k):
    """Keys staged per flush next to the running top-kpad."""
    return CHUNK - kpad_of(k)


def list_lengths(k):
    """The list lengths at which select_kernel takes another path for this k."""
    kpad, room = kpad_of(k), room_of(k)
    last_prefiltered = PREFILTER_KEYS // kpad * 1024        # the largest m with ceil(m / 1024) * kpad <= 4096
    ms = [k - 1, k, k + 1, kpad, 2 * kpad, PREFILTER_ONSET - 1, PREFILTER_ONSET, PREFILTER_ONSET + 1, last_prefiltered,
          last_prefiltered + 1, room - 1, room, room + 1, room + kpad, 2 * room, 2 * room + 1, 20000, 70001]
    out = []
    for m in ms:
        if m >= 1 and m not in out:
            out.append(m)
    return out


# ---- oracles ------------------------------------------------------------------------------------------------------------------
def _select(scores, idx, k, tie_desc=False, nan_first=False, neg_zero_lower=False, drop_last_piece=0):
    scores = np.asarray(scores, dtype=np.float32)
    idx = np.asarray(idx, dtype=np.int32)
    assert scores.shape == idx.shape and scores.ndim == 2
    q, m = scores.shape
    s = scores.astype(np.float64)
    i = idx.astype(np.int64)
    nan = np.isnan(s)
    live = i >= 0
    if nan_first:
        s = np.where(nan, np.inf, s)
    else:
        live &= ~nan
    if drop_last_piece:
        live &= (np.arange(m) < (max(m - 1, 0) // drop_last_piece) * drop_last_piece)[None, :]
    if neg_zero_lower:
        s = np.where((s == 0) & np.signbit(s), -1e-300, s)
    s = np.where(s == 0, 0.0, s)                                   # -0 and +0: one value
    k_score = np.where(live, -s, np.inf)                           # dead entries behind every live one, (-inf, live) included:
    k_idx = np.where(live, -i if tie_desc else i, np.iinfo(np.int64).max)      # equal -score, but the largest index key
    kk = min(k, m)
    out_s = np.full((q, k), -np.inf, dtype=np.float32)
    out_i = np.full((q, k), -1, dtype=np.int32)
    if kk:
        order = np.lexsort((k_idx, k_score), axis=1)[:, :kk]       # primary -score, secondary index; stable
        took = np.take_along_axis(live, order, axis=1)
        out_s[:, :kk] = np.where(took, np.take_along_axis(scores, order, axis=1), np.float32(-np.inf))
        out_i[:, :kk] = np.where(took, np.take_along_axis(idx, order, axis=1), -1)
    return out_s, out_i


def select_topk(scores, idx, k):
    """scores [Q, M] fp32, idx [Q, M] int32 -> (scores [Q, k] fp32, idx [Q, k] int32): the contract."""
    return _select(scores, idx, k)


def wrong_oracles(k):
    """name -> a selection that breaks ONE rule of the contract: what a subtly wrong kernel would return."""
    return {
        "ties by index descending": lambda s, i: _select(s, i, k, tie_desc=True),
        "NaN ranks as +inf": lambda s, i: _select(s, i, k, nan_first=True),
        "-0 below +0": lambda s, i: _select(s, i, k, neg_zero_lower=True),
        "last room-sized piece ignored": lambda s, i: _select(s, i, k, drop_last_piece=room_of(k)),
    }


def canon_bits(scores):
    s = np.asarray(scores, dtype=np.float32)
    return np.where(s == 0, np.float32(0.0), s).view(np.int32)


def same_bits(got_s, got_i, want_s, want_i):
    """[Q] bool: query rows whose scores (a zero of either sign is one value) and indices agree bit for bit."""
    return (canon_bits(got_s) == canon_bits(want_s)).all(axis=1) & (np.asarray(got_i) == np.asarray(want_i)).all(axis=1)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def _unique_idx(rng, m, wide=False):
    if wide:                                                       # spread over (0, 2^31 - 1), both ends left free
        return (rng.permutation(m).astype(np.int64) * ((I32_MAX - 2) // m) + 1).astype(np.int32)
    return (rng.permutation(m) * 7 + 3).astype(np.int32)


def _place_best(rng, s, positions, k):
    """The k best scores of the row at ``positions`` (as many as there are), well above everything else."""
    positions = np.unique(np.clip(np.asarray(positions, dtype=np.int64), 0, len(s) - 1))[:k]
    s[positions] = (10.0 + rng.random(len(positions)) * 4.0).astype(np.float32)
    if len(positions) >= 4:
        s[positions[1]] = s[positions[-1]]                         # an exact tie inside the winners, far apart
    return s


ROW_NAMES = (
    "ascending", "descending", "every third tied", "+0 against -0", "every fifth NaN", "all padding", "random, 10 % padding",
    "all scores equal", "fewer live than k", "live +-inf", "mismatched entries", "k best in the last piece",
    "k best in the first piece", "k best astride room - 1 | room and the last index", "indices 0 and 2^31 - 1",
    "a tie class of thousands holding the k-th place",
)
CALLS = ((0, 8), (8, 16))       # query rows per tt_topk_merge call


def query_rows(k, m, seed=None):
    """-> (scores [16, m] fp32, idx [16, m] int32): the wave kernel's contract rows (tests/test_abi_sweeps_gpu.py) and the rows
    that a k in (64, 1024] needs; ``ROW_NAMES`` names them."""
    rng = np.random.default_rng(1000 * k + m if seed is None else seed)
    room = room_of(k)
    first_of_last = (m - 1) // room * room                          # the last room-sized piece: [first_of_last, m)
    R = len(ROW_NAMES)
    s = rng.standard_normal((R, m)).astype(np.float32)
    ix = np.stack([_unique_idx(rng, m) for _ in range(R)])
    kk = min(k, m)
    # 0-2
    s[0] = np.sort(s[0])
    s[1] = np.sort(s[1])[::-1]
    s[2, ::3] = 0.25
    # 3: a few positives, then zeros of both signs (index alone orders them), the rest -1
    n_pos = max(1, min(k // 2, m // 8))
    s[3] = -1.0
    where = rng.permutation(m)
    s[3, where[:n_pos]] = np.abs(s[4, where[:n_pos]]) + 0.5
    zeros = where[n_pos:n_pos + max(2, (m - n_pos) // 2)]
    s[3, zeros] = np.where(rng.random(len(zeros)) < 0.5, np.float32(0.0), np.float32(-0.0))
    # 4
    s[4, ::5] = np.nan
    # padding as in the wave test: 10 % of rows 0-4 and 6, all of row 5
    pad = rng.random((R, m)) < 0.1
    pad[5] = True
    pad[7:] = False
    s[pad] = -np.inf
    ix[pad] = -1
    # 7
    s[7] = 0.5
    # 8: about half of k live entries, the rest padding or NaN
    n_live = max(1, kk // 2)
    dead = rng.permutation(m)[n_live:]
    s[8, dead[::2]] = -np.inf
    ix[8, dead[::2]] = -1
    s[8, dead[1::2]] = np.nan
    # 9: fewer finite entries than k, three +inf, and a class of live -inf that holds the k-th place
    where = rng.permutation(m)
    n_fin, n_ninf = max(1, min(k // 2, m // 4)), max(2, min(k, m // 4))
    s[9] = -np.inf
    s[9, where[:n_fin]] = rng.standard_normal(n_fin).astype(np.float32)
    s[9, where[n_fin:n_fin + 3]] = np.inf
    ix[9, where[n_fin + 3 + n_ninf:]] = -1
    # 10: (finite, -1) with scores above every live one, and (-inf, id >= 0) that fill the output behind the finite entries
    where = rng.permutation(m)
    rest = where[n_fin:]
    s[10, rest[::2]] += 10.0
    ix[10, rest[::2]] = -1
    s[10, rest[1::2]] = -np.inf
    # 11-13
    _place_best(rng, s[11], first_of_last + rng.permutation(m - first_of_last)[:k], k)
    # (12: one run of k neighbours -- k different strided shares of flush_staged's prefilter, whose threshold, the kpad-th best of
    #  the shares' maxima, then IS the kpad-th best key: at k = kpad a filter that kept only the keys above it would lose a winner)
    _place_best(rng, s[12], int(rng.integers(0, max(1, min(room, m) - k + 1))) + np.arange(k), k)
    seam = room if m > room else m // 2
    _place_best(rng, s[13], np.concatenate([[seam - 1, seam, m - 1, 0], np.arange(seam - k // 2 + 1, seam + k // 2 - 1)]), k)
    # 14: four score levels; the best one holds fewer than k entries, the lowest and the highest index among them
    ix[14] = _unique_idx(rng, m, wide=True)
    s[14] = rng.integers(0, 4, m).astype(np.float32) / 4
    top = rng.permutation(m)[:max(2, kk // 2)]
    s[14, top] = 5.0
    ix[14, top[0]], ix[14, top[1]] = I32_MAX, 0
    # 15: k / 2 entries above one level of up to 5000 entries, everything else below it
    where = rng.permutation(m)
    above = min(k // 2, m // 2)
    s[15] = (rng.random(m) * 1.5 - 1.0).astype(np.float32)
    s[15, where[:above]] = (2.0 + rng.random(above)).astype(np.float32)
    s[15, where[above:above + 5000]] = 1.0
    return s, ix


FALLBACK_K = 100
FALLBACK_LENGTHS = (8064, 16129)        # room and 2 * room + 1 at k = 100
FALLBACK_NAMES = (
    "every entry the same pair", "5000 copies on top of random entries", "5000 copies around the k-th place",
    "5000 copies below a class of zeros", "5000 copies, NaN and tied levels around them", "two pairs of 2500 copies, one score",
    "5000 copies at the end of the list, the best entry last",
)


def fallback_rows(m, seed=7):
    """Duplicate (score, idx) PAIRS, which only ``tt_topk_merge``'s caller can supply: more than 4096 keys reach the prefilter's
    threshold, so flush_staged has to give the prefilter up (``ns > kAux2``).  -> (scores [7, m], idx [7, m])."""
    rng = np.random.default_rng(seed + m)
    R, n_copies = len(FALLBACK_NAMES), 5000
    s = (rng.integers(-8, 9, (R, m)) / 4.0).astype(np.float32)      # 17 levels: ties everywhere
    ix = np.stack([_unique_idx(rng, m) for _ in range(R)])

    def copies(r, where, score, idx):
        s[r, where] = score
        ix[r, where] = idx

    copies(0, np.arange(m), 0.75, 12345)
    copies(1, rng.permutation(m)[:n_copies], 3.0, 11)
    where = rng.permutation(m)
    copies(2, where[:n_copies], 1.0, 2)
    s[2, where[n_copies:]] = np.minimum(s[2, where[n_copies:]], 0.5)
    s[2, where[n_copies:n_copies + 40]] = 2.0 + rng.random(40).astype(np.float32)
    where = rng.permutation(m)
    copies(3, where[:n_copies], -1.0, 4)
    rest = where[n_copies:]
    s[3, rest] = np.where(rng.random(len(rest)) < 0.5, np.float32(0.0), np.float32(-0.0))
    s[3, rest[:30]] = 1.0 + rng.random(30).astype(np.float32)
    s[3, rest[30::7]] = -2.0
    where = rng.permutation(m)
    s[4, ::5] = np.nan
    copies(4, where[:n_copies], 1.75, 6)
    where = rng.permutation(m)
    copies(5, where[:2500], 2.5, 9)
    copies(5, where[2500:5000], 2.5, 7)
    copies(6, np.arange(m - n_copies, m), 3.0, 5)
    copies(6, m - 1, 4.0, 1)            # the one entry of the last piece at m = 2 * room + 1: the best of the list
    return s, ix
