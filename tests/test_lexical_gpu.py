"""GPU: BGE-M3's lexical head and hybrid scoring (csrc/lexical.hip, tensor_truth_amd/lexical.py).

Every kernel is compared with fp64 on operands that are exactly representable in the operand type, under a bound computed from the
operands, ``u = 2^-24``:

* ``tt_lexical_weights[_f16|_f32]``.  A product of two operands converted to fp32 and added by fmaf carries one rounding per term;
  H terms in any order, the final butterfly and the bias: ``|pre - pre64| <= (H + 2) u (sum_j |w_j h_j| + |b|)``.  The inputs are
  drawn so that no token's fp64 pre-activation lies within its bound of zero (asserted), so the set of kept ids must be the fp64
  set exactly; a kept weight is the maximum over its id's occurrences, and ``|max a - max b| <= max |a - b|``.
* ``tt_lexical_score``.  ``matches`` products of two fp32 weights (one rounding each, fused into the addition) summed in any
  order: ``(matches + 1) u sum |q_w d_w|``.  Dense: bf16 products are exact in fp32, ``dim`` additions: ``(dim + 1) u sum |q_j d_j|``.
  Hybrid: two products, one addition, one division on the kernel's own two outputs: ``4 u (|w_dense dense| + |w_lex lex|) /
  (w_dense + w_lex)``.  Three wrong references -- one that lets every document entry count (no equality test after the search: the
  sum over the union), one that skips a document's last entry, one that reads one entry past it -- must lie outside the bound.
* ``tt_lexical_scan_topk`` against a stable sort of ``tt_lexical_score``'s own output: exact equality.
* The fixture (tests/golden/make_m3_golden.py) through ``M3Encoder``, ``LexicalStore``, ``HipM3HybridRerank`` and
  ``HipLexicalRetriever``: within 2 e_<type> of fp64 (DESIGN.md 4.8's factor for a second 16-bit implementation), every defect
  outside, the fp64 top-5 order.  The reference precision (fp32 hidden states, ``tt_lexical_weights_f32``) is held to the fp16 bound:
  its own error is smaller than fp16's.

Every figure is printed before it is asserted.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M3 = os.path.join(GOLDEN, "m3_l2")
U = 2.0 ** -24
FACTOR = 2.0
SKIP = (0, 2, 1, 3)                      # <s>, </s>, <pad>, <unk> of XLM-R
BIG_ID = 250001
DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}
SEQ_LENS = [1, 2, 63, 64, 65, 512, 513, 2049, 8192]
CONSTRUCTED = 40                          # length of each constructed sequence


# ---- tt_lexical_weights -------------------------------------------------------------------------------------------------------------
def _weights_inputs(H, dt, seed):
    """-> hidden [n_rows][H] (dt, CPU), w [H] (dt), bias, ids, seq_start, seq_len, pre64 [n_rows], bound [n_rows]."""
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    lens = SEQ_LENS + [CONSTRUCTED] * 4
    starts, row = [], 3                                      # unaligned start rows, gaps of 0 .. 5 rows between sequences
    for n in lens:
        starts.append(row)
        row += n + int(rng.integers(0, 6))
    n_rows = row + 2
    w = (torch.randn(H, generator=gen) * 0.1).to(dt)
    bias = float(np.float32(-0.37))
    hidden = torch.randn(n_rows, H, generator=gen).to(dt)
    ids = rng.integers(0, 4, n_rows).astype(np.int32)        # rows of no sequence: anything
    sgn = torch.sign(w.double()) + (w.double() == 0)
    for b, (s, n) in enumerate(zip(starts, lens)):
        pool = rng.integers(4, BIG_ID + 1, max(1, n // 3))
        seq = rng.choice(pool, n).astype(np.int32)
        special = rng.random(n) < 0.1
        seq[special] = rng.integers(0, 4, int(special.sum()))
        if b == len(SEQ_LENS) - 1:                           # the longest sequence holds the smallest and the largest id
            seq[5], seq[6], seq[-1] = 4, BIG_ID, BIG_ID
        k = b - len(SEQ_LENS)
        if k == 0:                                           # all one id, every weight positive: nnz 1
            seq[:] = 77777
            hidden[s:s + n] = (hidden[s:s + n].double().abs() * sgn).to(dt)
        elif k == 1:                                         # all distinct, every weight positive: nnz = its length
            seq = rng.permutation(np.arange(1000, 1000 + 7 * n, 7))[:n].astype(np.int32)
            hidden[s:s + n] = (hidden[s:s + n].double().abs() * sgn).to(dt)
        elif k == 2:                                         # all special: nnz 0
            seq = rng.integers(0, 4, n).astype(np.int32)
        elif k == 3:                                         # every pre-activation negative: nnz 0
            hidden[s:s + n] = (-hidden[s:s + n].double().abs() * sgn).to(dt)
        ids[s:s + n] = seq
    w64 = w.double()
    for _ in range(20):                                      # no pre-activation within its bound of zero: redraw such rows
        pre = hidden.double() @ w64 + bias
        bound = (H + 2) * U * (hidden.double().abs() @ w64.abs() + abs(bias))
        near = (pre.abs() <= 2 * bound).nonzero()[:, 0]
        if near.numel() == 0:
            break
        hidden[near] = (hidden[near].double() * 1.25 + 0.01 * sgn).to(dt)
    assert (pre.abs() > bound).all(), "the test's own inputs: a pre-activation within its bound of zero"
    return hidden, w, bias, ids, np.asarray(starts, dtype=np.int32), np.asarray(lens, dtype=np.int32), pre.numpy(), bound.numpy()


def _weights_reference(ids, pre, bound, s, n):
    """fp64 lexical vector of rows s .. s+n-1 -> {id: (weight, bound)}."""
    out = {}
    for t, v, e in zip(ids[s:s + n].tolist(), pre[s:s + n].tolist(), bound[s:s + n].tolist()):
        if t in SKIP or v <= 0:
            continue
        w0, e0 = out.get(t, (0.0, 0.0))
        out[t] = (max(w0, v), max(e0, e))
    return out


@pytest.mark.parametrize("dt", list(DTYPES.values()), ids=list(DTYPES))
@pytest.mark.parametrize("H", [128, 384, 1024])
def test_lexical_weights_match_fp64(dev, built_lib, H, dt):
    from tensor_truth_amd import lexical

    hidden, w, bias, ids, starts, lens, pre, bound = _weights_inputs(H, dt, 1000 + H)
    hd, wd = hidden.to(dev), w.to(dev)
    n_rows = hidden.shape[0]
    terms = torch.full((n_rows,), -7, dtype=torch.int32, device=dev)
    weights = torch.full((n_rows,), -7.0, dtype=torch.float32, device=dev)
    _, _, nnz = lexical.lexical_weights(hd, wd, bias, ids, starts, lens, SKIP, out=(terms, weights))
    terms, weights, nnz = terms.cpu().numpy(), weights.cpu().numpy(), nnz.cpu().numpy()
    in_seq = np.zeros(n_rows, dtype=bool)
    worst = 0.0
    for b, (s, n) in enumerate(zip(starts, lens)):
        in_seq[s:s + n] = True
        want = _weights_reference(ids, pre, bound, s, n)
        k = int(nnz[b])
        got_t, got_w = terms[s:s + k], weights[s:s + k]
        assert got_t.tolist() == sorted(want), f"sequence {b} (length {n}): the kept ids are not the fp64 set in ascending order"
        assert (terms[s + k:s + n] == -1).all() and (weights[s + k:s + n] == 0).all(), f"sequence {b}: slots past nnz must hold (-1, 0)"
        for t, v in zip(got_t.tolist(), got_w.tolist()):
            worst = max(worst, abs(v - want[t][0]) / want[t][1])
    assert (terms[~in_seq] == -7).all() and (weights[~in_seq] == -7.0).all(), "rows of no sequence were written"
    c0 = len(SEQ_LENS)
    assert nnz[c0:].tolist()[0] == 1 and nnz[c0 + 1] == CONSTRUCTED and nnz[c0 + 2] == 0 and nnz[c0 + 3] == 0
    big = _weights_reference(ids, pre, bound, starts[c0 - 1], lens[c0 - 1])
    assert 4 in big or BIG_ID in big
    print(f"\nlexical weights H {H} {dt}: max error / bound = {worst:.3f}, nnz {nnz.tolist()}")
    assert worst <= 1.0

    # a sequence alone, at another start row, under the LDS class of its own length: identical bits
    for b in (0, 2, 4, 6, 7, c0 + 1):
        s, n = int(starts[b]), int(lens[b])
        h1 = torch.zeros(n + 9, H, dtype=dt)
        h1[5:5 + n] = hidden[s:s + n]
        i1 = np.zeros(n + 9, dtype=np.int32)
        i1[5:5 + n] = ids[s:s + n]
        t1, w1, n1 = lexical.lexical_weights(h1.to(dev), wd, bias, i1, [5], [n], SKIP)
        assert int(n1[0]) == int(nnz[b])
        assert t1[5:5 + n].cpu().numpy().tolist() == terms[s:s + n].tolist(), f"sequence {b}: the ids differ alone and in the batch"
        assert w1[5:5 + n].cpu().numpy().tobytes() == weights[s:s + n].tobytes(), f"sequence {b}: the weights' bits differ"


def test_lexical_weights_refusals_come_before_a_launch(dev, built_lib):
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    h = torch.zeros(64, 128, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(64, dtype=torch.float32, device=dev)

    def call(H, max_len, ld=None):
        return lib.tt_lexical_weights(h.data_ptr(), 64, H if ld is None else ld, H, h.data_ptr(), 0.0, z.data_ptr(), z.data_ptr(),
                                      z.data_ptr(), 1, max_len, 0, 2, 1, 3, z.data_ptr(), f.data_ptr(), z.data_ptr(), None)

    for H, max_len in ((192, 8), (1152, 8), (0, 8), (128, 0), (128, 8193)):
        assert call(H, max_len) == -2 and lib.tt_last_error(), (H, max_len)
    assert b"8192" in lib.tt_last_error()
    assert call(128, 8, ld=64) == -1


# ---- tt_lexical_score -------------------------------------------------------------------------------------------------------------
Q_NNZ = [0, 1, 2, 31, 32, 33, 512]
D_NNZ = [-1, 0, 1, 63, 64, 65, 511, 513, 8192]


def _score_inputs(seed):
    """Queries of Q_NNZ entries that all start with id 4 and (from two entries on) end with id 250001; documents of D_NNZ entries in
    four kinds -- no shared id, only their first entry (id 4) shared, only their last entry (id 250001) shared, every entry one of
    the longest query's -- laid out so that the entry behind a no-overlap document is id 4."""
    rng = np.random.default_rng(seed)
    even = np.arange(6, BIG_ID, 2)                           # query ids; odd ids are fillers no query holds
    q_terms, q_nnz = [], []
    for n in Q_NNZ:
        body = np.sort(rng.choice(even, max(n - 2, 0), replace=False))
        t = np.concatenate([[4][: min(n, 1)], body, [BIG_ID][: max(min(n - 1, 1), 0)]]).astype(np.int32)
        assert len(t) == n
        q_terms.append(t)
        q_nnz.append(n)
    longest = q_terms[-1]
    odd = np.arange(7, BIG_ID, 2)
    d_terms, d_nnz, kinds = [], [], []
    for n in D_NNZ:
        if n <= 0:
            d_terms.append(np.zeros(0, dtype=np.int32)); d_nnz.append(n); kinds.append("none")
            continue
        fill = lambda k: np.sort(rng.choice(odd, k, replace=False))  # noqa: E731
        variants = {"none": fill(n), "first": np.concatenate([[4], fill(n - 1)]), "last": np.concatenate([fill(n - 1), [BIG_ID]])}
        if n <= len(longest):
            inner = np.sort(rng.choice(longest[1:-1], max(n - 2, 0), replace=False))
            variants["all"] = np.concatenate([[4], inner, [BIG_ID]]) if n > 1 else np.asarray([4])
        else:
            variants["all"] = np.sort(np.concatenate([longest, fill(n - len(longest))]))
        for kind in ("none", "first", "all", "last"):        # "none" right in front of "first": one entry past it is id 4
            t = variants[kind].astype(np.int32)
            assert len(t) == n and (np.diff(t) > 0).all()
            d_terms.append(t); d_nnz.append(n); kinds.append(kind)
    def pack(parts, dtype):
        nn = np.asarray([len(p) for p in parts], dtype=np.int64)
        st = np.zeros(len(parts), dtype=np.int64)
        np.cumsum(nn[:-1], out=st[1:])
        return np.concatenate(parts).astype(np.int32), st
    qt, qs = pack(q_terms, np.int32)
    dt_, ds = pack(d_terms, np.int32)
    qw = (rng.random(len(qt)) * 3 + 0.01).astype(np.float32)
    dw = (rng.random(len(dt_)) * 3 + 0.01).astype(np.float32)
    assert 4 in qt and BIG_ID in qt and 4 in dt_ and BIG_ID in dt_
    return dict(qt=qt, qw=qw, qs=qs.astype(np.int32), qn=np.asarray(q_nnz, dtype=np.int32), dt=dt_, dw=dw, ds=ds,
                dn=np.asarray(d_nnz, dtype=np.int32), kinds=kinds)


def _lex_reference(x, a, doc, variant=None):
    """fp64 lexical score of query a and document doc -> (score, sum |q_w d_w| over the matches, matches)."""
    qs, qn = int(x["qs"][a]), int(x["qn"][a])
    ds, dn = int(x["ds"][doc]), int(x["dn"][doc])
    qt, qw = x["qt"][qs:qs + qn], x["qw"][qs:qs + qn].astype(np.float64)
    if variant == "skiplast":
        dn = max(dn - 1, 0)
    if variant == "onepast":
        dn = min(dn + 1, len(x["dt"]) - ds)
    dt_, dw = x["dt"][ds:ds + dn], x["dw"][ds:ds + dn].astype(np.float64)
    pos = np.searchsorted(qt, dt_)
    ok = pos < qn
    if variant != "union":
        ok &= qt[np.minimum(pos, max(qn - 1, 0))] == dt_ if qn else False
    prod = qw[pos[ok]] * dw[ok] if qn else np.zeros(0)
    return float(prod.sum()), float(np.abs(prod).sum()), int(ok.sum()) if qn else 0


@pytest.mark.parametrize("dim", [128, 384, 1024])
def test_lexical_score_matches_fp64(dev, built_lib, dim):
    from tensor_truth_amd import lexical

    x = _score_inputs(7 + dim)
    n_q, n_d = len(x["qn"]), len(x["dn"])
    gen = torch.Generator().manual_seed(dim)
    qd = torch.randn(n_q, dim, generator=gen).to(torch.bfloat16)
    dd = torch.randn(n_d, dim, generator=gen).to(torch.bfloat16)
    wd, wl = float(np.float32(0.4)), float(np.float32(0.2))
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    dev_args = (t(x["qt"]), t(x["qw"]), x["qs"], x["qn"], t(x["dt"]), t(x["dw"]), x["ds"], x["dn"])
    lex, dense, hyb = lexical.lexical_score(*dev_args, q_dense=qd.to(dev), d_dense=dd.to(dev), hybrid_weights=(0.4, 0.2))
    lex, dense, hyb = (v.cpu().numpy().astype(np.float64) for v in (lex, dense, hyb))
    dense64 = qd.double() @ dd.double().T
    dense_bound = (dim + 1) * U * (qd.double().abs() @ dd.double().abs().T)
    worst = {"lex": 0.0, "dense": 0.0, "hybrid": 0.0}
    teeth = {"union": 0, "skiplast": 0, "onepast": 0}
    for a in range(n_q):
        for doc in range(n_d):
            if x["dn"][doc] < 0:
                assert lex[a, doc] == -math.inf and dense[a, doc] == -math.inf and hyb[a, doc] == -math.inf, "a tombstone scores -inf"
                continue
            want, mass, matches = _lex_reference(x, a, doc)
            bound = (matches + 1) * U * mass
            kind = x["kinds"][doc]
            if x["qn"][a] == 0 or x["dn"][doc] == 0 or kind == "none":
                assert matches == 0 and lex[a, doc] == 0.0, "no shared id scores exactly 0"
            elif kind in ("first", "last"):
                assert matches == (1 if kind == "first" or x["qn"][a] >= 2 else 0)
            elif a == n_q - 1:
                assert matches == min(x["dn"][doc], x["qn"][a])
            worst["lex"] = max(worst["lex"], abs(lex[a, doc] - want) / bound if bound else abs(lex[a, doc] - want) * 1e30)
            worst["dense"] = max(worst["dense"], abs(dense[a, doc] - float(dense64[a, doc])) / float(dense_bound[a, doc]))
            formula = (wd * dense[a, doc] + wl * lex[a, doc]) / (wd + wl)
            hb = 4 * U * (abs(wd * dense[a, doc]) + abs(wl * lex[a, doc])) / (wd + wl)
            worst["hybrid"] = max(worst["hybrid"], abs(hyb[a, doc] - formula) / hb)
            for v in teeth:
                wrong = _lex_reference(x, a, doc, v)[0]
                teeth[v] += abs(wrong - want) > 2 * max(bound, U * abs(wrong))
    print(f"\nlexical score dim {dim}: max error / bound {worst}; pairs on which a wrong reference is outside the bound {teeth}")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(v > 0 for v in teeth.values()), f"a wrong reference is inside the bound on these inputs: {teeth}"

    # lexical only: the same bits, nothing else written
    lex_only, none_d, none_h = lexical.lexical_score(*dev_args)
    assert none_d is None and none_h is None and lex_only.cpu().numpy().astype(np.float64).tobytes() == lex.tobytes()
    # a pair scores the same bits alone, in a batch, at another position of cand and with cand NULL; -1 scores -inf
    rng = np.random.default_rng(dim)
    cand = rng.integers(0, n_d, (n_q, 11)).astype(np.int32)
    cand[:, 4] = -1
    cand[0, 0] = -1
    cl, cd, ch = (v.cpu().numpy().astype(np.float64) for v in lexical.lexical_score(
        *dev_args, cand=cand, q_dense=qd.to(dev), d_dense=dd.to(dev), hybrid_weights=(0.4, 0.2)))
    for a in range(n_q):
        for j in range(cand.shape[1]):
            c = cand[a, j]
            if c < 0:
                assert cl[a, j] == -math.inf and cd[a, j] == -math.inf and ch[a, j] == -math.inf
            else:
                assert (cl[a, j], cd[a, j], ch[a, j]) == (lex[a, c], dense[a, c], hyb[a, c]) or x["dn"][c] < 0
    for a, doc in ((n_q - 1, n_d - 2), (3, 9), (1, 5)):
        one = lexical.lexical_score(t(x["qt"]), t(x["qw"]), x["qs"][a:a + 1], x["qn"][a:a + 1], t(x["dt"]), t(x["dw"]), x["ds"], x["dn"],
                                    cand=[[doc]], q_dense=qd[a:a + 1].to(dev), d_dense=dd.to(dev), hybrid_weights=(0.4, 0.2))
        assert tuple(float(v[0, 0]) for v in one) == (lex[a, doc], dense[a, doc], hyb[a, doc]), "a pair alone scores other bits"


def test_lexical_score_refusals_come_before_a_launch(dev, built_lib):
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    i = torch.zeros(8, dtype=torch.int32, device=dev)
    l = torch.zeros(8, dtype=torch.int64, device=dev)
    f = torch.zeros(8, dtype=torch.float32, device=dev)
    b = torch.zeros(8, 128, dtype=torch.bfloat16, device=dev)

    def call(dim, wd, wl):
        return lib.tt_lexical_score(i.data_ptr(), f.data_ptr(), i.data_ptr(), i.data_ptr(), 1, i.data_ptr(), f.data_ptr(), l.data_ptr(),
                                    i.data_ptr(), None, 1, b.data_ptr(), b.data_ptr(), dim, wd, wl, f.data_ptr(), f.data_ptr(),
                                    f.data_ptr(), None)

    assert call(192, 0.4, 0.2) == -2 and b"dim=192" in lib.tt_last_error()
    assert call(2048, 0.4, 0.2) == -2
    assert call(128, 0.0, 0.0) == -1 and call(128, -1.0, 2.0) == -1
    assert lib.tt_lexical_scan_topk(i.data_ptr(), f.data_ptr(), i.data_ptr(), i.data_ptr(), 65, i.data_ptr(), f.data_ptr(), l.data_ptr(),
                                    i.data_ptr(), 4, 2, f.data_ptr(), i.data_ptr(), f.data_ptr(), 32, None) == -2
    assert lib.tt_lexical_scan_topk(i.data_ptr(), f.data_ptr(), i.data_ptr(), i.data_ptr(), 1, i.data_ptr(), f.data_ptr(), l.data_ptr(),
                                    i.data_ptr(), 4, 1025, f.data_ptr(), i.data_ptr(), f.data_ptr(), 32, None) == -2
    assert lib.tt_lexical_scan_topk(i.data_ptr(), f.data_ptr(), i.data_ptr(), i.data_ptr(), 1, i.data_ptr(), f.data_ptr(), l.data_ptr(),
                                    i.data_ptr(), 4, 2, f.data_ptr(), i.data_ptr(), f.data_ptr(), 8, None) == -3     # workspace too small
    assert lib.tt_lexical_scan_workspace_bytes(1000, 3) >= 3 * 1000 * 4


# ---- tt_lexical_scan_topk ---------------------------------------------------------------------------------------------------------
def _scan_inputs(n_docs, n_q, seed):
    rng = np.random.default_rng(seed)
    vocab = np.arange(10, 10 + 400)
    d_terms, d_nnz = [], []
    for d in range(n_docs):
        n = int(rng.integers(0, 12))
        d_terms.append(np.sort(rng.choice(vocab, n, replace=False)).astype(np.int32))
        d_nnz.append(-1 if (d % 7 == 3 and n_docs > 1) else n)         # tombstones keep their entries
    q_terms = [np.sort(rng.choice(vocab, int(rng.integers(1, 5)), replace=False)).astype(np.int32) for _ in range(n_q)]
    def pack(parts):
        nn = np.asarray([len(p) for p in parts], dtype=np.int64)
        st = np.zeros(len(parts), dtype=np.int64)
        np.cumsum(nn[:-1], out=st[1:])
        return (np.concatenate(parts) if nn.sum() else np.zeros(1, dtype=np.int32)).astype(np.int32), st
    qt, qs = pack(q_terms)
    dt_, ds = pack(d_terms)
    # weights on a coarse grid: equal scores between different documents are the rule, not the exception
    qw = rng.integers(1, 4, len(qt)).astype(np.float32) * 0.5
    dw = rng.integers(1, 3, len(dt_)).astype(np.float32) * 0.5
    return qt, qw, qs.astype(np.int32), np.asarray([len(p) for p in q_terms], dtype=np.int32), dt_, dw, ds, np.asarray(d_nnz, dtype=np.int32)


@pytest.mark.parametrize("n_q", [1, 3, 64])
@pytest.mark.parametrize("n_docs", [1, 63, 64, 65, 1000])
def test_lexical_scan_topk_is_the_sorted_score(dev, built_lib, n_docs, n_q):
    from tensor_truth_amd import lexical

    qt, qw, qs, qn, dt_, dw, ds, dn = _scan_inputs(n_docs, n_q, 31 * n_docs + n_q)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    args = (t(qt), t(qw), qs, qn, t(dt_), t(dw), ds, dn)
    full = lexical.lexical_score(*args)[0].cpu().numpy()
    live = dn >= 0
    assert np.isneginf(full[:, ~live]).all() and np.isfinite(full[:, live]).all()
    zeros = int((full[:, live] == 0).sum())
    assert n_docs < 63 or zeros > full[:, live].size // 3, "many documents share no id with the query"
    for k in (1, 10, 64, 65, 1024):
        scores, idx = (v.cpu().numpy() for v in lexical.lexical_scan_topk(*args, k=k))
        for a in range(n_q):
            docs = np.flatnonzero(live)
            order = docs[np.argsort(-full[a, docs], kind="stable")][:k]                 # (score desc, document asc)
            want_i = np.full(k, -1, dtype=np.int32)
            want_s = np.full(k, -np.inf, dtype=np.float32)
            want_i[:len(order)] = order
            want_s[:len(order)] = full[a, order]
            assert idx[a].tolist() == want_i.tolist(), f"n_docs {n_docs} k {k} query {a}: indices"
            assert scores[a].tobytes() == want_s.tobytes(), f"n_docs {n_docs} k {k} query {a}: scores"
        assert not np.isin(idx, np.flatnonzero(~live)).any(), "a tombstone was returned"
    print(f"\nlexical scan n_docs {n_docs} n_q {n_q}: {zeros} zero scores of {full[:, live].size}, {int((~live).sum())} tombstones")


# ---- the fixture --------------------------------------------------------------------------------------------------------------------
PRECISIONS = {"bf16": "bf16", "fp16": "fp16", "reference": "fp16"}      # precision -> the type whose e bounds it


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(GOLDEN, "m3_l2_expected.npz"))


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


def _dense_rows(lw):
    out = np.zeros((len(lw), 600))
    for i, d in enumerate(lw.as_dicts()):
        for t, v in d.items():
            out[i, t] = v
    return out


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_fixture_encoder_and_scores_within_2e_of_fp64(dev, built_lib, expected, embedders, precision):
    from tensor_truth_amd import lexical

    z, key = expected, PRECISIONS[precision]
    emb = embedders(precision)
    queries, passages = _texts(z)
    n_q = len(queries)
    before = emb.get_text_embedding_batch(passages[:5] + queries[:1])
    enc = lexical.M3Encoder(emb)
    assert enc.skip == SKIP and enc.w.dtype == emb._encoder.path.hidden
    q_dense, q_lw = enc.encode(queries, is_query=True)
    d_dense, d_lw = enc.encode(passages, is_query=False)
    assert emb.get_text_embedding_batch(passages[:5] + queries[:1]) == before, "the embedder's own output changed"
    # token ids give what the strings give, in any batch
    off = np.concatenate([[0], np.cumsum(z["lens"])])
    seqs = [z["ids"][off[i]:off[i + 1]].tolist() for i in range(len(z["lens"]))]
    d2, lw2 = enc.encode(seqs[n_q + 3:n_q + 9], is_query=False)
    assert torch.equal(d2, d_dense[3:9]) and lw2.as_dicts() == d_lw.as_dicts()[3:9]

    e = {q: float(z[f"e_{q}_{key}"]) for q in ("weights", "dense", "lex", "dense_score", "hybrid")}
    W = np.concatenate([_dense_rows(q_lw), _dense_rows(d_lw)])
    dense = torch.cat([q_dense, d_dense]).cpu().numpy().astype(np.float64)
    assert float(z["preact_margin"]) > FACTOR * e["weights"]
    assert ((W > 0) == (z["weights"] > 0)).all(), "the kept ids are not the fp64 set"
    store = lexical.LexicalStore(128, dev, capacity_terms=16, capacity_docs=2)          # (grows by doubling)
    store.add(list(range(len(passages))), d_lw, d_dense)
    hw = tuple(float(v) for v in z["hybrid_weights"])
    lex, dscore, hyb = (v.cpu().numpy().astype(np.float64) for v in
                        store.score(q_lw, np.tile(np.arange(len(passages), dtype=np.int32), (n_q, 1)), dense=q_dense, hybrid_weights=hw))
    got = {"weights": W, "dense": dense, "lex": lex, "dense_score": dscore, "hybrid": hyb}
    err = {q: float(np.abs(got[q] - z[q]).max()) for q in got}
    print(f"\nfixture {precision}: max |hip - fp64| {err}; 2 e_{key} " + str({q: FACTOR * v for q, v in e.items()}))
    for q in got:
        assert err[q] <= FACTOR * e[q], f"{q}: {err[q]:.5g} > 2 e = {FACTOR * e[q]:.5g}"
    assert (lex[z["lex"] == 0] == 0).all() and (z["lex"] == 0).any(), "a pair that shares no id scores exactly 0"
    for dn in z["defects"]:
        d = np.load(os.path.join(GOLDEN, f"m3_l2_defect_{dn}.npz"))
        gap = {q: float(np.abs(got[q] - d[q]).max()) for q in ("weights", "lex", "hybrid")}
        print(f"  defect {dn}: max |hip - defect| {gap}")
        for q, g in gap.items():
            assert g > FACTOR * e[q], f"defect {dn}: {q} is within 2 e of the implementation"
    assert (np.argsort(-hyb, 1)[:, :5] == np.argsort(-z["hybrid"], 1)[:, :5]).all(), "the fp64 top-5 order"


def _nodes(passages):
    from tensor_truth_amd.schema import NodeWithScore, TextNode

    return [NodeWithScore(node=TextNode(text=t, id_=f"p{i}"), score=0.0) for i, t in enumerate(passages)]


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_fixture_postprocessor_store_and_retriever(dev, built_lib, expected, embedders, precision):
    from tensor_truth_amd import lexical
    from tensor_truth_amd.schema import QueryBundle

    z = expected
    queries, passages = _texts(z)
    emb = embedders(precision)
    hw = tuple(float(v) for v in z["hybrid_weights"])
    make = lambda weights, top_n=5: lexical.HipM3HybridRerank(model=M3, top_n=top_n, model_kwargs={"hybrid_weights": weights, "embedder": emb})  # noqa: E731
    with pytest.raises(ValueError, match="hybrid_weights"):
        lexical.HipM3HybridRerank(model=M3, model_kwargs={"embedder": emb})
    stored, fresh, mixed = make(hw, 24), make(hw, 24), make(hw)
    assert stored.index_nodes(_nodes(passages)) == 24 and mixed.index_nodes(_nodes(passages)[::2]) == 12
    assert len(list(stored.model.parameters())) > 10 and stored.store.nbytes > 0 and len(stored.store) == 24
    for qi, q in enumerate(queries):
        a = {n.node.id_: n.score for n in stored.postprocess_nodes(_nodes(passages), QueryBundle(query_str=q))}
        b = {n.node.id_: n.score for n in fresh.postprocess_nodes(_nodes(passages), query_str=q)}
        assert a == b, "a stored node and one encoded in the call score different bits"
        top = mixed.postprocess_nodes(_nodes(passages), QueryBundle(query_str=q))
        assert [n.node.id_ for n in top] == [f"p{i}" for i in np.argsort(-z["hybrid"][qi])[:5]], "the fp64 top-5 order"
        assert [n.score for n in top] == [a[n.node.id_] for n in top]
        assert max(abs(a[f"p{i}"] - z["hybrid"][qi, i]) for i in range(24)) <= FACTOR * float(z[f"e_hybrid_{precision}"])
    assert stored.stats == {"queries": 4, "stored": 96, "encoded": 0} and fresh.stats == {"queries": 4, "stored": 0, "encoded": 96}
    assert mixed.stats == {"queries": 4, "stored": 48, "encoded": 48}
    pred = fresh.predict([(queries[1], passages[6]), (queries[1], passages[7]), (queries[2], passages[6])])
    rr = fresh.rerank(queries[1], passages[6:9], top_n=2)
    assert [r["index"] for r in rr] == [0, 1] and rr[0]["relevance_score"] == pred[0] and pred[2] < pred[1] < pred[0]

    # pure lexical and pure dense mixes
    lex_rr, dense_rr = make((0, 1), 24), make((1, 0), 24)
    lex_rr.index_nodes(_nodes(passages))
    dense_rr.index_nodes(_nodes(passages))
    e_d = float(z[f"e_dense_score_{precision}"])
    for qi, q in enumerate(queries):
        _, q_lw = lex_rr.encoder.encode([q], is_query=True)
        q_dense, _ = dense_rr.encoder.encode([q], is_query=True)
        l, d, _ = dense_rr.store.score(q_lw, np.arange(24, dtype=np.int32)[None], dense=q_dense, hybrid_weights=(1, 0))
        got_l = {n.node.id_: n.score for n in lex_rr.postprocess_nodes(_nodes(passages), query_str=q)}
        got_d = {n.node.id_: n.score for n in dense_rr.postprocess_nodes(_nodes(passages), query_str=q)}
        assert [got_l[f"p{i}"] for i in range(24)] == l[0].cpu().tolist(), "(0, 1) gives the lexical scores"
        assert [got_d[f"p{i}"] for i in range(24)] == d[0].cpu().tolist(), "(1, 0) gives the dense scores"
        order = [int(n[1:]) for n in sorted(got_d, key=lambda k: -got_d[k])]
        want = z["dense_score"][qi]
        assert order[0] == int(np.argmax(want)), "(1, 0): the best passage by the dense score"
        rank = {doc: r for r, doc in enumerate(order)}
        clear = [(i, j) for i in range(24) for j in range(24) if want[i] - want[j] > 2 * FACTOR * e_d]
        assert len(clear) > 20 and all(rank[i] < rank[j] for i, j in clear), "(1, 0) reproduces the dense ranking"

    # retrieval: the fp64 lexical order of the passages that score > 0, nothing else
    retr = lexical.HipLexicalRetriever(stored, similarity_top_k=10)
    for qi, q in enumerate(queries):
        hits = retr.retrieve(q)
        want = [i for i in np.argsort(-z["lex"][qi], kind="stable") if z["lex"][qi, i] > 0]
        assert len(want) == 6 and [n.node.id_ for n in hits] == [f"p{i}" for i in want], "the fp64 lexical order, zero scores dropped"
        assert all(n.score > 0 for n in hits) and hits[0].node.text == passages[want[0]]
    best = retr.retrieve(queries[0])[0].node.id_
    assert stored.remove_node(best) and not stored.remove_node(best) and len(stored.store) == 23
    again = retr.retrieve(queries[0])
    assert len(again) == 5 and best not in [n.node.id_ for n in again], "a removed node was returned"
    _, q_lw = stored.encoder.encode(queries[:1], is_query=True)
    scores, idx = stored.store.search(q_lw, 30)
    idx = idx[0].cpu().numpy()
    assert int(best[1:]) not in idx and (idx[23:] == -1).all() and np.isneginf(scores[0].cpu().numpy()[23:]).all()
    assert sorted(idx[:23].tolist()) == [i for i in range(24) if i != int(best[1:])], "zero-overlap documents are valid results"
    assert np.isneginf(stored.store.score(q_lw, [[int(best[1:])]])[0].cpu().numpy()).all(), "a removed document scores -inf"
    assert stored.store.lookup([best, "p1"]).tolist() == [-1, 1]
