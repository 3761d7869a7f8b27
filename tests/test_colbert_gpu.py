"""GPU: late-interaction reranking (csrc/colbert.hip, tensor_truth_amd/colbert.py).

* ``tt_maxsim[_f16]`` against fp64 on the element-rounded operands.  Products of two 16-bit values are exact in fp32, so a dot
  product of ``dim`` terms accumulated in fp32 in any order is within ``dim u A`` of the exact one, ``u = 2^-24``,
  ``A = max_ij sum_k |q_ik d_jk|``; ``|max a - max b| <= max |a - b|`` carries that to a token's maximum; the sum of ``q_len``
  maxima, each at most A, adds ``q_len u`` per term: per score ``q_len (dim + q_len) u A`` -- computed from the operands, not measured.
* ``tt_colbert_project[_f16]`` against fp64.  ``y_k = sum_h W_kh x_h`` in fp32 (exact products, any order): ``|dy_k| <= H u a_k``,
  ``a_k = sum_h |W_kh x_h|``.  The norm ``n = sqrt(sum y_k^2)`` in fp32: relative ``(dim + 4) u`` on top of ``|dy|_2 / n``.  One
  division and one rounding to the element type (unit roundoff e: 2^-8 bf16, 2^-11 fp16 with its 2^-25 subnormal half-step):
      |dv_k| <= H u a_k / n + |v_k| (H u |a|_2 / n + (dim + 8) u) + e |v_k| + e_abs,
  evaluated with the fp64 values, times (1 + 2^-10) for the second-order terms.
* ``tt_attention_keylimit[_f16]`` against an fp64 softmax over the first ``key_len`` keys, with tests/test_modernbert_gpu.py's bound
  (its module docstring) restated for a key-limit mask and both head widths; a reference that attends to all ``seq_len`` keys must
  fall outside it.
* The fixture (tests/golden/make_colbert_golden.py) through ``HipColbertRerank``: vectors and scores within 2 e_<type> of fp64
  (DESIGN.md 4.8's factor for a second 16-bit implementation, e the same torch model's own error in that type), every defect outside,
  the fp64 top-5 order, stored == encoded-in-call, the two layouts bit-equal.

Every figure is printed before it is asserted.
"""
import math
import os
import string

import numpy as np
import pytest
import torch

from test_modernbert_gpu import DTYPES, EPS, KEY, LAM, U, _pack, _ratio, _v8

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LAYOUTS = {"stanford": os.path.join(GOLDEN, "colbert_l2"), "pylate": os.path.join(GOLDEN, "colbert_l2_pylate")}
FACTOR = 2.0
Q_LENS = [1, 15, 16, 17, 32, 33, 128]
D_LENS = [0, 1, 15, 16, 17, 31, 33, 180, 512]
_DT = list(DTYPES.values())
_IDS = list(DTYPES)


# ---- MaxSim -----------------------------------------------------------------------------------------------------------------------
def _packed(lens, dim, dt, dev, gen, scale=1.0):
    lens = np.asarray(lens, dtype=np.int32)
    starts = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(lens[:-1], out=starts[1:])
    v = torch.randn(max(int(lens.sum()), 1), dim, generator=gen, device=dev) * scale
    v = torch.nn.functional.normalize(v, dim=-1).to(dt)
    return v, starts, lens


def _maxsim_reference(q, qs, ql, d, ds, dl, cand):
    """fp64 scores and their bound, [n_q][n_cand]; cand: document numbers, -1 = none."""
    n_q, n_c = cand.shape
    want = torch.zeros(n_q, n_c, dtype=torch.float64)
    bound = torch.zeros(n_q, n_c, dtype=torch.float64)
    dim = q.shape[1]
    q64, d64 = q.double().cpu(), d.double().cpu()
    for a in range(n_q):
        Q = q64[qs[a]:qs[a] + ql[a]]
        for c in range(n_c):
            doc = int(cand[a, c])
            if doc < 0:
                want[a, c] = -math.inf
                continue
            if dl[doc] == 0:
                continue
            D = d64[ds[doc]:ds[doc] + dl[doc]]
            want[a, c] = (Q @ D.T).max(-1).values.sum()
            bound[a, c] = ql[a] * (dim + ql[a]) * U * float((Q.abs() @ D.abs().T).max())
    return want, bound


def _check_scores(got, want, bound, what):
    got = got.double().cpu()
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), f"{what}: a negative candidate must score -inf"
    err = (got[~inf] - want[~inf]).abs()
    ratio = _ratio(err, bound[~inf]) if err.numel() else 0.0
    print(f"\n{what}: max error / bound = {ratio:.3f} (max abs error {err.max().item() if err.numel() else 0:.3g})")
    assert ratio <= 1.0, f"{what}: error {ratio:.3g} x its bound"


@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("n_q", [1, 3])
@pytest.mark.parametrize("dim", [32, 96, 128])
def test_maxsim_matches_fp64(dev, built_lib, dim, n_q, dt):
    from tensor_truth_amd import colbert

    gen = torch.Generator(device=dev).manual_seed(100 + dim + n_q)
    d, ds, dl = _packed(D_LENS + [33, 16], dim, dt, dev, gen)
    groups = [[n] for n in Q_LENS] if n_q == 1 else [[1, 15, 16], [17, 32, 33], [128, 16, 1]]
    rng = np.random.default_rng(dim + n_q)
    for qlens in groups:
        q, qs, ql = _packed(qlens, dim, dt, dev, gen)
        # every document, in order: the NULL form
        got = colbert.maxsim(q, qs.astype(np.int32), ql, d, ds, dl)
        cand = np.tile(np.arange(len(dl), dtype=np.int32), (n_q, 1))
        _check_scores(got, *_maxsim_reference(q, qs, ql, d, ds, dl, cand), f"maxsim dim {dim} q_len {qlens} NULL {dt}")
        got_n = colbert.maxsim(q, qs.astype(np.int32), ql, d, ds, dl, n_cand=4)
        assert torch.equal(got_n, got[:, :4])
        # candidate lists with repeats and with -1
        cand = rng.integers(-1, len(dl), (n_q, 13)).astype(np.int32)
        cand[:, 3] = cand[:, 2]
        cand[0, 0] = -1
        got_c = colbert.maxsim(q, qs.astype(np.int32), ql, d, ds, dl, cand=cand)
        _check_scores(got_c, *_maxsim_reference(q, qs, ql, d, ds, dl, cand), f"maxsim dim {dim} q_len {qlens} lists {dt}")
        # a score does not depend on the list it travels in
        flat = got.cpu()
        for a in range(n_q):
            for c in range(cand.shape[1]):
                if cand[a, c] >= 0:
                    assert got_c[a, c].item() == flat[a, cand[a, c]].item()
    assert (got[:, 0] == 0).all(), "a document of length 0 scores 0"


@pytest.mark.parametrize("dt", _DT, ids=_IDS)
def test_maxsim_negative_maxima_and_document_ends(dev, built_lib, dt):
    """Two constructed cases a wrong kernel fails: a maximum that is negative (a running maximum started at 0 returns 0), and a
    neighbour in the store whose first row is a query row (reading one row past d_len finds a perfect match)."""
    from tensor_truth_amd import colbert

    dim = 96
    gen = torch.Generator(device=dev).manual_seed(7)
    q, qs, ql = _packed([17], dim, dt, dev, gen)
    # document 0: every row is -q_5, so token 5's maximum is -|q_5|^2; document 1 (15 rows) is followed by document 2, whose first row
    # is q_9 itself
    neg = (-q[5]).repeat(16, 1)
    body, _, _ = _packed([15], dim, dt, dev, gen)
    nxt = torch.cat([q[9:10], _packed([7], dim, dt, dev, gen)[0]])
    d = torch.cat([neg, body, nxt]).contiguous()
    ds, dl = np.array([0, 16, 31], dtype=np.int64), np.array([16, 15, 8], dtype=np.int32)
    got = colbert.maxsim(q, qs.astype(np.int32), ql, d, ds, dl)
    cand = np.arange(3, dtype=np.int32)[None]
    want, bound = _maxsim_reference(q, qs, ql, d, ds, dl, cand)
    _check_scores(got, want, bound, f"maxsim constructed {dt}")
    Q, D0 = q.double().cpu(), neg.double().cpu()
    from_zero = (Q @ D0.T).max(-1).values.clamp_min(0).sum()
    assert (Q[5] @ D0.T).max() < -0.9 and abs(from_zero - want[0, 0]) > 100 * bound[0, 0]
    assert abs(got[0, 0].item() - from_zero) > bound[0, 0]
    past, _ = _maxsim_reference(q, qs, ql, d, ds, np.array([16, 16, 8], dtype=np.int32), cand)
    assert abs(past[0, 1] - want[0, 1]) > 100 * bound[0, 1] and abs(got[0, 1].item() - past[0, 1]) > bound[0, 1]


@pytest.mark.parametrize("dt", _DT, ids=_IDS)
def test_a_pair_scores_the_same_alone_in_a_batch_and_elsewhere_in_the_store(dev, built_lib, dt):
    from tensor_truth_amd import colbert

    dim = 128
    gen = torch.Generator(device=dev).manual_seed(11)
    q, qs, ql = _packed([32, 5, 128], dim, dt, dev, gen)
    d, ds, dl = _packed([180, 33, 512, 1, 64], dim, dt, dev, gen)
    batch = colbert.maxsim(q, qs.astype(np.int32), ql, d, ds, dl).cpu()
    for a in range(3):
        for c in range(5):
            alone = colbert.maxsim(q, qs[a:a + 1].astype(np.int32), ql[a:a + 1], d, ds[c:c + 1], dl[c:c + 1])
            assert alone.item() == batch[a, c].item()
    # the same documents at other offsets of a store (in reverse order behind 3 filler rows), the queries behind one filler row
    order = [4, 3, 2, 1, 0]
    d2 = torch.cat([torch.ones(3, dim, dtype=dt, device=dev)] + [d[ds[c]:ds[c] + dl[c]] for c in order]).contiguous()
    dl2 = dl[order]
    ds2 = 3 + np.concatenate([[0], np.cumsum(dl2[:-1])]).astype(np.int64)
    q2 = torch.cat([torch.ones(1, dim, dtype=dt, device=dev), q]).contiguous()
    moved = colbert.maxsim(q2, (qs + 1).astype(np.int32), ql, d2, ds2, dl2).cpu()
    assert torch.equal(moved, batch[:, order])


# ---- projection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("dim", [96, 128])
@pytest.mark.parametrize("H", [128, 384, 768])
def test_projection_matches_fp64(dev, built_lib, H, dim, dt):
    """The element bound of the module docstring: one 16-bit rounding plus fp32 accumulation over H (and over dim for the norm)."""
    from tensor_truth_amd import colbert

    gen = torch.Generator(device=dev).manual_seed(H + dim)
    n_rows = 320
    hidden = torch.randn(n_rows, H, generator=gen, device=dev).to(dt)
    hidden[7] = 0                                                   # a zero row gives zeros
    W = (torch.randn(dim, H, generator=gen, device=dev) * 0.05).to(dt)
    e = EPS[dt]
    for n_out in (1, 17, 300):
        rows = torch.randperm(n_rows, generator=torch.Generator().manual_seed(n_out))[:n_out].numpy().astype(np.int32)
        if n_out > 1:
            rows[1] = 7
        got = colbert.project(hidden, W, rows)
        assert got.shape == (n_out, dim) and got.dtype == dt
        x, w = hidden[torch.as_tensor(rows.astype(np.int64), device=dev)].double(), W.double()
        y = x @ w.T
        a = x.abs() @ w.abs().T
        n = y.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        v = y / n
        bound = (H * U * a / n + v.abs() * (H * U * a.norm(dim=-1, keepdim=True) / n + (dim + 8) * U) + e["out"] * v.abs()
                 + e["out_abs"]) * (1 + 2.0 ** -10)
        err = (got.double() - v).abs()
        ratio = _ratio(err, bound)
        print(f"\nprojection H {H} dim {dim} n_out {n_out} {dt}: max error / bound = {ratio:.3f} (max abs error {err.max().item():.3g})")
        assert ratio <= 1.0
        if n_out > 1:
            assert (got[1].view(torch.int16) == 0).all()
        # a row's bits do not depend on where in the list it stands
        again = colbert.project(hidden, W, rows[::-1].copy())
        assert torch.equal(again.flip(0), got)


# ---- key-limited attention ------------------------------------------------------------------------------------------------------------
PAIRS = [(32, 1), (32, 5), (32, 8), (32, 9), (32, 31), (32, 32), (17, 16), (64, 40), (128, 3), (128, 128)]


def _keylimit_reference(q, k, v, starts, lens, klens, heads, dh, eps=None):
    """tests/test_modernbert_gpu._window_reference with the mask 'key j is live iff j < key_len' and a head width of dh."""
    scale = 1.0 / math.sqrt(dh)
    outs, bounds = [], []
    for s0, n, kl in zip(starts, lens, klens):
        Q, K, V = (x[s0:s0 + n].double().view(n, heads, dh).transpose(0, 1) for x in (q, k, v))
        live = (torch.arange(n, device=q.device) < kl)[None, :].expand(n, n)
        S = ((Q @ K.transpose(1, 2)) * scale).masked_fill(~live, -math.inf)
        P = torch.softmax(S, dim=-1)
        O = P @ V
        outs.append(O.transpose(0, 1).reshape(n, heads * dh))
        if eps is None:
            continue
        Sa = torch.where(live, S.abs(), torch.zeros_like(S))
        dS = LAM * U * math.sqrt(dh) * (Q.abs() @ K.abs().transpose(1, 2)) * scale + 2 * U * (Sa + Sa.amax(-1, keepdim=True))
        dS = torch.where(live, dS, torch.zeros_like(dS))
        dS = dS * (1.0 + dS.amax())
        PW, Oa, Vabs = P * dS, O.abs(), V.abs()
        PV = P @ Vabs
        kn = live.sum(-1, keepdim=True).double()
        V2 = (live.double() @ V.pow(2)).sqrt()
        l_inv = torch.exp(S.amax(-1, keepdim=True) - torch.logsumexp(S, -1, keepdim=True))
        b = (PW @ Vabs + Oa * PW.sum(-1, keepdim=True) + eps["p"] * (PV + Oa) + LAM * eps["p_abs"] * V2 * l_inv
             + LAM * U * kn.sqrt() * (PV + Oa) + eps["out"] * Oa + eps["out_abs"])
        bounds.append(b.transpose(0, 1).reshape(n, heads * dh))
    return torch.cat(outs), (torch.cat(bounds) if eps is not None else None)


@pytest.mark.parametrize("dt", _DT, ids=_IDS)
@pytest.mark.parametrize("mode", ["alt", "tight", "aligned"])
@pytest.mark.parametrize("dh", [32, 64])
def test_keylimited_attention_matches_fp64(dev, built_lib, dh, mode, dt):
    from tensor_truth_amd import colbert

    heads = 3
    H = heads * dh
    lens, klens = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    starts, T = _pack(lens, mode)
    gen = torch.Generator(device=dev).manual_seed(31 + dh)
    q, k, v = (torch.randn(T, H, generator=gen, device=dev) * s for s in (1.5, 1.5, 1.0))
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    qkv = torch.cat([q, k, v], dim=1).contiguous()
    out = torch.zeros(T, H, dtype=dt, device=dev)
    colbert.attention_keylimit(qkv, 0, H, _v8(v), out, starts, lens, klens, heads, dh)
    torch.cuda.synchronize()
    live = torch.zeros(T, dtype=torch.bool, device=dev)
    for s, n in zip(starts, lens):
        live[s:s + n] = True
    assert (out[~live].view(torch.int16) == 0).all(), "rows of no sequence stay zero"
    got = torch.cat([out[s:s + n] for s, n in zip(starts, lens)])
    assert torch.isfinite(got.float()).all()
    want, bound = _keylimit_reference(q, k, v, starts, lens, klens, heads, dh, EPS[dt])
    err = (got.double() - want).abs()
    ratio = _ratio(err, bound)
    print(f"\nkey-limited attention dh {dh} {mode} {dt}: max error / bound = {ratio:.3f} (max abs error {err.max().item():.3g})")
    assert ratio <= 1.0
    # teeth: attending to all seq_len keys, and to one key more or fewer, lies outside the bound
    for other_k in (lens, [min(kl + 1, n) for kl, n in zip(klens, lens)], [max(kl - 1, 1) for kl in klens]):
        other, _ = _keylimit_reference(q, k, v, starts, lens, other_k, heads, dh)
        gap = _ratio((other - want).abs(), bound)
        assert gap > 2.0, f"the fp64 references are only {gap:.3g} bounds apart on these inputs"
        assert _ratio((got.double() - other).abs(), bound) > 1.0


# ---- the fixture through HipColbertRerank ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected():
    z = np.load(os.path.join(GOLDEN, "colbert_l2_expected.npz"))
    out = {k: z[k] for k in z.files}

    def bodies(which):
        ids, lens = out[which + "_ids"], out[which + "_lens"]
        off = np.concatenate([[0], np.cumsum(lens)])
        return [ids[off[i]:off[i + 1]].tolist() for i in range(len(lens))]

    out["q_bodies"], out["d_bodies"] = bodies("q"), bodies("d")
    out["defect"] = {str(d): dict(np.load(os.path.join(GOLDEN, f"colbert_l2_defect_{d}.npz"))) for d in out["defects"]}
    return out


_RERANKERS = {}


def _reranker(layout, dtype, dev):
    """One instance per (layout, type) for the module: loading is the slow part."""
    from tensor_truth_amd.colbert import HipColbertRerank

    key = (layout, dtype)
    if key not in _RERANKERS:
        _RERANKERS[key] = HipColbertRerank(model=LAYOUTS[layout], top_n=5, device=str(dev), model_kwargs={"torch_dtype": dtype})
    return _RERANKERS[key]


def _rowwise_gap(a, a_lens, b, b_lens):
    """max |a - b| sequence by sequence, row for row up to the shorter one (a defect may add or drop rows)."""
    gap, oa, ob = 0.0, 0, 0
    for la, lb in zip(a_lens, b_lens):
        n = min(la, lb)
        if n:
            gap = max(gap, float(np.abs(a[oa:oa + n] - b[ob:ob + n]).max()))
        oa, ob = oa + la, ob + lb
    return gap


def _text(body):
    """The fixture's word-level vocabulary: ids 7 .. 38 are string.punctuation's characters, 39 + i is the word w<i>."""
    return " ".join(string.punctuation[t - 7] if t < 39 else f"w{t - 39}" for t in body)


@pytest.mark.parametrize("dtype", _IDS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fixture_vectors_scores_and_ranking(dev, built_lib, expected, layout, dtype):
    from tensor_truth_amd import colbert

    rr = _reranker(layout, dtype, dev)
    enc, key = rr.encoder, KEY[dtype]
    e_vec, e_score = float(expected[f"e_vec_{key}"]), float(expected[f"e_score_{key}"])
    qv, dv = enc.encode_queries(expected["q_bodies"]), enc.encode_documents(expected["d_bodies"])
    assert qv.lens.tolist() == [32] * 4 and dv.lens.tolist() == expected["d_kept"].tolist()
    got_q, got_d = qv.vectors.double().cpu().numpy(), dv.vectors.double().cpu().numpy()
    err_q, err_d = np.abs(got_q - expected["q_vec"]).max(), np.abs(got_d - expected["d_vec"]).max()
    print(f"\n{layout} {dtype}: |vec - fp64| queries {err_q:.3g} documents {err_d:.3g}; e_vec {e_vec:.3g} (bound {FACTOR * e_vec:.3g})")
    scores = colbert.maxsim(qv.vectors, qv.starts.astype(np.int32), qv.lens, dv.vectors, dv.starts, dv.lens).double().cpu().numpy()
    err_s = np.abs(scores - expected["scores"]).max()
    print(f"{layout} {dtype}: |score - fp64| {err_s:.3g}; e_score {e_score:.3g} (bound {FACTOR * e_score:.3g})")
    assert max(err_q, err_d) <= FACTOR * e_vec
    assert err_s <= FACTOR * e_score
    # every applicable defect lies outside those bounds
    fp16_only = set(expected["defects_fp16_only"].tolist())
    for name, ref in expected["defect"].items():
        for quantity, arr in ref.items():
            if key == "bf16" and f"{name}:{quantity}" in fp16_only:
                continue
            if quantity == "score":
                gap, lim = np.abs(scores - arr).max(), FACTOR * e_score
            elif quantity == "q_vec":
                gap, lim = _rowwise_gap(got_q, [32] * 4, arr, [32] * 4), FACTOR * e_vec
            else:
                kept = expected["d_kept"].tolist()
                extra = (len(arr) - sum(kept)) // len(kept)         # nomarker: one row fewer per document
                gap, lim = _rowwise_gap(got_d, kept, arr, [n + extra for n in kept]), FACTOR * e_vec
            print(f"{layout} {dtype}: defect {name}:{quantity} is {gap:.3g} away (bound {lim:.3g})")
            assert gap > lim, f"defect {name}:{quantity} is inside the bound"
    # the fp64 top-5 order for all four queries
    for a in range(4):
        assert np.argsort(-scores[a])[:5].tolist() == np.argsort(-expected["scores"][a])[:5].tolist(), f"query {a}"


def _all_scores(rr, nodes, **query):
    """node id -> score of EVERY node (top_n lifted for the call)."""
    top_n, rr.top_n = rr.top_n, len(nodes)
    try:
        return {n.node.id_: n.score for n in rr.postprocess_nodes(nodes, **query)}
    finally:
        rr.top_n = top_n


@pytest.mark.parametrize("dtype", _IDS)
def test_stored_and_encoded_in_call_are_bit_equal_and_the_surface_holds(dev, built_lib, expected, dtype):
    from tensor_truth_amd.colbert import HipColbertRerank
    from tensor_truth_amd.schema import NodeWithScore, QueryBundle, TextNode

    rr = HipColbertRerank(model=LAYOUTS["stanford"], top_n=5, device=str(dev), keep_retrieval_score=True,
                          model_kwargs={"torch_dtype": dtype})
    assert sum(p.numel() * p.element_size() for p in rr.model.parameters()) == rr.model.nbytes() > 0
    texts = [_text(b) for b in expected["d_bodies"]]
    query = _text(expected["q_bodies"][2])

    def nodes():
        return [NodeWithScore(node=TextNode(text=t, id_=f"n{i}"), score=0.5) for i, t in enumerate(texts)]

    assert rr.postprocess_nodes([], query_str=query) == []
    with pytest.raises(ValueError, match="Missing query"):
        rr.postprocess_nodes(nodes())
    fresh = rr.postprocess_nodes(nodes(), QueryBundle(query_str=query))                 # positional, nothing stored
    assert rr.stats["stored"] == 0 and len(fresh) == 5 and all(type(n.score) is float for n in fresh)
    assert [n.score for n in fresh] == sorted((n.score for n in fresh), reverse=True) and fresh[0].node.metadata["retrieval_score"] == 0.5
    # text goes through the tokenizer to the fixture's ids: the fixture's fp64 order
    assert [n.node.id_ for n in fresh] == [f"n{i}" for i in np.argsort(-expected["scores"][2])[:5]]
    all_fresh = _all_scores(rr, nodes(), query_str=query)

    # half stored, then all stored: the same floats
    assert rr.index_nodes(nodes()[::2]) == 12 and len(rr.store) == 12
    rr.stats.update(stored=0, encoded=0)
    mixed = _all_scores(rr, nodes(), query_bundle=QueryBundle(query_str=query))
    assert (rr.stats["stored"], rr.stats["encoded"]) == (12, 12) and mixed == all_fresh
    rr.index_nodes([n.node for n in nodes()[1::2]])
    stored = _all_scores(rr, nodes(), query_str=query)
    assert rr.stats["encoded"] == 12 and stored == all_fresh

    # remove, then add again: scored in the call in between, from the store (a new copy) afterwards; the old rows are not reclaimed
    tokens, nbytes = rr.store.n_tokens, rr.store.nbytes
    assert rr.store.remove("n3") and not rr.store.remove("n3") and rr.store.lookup(["n3", "n4", "nope"]).tolist()[::2] == [-1, -1]
    rr.stats.update(stored=0, encoded=0)
    again = _all_scores(rr, nodes(), query_str=query)
    assert (rr.stats["stored"], rr.stats["encoded"]) == (23, 1) and again == all_fresh
    rr.index_nodes(nodes()[3:4])
    assert rr.store.lookup(["n3"])[0] == 24 and rr.store.n_tokens == tokens + int(expected["d_kept"][3]) and rr.store.nbytes >= nbytes
    assert _all_scores(rr, nodes(), query_str=query) == all_fresh

    # predict / rerank: the same scores from pairs of strings
    pairs = [(query, t) for t in texts[:6]] + [(_text(expected["q_bodies"][1]), texts[4])]
    pred = rr.predict(pairs)
    assert pred[:6] == [all_fresh[f"n{i}"] for i in range(6)] and rr.predict([]) == []
    ranked = rr.rerank(query, texts, top_n=3)
    assert [r["index"] for r in ranked] == np.argsort(-expected["scores"][2])[:3].tolist()
    assert ranked[0]["relevance_score"] == all_fresh[f"n{ranked[0]['index']}"]


@pytest.mark.parametrize("dtype", _IDS)
def test_the_two_layouts_are_bit_equal(dev, built_lib, expected, dtype):
    a, b = _reranker("stanford", dtype, dev), _reranker("pylate", dtype, dev)
    assert a.settings == b.settings
    for fn, items in (("encode_queries", expected["q_bodies"]), ("encode_documents", expected["d_bodies"])):
        va, vb = getattr(a.encoder, fn)(items), getattr(b.encoder, fn)(items)
        assert torch.equal(va.vectors, vb.vectors) and va.lens.tolist() == vb.lens.tolist()
    # and documents encoded one at a time are the bits of the batch
    whole = a.encoder.encode_documents(expected["d_bodies"])
    for i in (0, 8, 23):
        one = a.encoder.encode_documents(expected["d_bodies"][i:i + 1])
        assert torch.equal(one.vectors, whole.vectors[whole.starts[i]:whole.starts[i] + whole.lens[i]])


def test_attending_to_expansion_tokens_takes_the_plain_forward(dev, built_lib, expected):
    """``attend_to_expansion_tokens`` (an override here): the query runs through tt_encoder_forward -- and a key_len equal to the
    sequence length is that forward's attention up to the kernel's own rounding."""
    from tensor_truth_amd.colbert import HipColbertRerank

    rr = HipColbertRerank(model=LAYOUTS["stanford"], device=str(dev), model_kwargs={"attend_to_expansion_tokens": True})
    assert rr.settings.attend_to_expansion_tokens
    got = rr.encoder.encode_queries(expected["q_bodies"]).vectors.double().cpu().numpy()
    ref = expected["defect"]["attendmask"]["q_vec"]
    lim = FACTOR * float(expected["e_vec_bf16"])
    err = np.abs(got - ref).max()
    print(f"\nattended expansion tokens: |vec - fp64 attendmask| {err:.3g} (bound {lim:.3g})")
    assert err <= lim


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["", "_f16"])
def test_bad_arguments_refused_before_a_launch(dev, built_lib, sfx):
    from tensor_truth_amd import _lib, colbert

    lib = _lib.load_library()
    st = torch.cuda.current_stream(dev).cuda_stream
    dt = torch.float16 if sfx else torch.bfloat16
    buf = torch.zeros(1024, 128, dtype=dt, device=dev)
    i32 = torch.ones(8, dtype=torch.int32, device=dev)
    i64 = torch.zeros(8, dtype=torch.int64, device=dev)
    f32 = torch.zeros(64, dtype=torch.float32, device=dev)

    def refused(rc, text):
        assert rc != 0 and text in lib.tt_last_error().decode(), lib.tt_last_error()

    for dim in (48, 0, 160):
        refused(getattr(lib, "tt_maxsim" + sfx)(buf.data_ptr(), i32.data_ptr(), i32.data_ptr(), 1, buf.data_ptr(), i64.data_ptr(),
                                                i32.data_ptr(), None, 1, dim, f32.data_ptr(), st), f"dim={dim}")
        refused(getattr(lib, "tt_colbert_project" + sfx)(buf.data_ptr(), 8, 128, buf.data_ptr(), dim, i32.data_ptr(), 1, buf.data_ptr(), st),
                f"dim={dim}")
    refused(getattr(lib, "tt_colbert_project" + sfx)(buf.data_ptr(), 8, 100, buf.data_ptr(), 96, i32.data_ptr(), 1, buf.data_ptr(), st),
            "hidden=100")
    refused(getattr(lib, "tt_maxsim" + sfx)(None, i32.data_ptr(), i32.data_ptr(), 1, buf.data_ptr(), i64.data_ptr(), i32.data_ptr(), None, 1,
                                            96, f32.data_ptr(), st), "null pointer")
    att = getattr(lib, "tt_attention_keylimit" + sfx)
    args = lambda hd, max_len: (buf.data_ptr(), 128, 0, 64, buf.data_ptr(), 8 * 64, buf.data_ptr(), 64, i32.data_ptr(), i32.data_ptr(),  # noqa: E731
                                i32.data_ptr(), 1, 64 // hd if hd in (32, 64) else 1, hd, max_len, st)
    refused(att(*args(48, 32)), "head_dim=48")
    refused(att(*args(64, 129)), "max_len=129")
    refused(att(*args(64, 0)), "max_len=0")
    # the length arrays live in device memory: the host wrappers, which hold the values, refuse them before anything is launched
    v = buf[:, :96].contiguous()
    with pytest.raises(ValueError, match=r"q_len\[0\]=129"):
        colbert.maxsim(v, [0], [129], v, [0], [4])
    with pytest.raises(ValueError, match=r"q_len\[0\]=0"):
        colbert.maxsim(v, [0], [0], v, [0], [4])
    with pytest.raises(ValueError, match=r"d_len\[1\]=513"):
        colbert.maxsim(v, [0], [4], v, [0, 4], [4, 513])
    with pytest.raises(ValueError, match=r"d_start\[0\]=1020"):
        colbert.maxsim(v, [0], [4], v, [1020], [8])
    with pytest.raises(ValueError, match="document number 2"):
        colbert.maxsim(v, [0], [4], v, [0, 4], [4, 4], cand=[[0, 2]])
    out = torch.zeros(256, 64, dtype=dt, device=dev)
    qkv = torch.zeros(256, 192, dtype=dt, device=dev)
    for klen, text in (([0], r"key_len\[0\]=0"), ([33], r"key_len\[0\]=33")):
        with pytest.raises(ValueError, match=text):
            colbert.attention_keylimit(qkv, 0, 64, qkv[:, 128:].reshape(32, 8, 64).permute(0, 2, 1).contiguous(), out, [0], [32], klen, 1, 64)
    store = colbert.TokenVectorStore(96, dt, dev)
    with pytest.raises(ValueError, match=r"lens\[0\]=513"):
        store.add(["a"], torch.zeros(513, 96, dtype=dt, device=dev), [513])
    assert (out == 0).all()
