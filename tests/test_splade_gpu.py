"""GPU: a SPLADE checkpoint end to end (tensor_truth_amd/splade.py, csrc/splade.hip) on the fixture of
tests/golden/make_splade_golden.py, in bf16 and fp16.

* Weights, as dense vectors: ``|weights - fp64| <= 2 e_weights_<type>`` (DESIGN.md 4.8's factor for a second 16-bit implementation);
  the padding ids 600 .. 639 weigh exactly 0.
* Kept set: an id whose fp64 pre-activation is above ``2 e_pre`` must be kept, one below ``-2 e_pre`` must be absent, one inside
  the band may go either way -- and the band holds at most 5 % of a text's ids (asserted), so it cannot hide a failure.
* Scores from the store: ``lex`` within ``2 e_lex``, the fp64 order of every query's top 6, every defect file outside the bound.
* ``HipSpladeRetriever``: the fp64 top-k, ``remove_node`` removes a hit, scores are Python floats.
* ``max_terms = 8`` equals pruning the fp64 vectors, on the texts the generator recorded (8th and 9th weight more than 4 e apart).
* A text encoded alone, and in other batches, gives the bits it gives in the full batch.

Every figure is printed before it is asserted.
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SPLADE = os.path.join(GOLDEN, "splade_l2")
FACTOR = 2.0
V = 600
TYPES = {"bf16": "bfloat16", "fp16": "float16"}


@functools.lru_cache(maxsize=None)
def _expected():
    z = np.load(os.path.join(GOLDEN, "splade_l2_expected.npz"))
    return {k: z[k] for k in z.files}


def _texts():
    z = _expected()
    n_q = int(z["n_queries"])
    texts = [str(t) for t in z["texts"]]
    return texts[:n_q], texts[n_q:]


@functools.lru_cache(maxsize=None)
def _retriever(tname):
    from tensor_truth_amd.splade import HipSpladeRetriever

    return HipSpladeRetriever(model=SPLADE, similarity_top_k=6,
                              model_kwargs={"torch_dtype": TYPES[tname], "max_length": int(_expected()["max_length"])})


@functools.lru_cache(maxsize=None)
def _encoded(tname):
    """-> (LexicalWeights of the queries, of the passages): computed once per type and left unchanged."""
    enc = _retriever(tname).encoder
    queries, passages = _texts()
    return enc.encode(queries, is_query=True), enc.encode(passages, is_query=False)


def _dense(lw):
    out = np.zeros((len(lw), V))
    t, w = lw.terms.cpu().numpy(), lw.weights.cpu().numpy()
    for i, (s, n) in enumerate(zip(lw.starts, lw.nnz)):
        ids = t[s:s + n]
        assert (np.diff(ids) > 0).all() and (ids >= 0).all() and (ids < V).all(), f"text {i}: ids must be ascending, distinct and < {V}"
        out[i, ids] = w[s:s + n]
    return out


def _nodes(passages):
    from tensor_truth_amd.schema import NodeWithScore, TextNode

    return [NodeWithScore(node=TextNode(text=t, id_=f"p{i}"), score=0.0) for i, t in enumerate(passages)]


@pytest.mark.parametrize("tname", list(TYPES))
def test_weights_and_kept_set(dev, built_lib, tname):
    z = _expected()
    q_lw, d_lw = _encoded(tname)
    got = np.concatenate([_dense(q_lw), _dense(d_lw)])
    e_w, e_pre = float(z[f"e_weights_{tname}"]), float(z[f"e_pre_{tname}"])
    err = float(np.abs(got - z["weights"]).max())
    band = np.abs(z["pre"]) <= FACTOR * e_pre
    must, never = z["pre"] > FACTOR * e_pre, z["pre"] < -FACTOR * e_pre
    kept = got > 0
    print(f"\nsplade weights {tname}: max |w - w64| = {err:.5f} (2 e = {FACTOR * e_w:.5f}); band share per text up to "
          f"{band.mean(1).max():.3%}; kept {kept.sum(1).min()} .. {kept.sum(1).max()} ids; missing {int((must & ~kept).sum())}, "
          f"extra {int((never & kept).sum())}")
    assert band.mean(1).max() <= 0.05, "the test's own inputs: the band may not hold more than 5 % of a text's ids"
    assert err <= FACTOR * e_w
    assert not (must & ~kept).any(), "an id clearly above zero in fp64 is not kept"
    assert not (never & kept).any(), "an id clearly below zero in fp64 is kept"
    # the padding ids weigh exactly 0 in the dense rows the compaction reads
    enc = _retriever(tname).encoder
    rows = enc.weights_packed([z["ids"][: z["lens"][0]].tolist()]).cpu().numpy()
    assert rows.shape == (1, 640) and (rows[:, V:] == 0).all()
    for name in z["defects"]:
        d = np.load(os.path.join(GOLDEN, f"splade_l2_defect_{name}.npz"))["weights"]
        assert float(np.abs(d - got).max()) > FACTOR * e_w, f"defect {name}: its weights are inside the bound"


@pytest.mark.parametrize("tname", list(TYPES))
def test_scores_from_the_store(dev, built_lib, tname):
    from tensor_truth_amd.splade import SpladeStore

    z = _expected()
    q_lw, d_lw = _encoded(tname)
    n_q, n_d = len(q_lw), len(d_lw)
    store = SpladeStore(dev, capacity_terms=64, capacity_docs=4)        # (grows)
    docs = store.add([f"p{i}" for i in range(n_d)], d_lw)
    assert docs.tolist() == list(range(n_d)) and len(store) == n_d
    got = store.score(q_lw, np.tile(np.arange(n_d, dtype=np.int32), (n_q, 1))).cpu().numpy().astype(np.float64)
    e_lex = float(z[f"e_lex_{tname}"])
    err = float(np.abs(got - z["lex"]).max())
    print(f"\nsplade lex {tname}: max |lex - lex64| = {err:.5f} (2 e = {FACTOR * e_lex:.5f})")
    assert err <= FACTOR * e_lex
    for q in range(n_q):
        assert np.argsort(-got[q], kind="stable")[:6].tolist() == np.argsort(-z["lex"][q], kind="stable")[:6].tolist(), f"query {q}: top 6"
    scores, idx = store.search(q_lw, 6)
    for q in range(n_q):
        assert idx[q].cpu().tolist() == np.argsort(-z["lex"][q], kind="stable")[:6].tolist()
        assert np.array_equal(scores[q].cpu().numpy(), got[q][idx[q].cpu().numpy()].astype(np.float32)), "search and score differ"
    for name in z["defects"]:
        d = np.load(os.path.join(GOLDEN, f"splade_l2_defect_{name}.npz"))["lex"]
        assert float(np.abs(d - got).max()) > FACTOR * e_lex, f"defect {name}: its scores are inside the bound"
    # a tombstone
    assert store.remove("p3") and not store.remove("p3")
    again = store.score(q_lw, np.tile(np.arange(n_d, dtype=np.int32), (n_q, 1))).cpu().numpy()
    assert np.isneginf(again[:, 3]).all() and np.array_equal(np.delete(again, 3, 1), np.delete(got, 3, 1).astype(np.float32))
    assert 3 not in store.search(q_lw, 24)[1].cpu().numpy()


@pytest.mark.parametrize("tname", list(TYPES))
def test_retriever(dev, built_lib, tname):
    from tensor_truth_amd.splade import HipSpladeRetriever

    z = _expected()
    queries, passages = _texts()
    retr = HipSpladeRetriever(model=SPLADE, similarity_top_k=6,
                              model_kwargs={"torch_dtype": TYPES[tname], "max_length": int(z["max_length"])})
    assert retr.retrieve(queries[0]) == []
    assert retr.index_nodes(_nodes(passages)) == len(passages)
    e_lex = float(z[f"e_lex_{tname}"])
    for q, text in enumerate(queries):
        hits = retr.retrieve(text)
        want = np.argsort(-z["lex"][q], kind="stable")[:6]
        assert [h.node.id_ for h in hits] == [f"p{i}" for i in want], f"query {q}"
        assert all(type(h.score) is float for h in hits)
        assert max(abs(h.score - z["lex"][q][i]) for h, i in zip(hits, want)) <= FACTOR * e_lex
    best = retr.retrieve(queries[0])[0].node.id_
    assert retr.remove_node(best) and not retr.remove_node(best)
    again = [h.node.id_ for h in retr.retrieve(queries[0])]
    want = [f"p{i}" for i in np.argsort(-z["lex"][0], kind="stable")[:7]]
    assert best == want[0] and again == want[1:]


@pytest.mark.parametrize("tname", list(TYPES))
def test_max_terms_prunes_like_fp64(dev, built_lib, tname):
    z = _expected()
    enc = _retriever(tname).encoder
    queries, passages = _texts()
    texts = queries + passages
    pick = np.flatnonzero(z[f"prune8_{tname}"])
    assert len(pick) >= 1
    lw = enc.encode([texts[i] for i in pick], is_query=False, max_terms=8)
    t = lw.terms.cpu().numpy()
    print(f"\nmax_terms 8 {tname}: texts {pick.tolist()}")
    for j, i in enumerate(pick):
        assert int(lw.nnz[j]) == 8
        want = np.sort(np.argsort(-z["weights"][i], kind="stable")[:8])
        assert t[lw.starts[j]:lw.starts[j] + 8].tolist() == want.tolist(), f"text {i}: the 8 kept ids are not fp64's 8 largest"
    with pytest.raises(ValueError, match="max_terms"):
        enc.encode(texts[:1], is_query=True, max_terms=513)
    with pytest.raises(ValueError, match="max_terms"):
        enc.encode(texts[:1], max_terms=0)


@pytest.mark.parametrize("tname", list(TYPES))
def test_a_text_alone_gives_the_bits_of_the_batch(dev, built_lib, tname):
    from tensor_truth_amd.splade import SpladeEncoder

    r = _retriever(tname)
    _, passages = _texts()
    _, full = _encoded(tname)
    ft, fw = full.terms.cpu().numpy(), full.weights.cpu().numpy().view(np.int32)
    for i, text in enumerate(passages):
        one = r.encoder.encode([text])
        s, n = int(full.starts[i]), int(full.nnz[i])
        assert int(one.nnz[0]) == n and np.array_equal(one.terms.cpu().numpy(), ft[s:s + n]), f"passage {i} alone: other ids"
        assert np.array_equal(one.weights.cpu().numpy().view(np.int32), fw[s:s + n]), f"passage {i} alone: other weight bits"
    small = SpladeEncoder(r.model, r.encoder.tokenizer, max_length=r.encoder.max_length, embed_batch_size=5, forward_tokens=1)
    other = small.encode(passages)
    assert np.array_equal(other.nnz, full.nnz) and torch.equal(other.terms, full.terms)
    assert torch.equal(other.weights.view(torch.int32), full.weights.view(torch.int32)), "batches of 5: other weight bits"
    # token ids in, the same bits out
    z = _expected()
    n_q = int(z["n_queries"])
    first = np.concatenate([[0], np.cumsum(z["lens"])])
    seqs = [z["ids"][first[i]:first[i + 1]].tolist() for i in range(n_q, len(z["lens"]))]
    by_id = r.encoder.encode(seqs)
    assert torch.equal(by_id.terms, full.terms) and torch.equal(by_id.weights.view(torch.int32), full.weights.view(torch.int32))
