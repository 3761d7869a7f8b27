"""CPU: the MMR rule as the tests replay it (tests/mmr_refs.py) on constructed cases, and the host side of the query mode --
the retriever's keywords and their validation, and the packed single-pass scan standing aside for a retriever in MMR mode."""
import numpy as np
import pytest

import mmr_refs as mr
import tensor_truth_amd  # noqa: F401
from tensor_truth_amd import retrievers as rt
from tensor_truth_amd.schema import QueryBundle
from tensor_truth_amd.vector_index import HipVectorIndex, HipVectorRetriever


def _four_rows():
    rows, q = mr.constructed_rows(128)
    rel = (rows @ q).astype(np.float32)                       # one non-zero product per row: exact
    G = (rows.astype(np.float64) @ rows.T.astype(np.float64)).astype(np.float32)
    return rel, G


def test_constructed_rows_tie_and_orders():
    """a and its near-duplicate a' score the same bits; lambda 1 keeps the scan's order, 0.5 trades a' for b and then f, 0 looks at
    the penalty alone (all values tie at step 0: the lowest position wins)."""
    rel, G = _four_rows()
    assert rel.tolist() == [0.70703125, 0.70703125, 0.671875, 0.287109375]
    v, r, p = mr.greedy_f32(rel, G, 3, 1.0, "max")
    assert p.tolist() == [0, 1, 2] and np.array_equal(v, r) and np.array_equal(r, rel[:3])
    v, r, p = mr.greedy_f32(rel, G, 3, 0.5, "max")
    assert p.tolist() == [0, 2, 3] and np.array_equal(r, rel[[0, 2, 3]])
    assert v[0] == np.float32(0.353515625)
    assert v[1] == pytest.approx(0.0984, abs=1e-4) and v[2] == pytest.approx(0.04206, abs=1e-4)
    # what a' would have scored at step 1: a hundred roundings away from b
    assert np.float32(0.5) * rel[1] - np.float32(0.5) * G[0, 1] == pytest.approx(-0.146, abs=1e-3)
    v, r, p = mr.greedy_f32(rel, G, 3, 0.0, "max")
    assert p.tolist() == [0, 3, 2] and v[0] == 0.0
    assert v[1] == pytest.approx(-0.2030, abs=1e-4) and v[2] == pytest.approx(-0.4750, abs=1e-4)
    # k = P takes the duplicate last
    assert mr.greedy_f32(rel, G, 4, 0.5, "max")[2].tolist() == [0, 2, 3, 1]


def test_penalty_last_differs_from_max_on_five_candidates():
    """Candidates 0 and 3 are near-duplicates, 1 is unrelated to both, 2 and 4 are mildly related to everything.  After picking 0
    and then 1, "last" has forgotten 0 and takes its duplicate 3; "max" still holds 3's similarity to 0 against it."""
    rel = np.array([0.9, 0.6, 0.5, 0.88, 0.3], dtype=np.float32)
    G = np.array([[1.0, 0.0, 0.3, 0.98, 0.2],
                  [0.0, 1.0, 0.3, 0.0, 0.2],
                  [0.3, 0.3, 1.0, 0.3, 0.2],
                  [0.98, 0.0, 0.3, 1.0, 0.2],
                  [0.2, 0.2, 0.2, 0.2, 1.0]], dtype=np.float32)
    assert mr.greedy_f32(rel, G, 3, 0.5, "max")[2].tolist() == [0, 1, 2]
    assert mr.greedy_f32(rel, G, 3, 0.5, "last")[2].tolist() == [0, 1, 3]
    assert mr.greedy_f32(rel, G, 3, 0.5, 1)[2].tolist() == [0, 1, 3]
    # values of the third pick, by hand: max 0.25 - 0.5 * 0.3; last 0.44 - 0.5 * 0
    assert mr.greedy_f32(rel, G, 3, 0.5, "max")[0][2] == pytest.approx(0.1, abs=1e-6)
    assert mr.greedy_f32(rel, G, 3, 0.5, "last")[0][2] == pytest.approx(0.44, abs=1e-6)


def test_reference_padding_nan_and_ties():
    rel = np.array([0.5, 0.5, 0.4, 0.3], dtype=np.float32)
    G = np.eye(4, dtype=np.float32)
    G[2, :] = G[:, 2] = np.nan                                   # candidate 2's row went NaN: never picked once pen[2] is NaN
    v, r, p = mr.greedy_f32(rel, G, 4, 0.5, "max", valid=[True, True, True, False])
    assert p.tolist() == [0, 1, -1, -1]
    assert np.isneginf(v[2:]).all() and np.isneginf(r[2:]).all()
    # -0 == +0 is a tie: the lower position wins
    v, r, p = mr.greedy_f32(np.array([-0.0, 0.0], dtype=np.float32), np.zeros((2, 2), np.float32), 2, 1.0, "max")
    assert p.tolist() == [0, 1]


class _FakeIndex:                        # the attributes a HipVectorRetriever reads at construction (tests/test_host_logic.py)
    docstore = {}
    leaf_ids = []
    num_live = 0

    @staticmethod
    def node_score(c):
        return c


def test_retriever_accepts_and_validates_the_mmr_keywords():
    r = HipVectorRetriever(_FakeIndex(), 5, coalesce=False)
    assert (r.query_mode, r.mmr_threshold, r.mmr_prefetch_factor, r.mmr_penalty) == ("default", 0.5, 4.0, "max")
    assert HipVectorRetriever(_FakeIndex(), 5, coalesce=False, query_mode="default").query_mode == "default"
    r = HipVectorRetriever(_FakeIndex(), 5, coalesce=False, query_mode="mmr", mmr_threshold=0.25, mmr_prefetch_factor=2,
                           mmr_penalty="last")
    assert (r.query_mode, r.mmr_threshold, r.mmr_prefetch_factor, r.mmr_penalty) == ("mmr", 0.25, 2.0, "last")
    for bad in ({"mmr_threshold": -0.1}, {"mmr_threshold": 1.5}, {"mmr_threshold": float("nan")}, {"mmr_prefetch_factor": 0.5},
                {"mmr_prefetch_factor": float("nan")}, {"mmr_penalty": "mean"}):
        with pytest.raises(ValueError):
            HipVectorRetriever(_FakeIndex(), 5, coalesce=False, query_mode="mmr", **bad)
    # the index's as_retriever spells it as llama-index does and hands the keywords on
    r = HipVectorIndex.as_retriever(_FakeIndex(), similarity_top_k=7, coalesce=False, vector_store_query_mode="mmr",
                                    vector_store_kwargs={"mmr_threshold": 0.7, "mmr_prefetch_factor": 3.0, "mmr_penalty": "last"})
    assert (r.similarity_top_k, r.query_mode, r.mmr_threshold, r.mmr_prefetch_factor, r.mmr_penalty) == (7, "mmr", 0.7, 3.0, "last")
    assert HipVectorIndex.as_retriever(_FakeIndex(), similarity_top_k=7, coalesce=False).query_mode == "default"
    with pytest.raises(ValueError):
        HipVectorIndex.as_retriever(_FakeIndex(), vector_store_query_mode="mmr", vector_store_kwargs={"mmr_threshold": 2})


def test_single_pass_scan_stands_aside_for_mmr_retrievers():
    plain = [HipVectorRetriever(_FakeIndex(), 5, coalesce=False) for _ in range(2)]
    mmr = [HipVectorRetriever(_FakeIndex(), 5, coalesce=False, query_mode="mmr") for _ in range(2)]
    bundle = QueryBundle(query_str="q", embedding=[1.0, 0.0])
    assert rt.MultiIndexRetriever(mmr, enable_cache=False)._single_pass_retrieve(bundle) is None
    assert rt.MultiIndexRetriever([plain[0], mmr[0]], enable_cache=False)._single_pass_retrieve(bundle) is None
    # (two plain retrievers get past that check: the stub has no matrix to pack, which is where they stop)
    with pytest.raises(AttributeError):
        rt.MultiIndexRetriever(plain, enable_cache=False)._single_pass_retrieve(bundle)
