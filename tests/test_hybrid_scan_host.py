"""CPU: the host side of exact hybrid retrieval (tensor_truth_amd/lexical.py) -- the two new library names are bound with the
header's arity, ``tt_hybrid_scan_workspace_bytes`` is pure host and follows the lexical scan's rule, the retriever refuses a
``similarity_top_k`` the scan cannot serve, ``top_nodes`` runs a caller's search instead of the store's, and the wrapper refuses bad
host arguments before it asks for a device."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "tt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in tt_hip.h"
    return m.group(1), [p.strip() for p in m.group(2).split(",")]


def test_both_names_are_bound_with_the_headers_arity():
    import ctypes

    from tensor_truth_amd import _lib

    ret, params = _header_params("tt_hybrid_scan_workspace_bytes")
    assert ret == "size_t" and len(params) == 2
    assert _lib.SIGNATURES["tt_hybrid_scan_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    ret, params = _header_params("tt_hybrid_scan_topk")
    restype, argtypes = _lib.SIGNATURES["tt_hybrid_scan_topk"]
    assert ret == "int" and restype is ctypes.c_int and len(argtypes) == len(params) == 22
    kinds = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for p, a in zip(params, argtypes):
        want = ctypes.c_void_p if "*" in p else kinds[p.split()[0]]
        assert a is want, f"tt_hybrid_scan_topk: parameter '{p}' is bound as {a}"


def test_workspace_sizing_is_pure_host_and_the_lexical_scans_rule(built_lib):
    from tensor_truth_amd import _lib

    lib = _lib.load_library()
    for n_docs, n_q in ((0, 1), (1, 1), (31, 3), (32, 3), (33, 64), (1000, 64), (1_000_003, 17), (2**31 - 1, 64)):
        want = (n_q * ((n_docs + 31) // 32 * 32) * 4 + 255) // 256 * 256
        assert lib.tt_hybrid_scan_workspace_bytes(n_docs, n_q) == want, (n_docs, n_q)
        assert lib.tt_lexical_scan_workspace_bytes(n_docs, n_q) == want
    assert lib.tt_hybrid_scan_workspace_bytes(1000, 0) == 0 and lib.tt_hybrid_scan_workspace_bytes(1000, -3) == 0
    assert lib.tt_hybrid_scan_workspace_bytes(-1, 4) == 0


def test_retriever_refuses_a_top_k_the_scan_cannot_serve():
    from tensor_truth_amd.lexical import MAX_SCAN_K, HipM3HybridRetriever

    assert MAX_SCAN_K == 1024
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="similarity_top_k"):
            HipM3HybridRetriever(object(), similarity_top_k=k)
    assert HipM3HybridRetriever(object(), similarity_top_k=1024).similarity_top_k == 1024
    assert HipM3HybridRetriever(object()).similarity_top_k == 10


class _Store:
    """What ``top_nodes`` needs of a store, on the host."""

    postings, index, sealed = True, None, 0

    def seal(self):
        self.sealed += 1
        self.index = object()

    def search(self, query, k):
        return torch.tensor([[2.0, 0.0, -1.0][:k]]), torch.tensor([[0, 1, 2][:k]], dtype=torch.int32)

    def node_id(self, doc):
        return f"n{doc}"


def test_top_nodes_runs_the_callers_search_and_builds_no_posting_lists_for_it():
    from tensor_truth_amd._stored import top_nodes

    nodes = {f"n{i}": f"node {i}" for i in range(4)}
    hit = lambda node, score: (node, score)  # noqa: E731
    store = _Store()
    mine = lambda q, k: (torch.tensor([[0.5, -0.25, float("-inf")]]), torch.tensor([[3, 1, -1]], dtype=torch.int32))  # noqa: E731
    assert top_nodes(store, "q", 3, nodes, hit, positive_only=False, search=mine) == [("node 3", 0.5), ("node 1", -0.25)]
    assert top_nodes(store, "q", 3, nodes, hit, positive_only=True, search=mine) == [("node 3", 0.5)]
    assert store.sealed == 0, "the hybrid scan uses no posting lists"
    # without `search`: what every existing caller sees
    assert top_nodes(store, "q", 3, nodes, hit) == [("node 0", 2.0)] and store.sealed == 1
    assert top_nodes(store, "q", 3, nodes, hit, False) == [("node 0", 2.0), ("node 1", 0.0), ("node 2", -1.0)] and store.sealed == 1


def test_wrapper_refuses_bad_host_arguments_before_the_device():
    from tensor_truth_amd import lexical

    i, f = torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.float32)
    qd, dd = torch.zeros(2, 128, dtype=torch.bfloat16), torch.zeros(3, 128, dtype=torch.bfloat16)
    z2, z3 = np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int32)

    def call(q_nnz=z2, d_nnz=z3, q_dense=qd, d_dense=dd, hw=(0.4, 0.2), k=2, **kw):
        return lexical.hybrid_scan_topk(i, f, np.zeros(len(q_nnz), dtype=np.int32), q_nnz, i, f, np.zeros(len(d_nnz), dtype=np.int64),
                                        d_nnz, q_dense, d_dense, hw, k, **kw)

    with pytest.raises(ValueError, match="65 queries"):
        call(q_nnz=np.zeros(65, dtype=np.int32))
    with pytest.raises(ValueError, match="k=1025"):
        call(k=1025)
    with pytest.raises(ValueError, match="q_nnz"):
        call(q_nnz=np.asarray([0, 513], dtype=np.int32))
    with pytest.raises(ValueError, match="d_nnz"):
        call(d_nnz=np.asarray([0, -2, 0], dtype=np.int32))
    with pytest.raises(ValueError, match="d_nnz"):
        call(d_nnz=np.asarray([0, 8193, 0], dtype=np.int32))
    with pytest.raises(ValueError, match="max_q_nnz=513"):
        call(max_q_nnz=513)
    with pytest.raises(ValueError, match="hybrid_weights"):
        call(hw=(0.0, 0.0))
    with pytest.raises(ValueError, match="bfloat16"):
        call(q_dense=qd.float())
    with pytest.raises(NotImplementedError, match="dim=192"):
        call(q_dense=torch.zeros(2, 192, dtype=torch.bfloat16), d_dense=torch.zeros(3, 192, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="dense rows"):
        call(d_dense=dd[:2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        call()
