"""CPU: the host side of exact MaxSim retrieval (tensor_truth_amd/colbert.py) -- the two new library names are bound with the
header's arity, the retriever refuses a ``similarity_top_k`` the scan cannot serve, and ``TokenVectorStore.alive`` follows ``add``,
``remove`` and a re-add.  No device: the store's arrays are host tensors here, which its bookkeeping does not mind."""
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

    ret, params = _header_params("tt_maxsim_scan_workspace_bytes")
    assert ret == "size_t" and len(params) == 2
    assert _lib.SIGNATURES["tt_maxsim_scan_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int])
    for name in ("tt_maxsim_scan_topk", "tt_maxsim_scan_topk_f16"):
        ret, params = _header_params(name)
        restype, argtypes = _lib.SIGNATURES[name]
        assert ret == "int" and restype is ctypes.c_int and len(argtypes) == len(params) == 16
        for p, a in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}[p.split()[0]]
            assert a is want, f"{name}: parameter '{p}' is bound as {a}"
    assert _lib.SIGNATURES["tt_maxsim_scan_topk"] == _lib.SIGNATURES["tt_maxsim_scan_topk_f16"]


def test_retriever_refuses_a_top_k_the_scan_cannot_serve():
    from tensor_truth_amd.colbert import MAX_SCAN_K, HipColbertRetriever

    assert MAX_SCAN_K == 1024
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="similarity_top_k"):
            HipColbertRetriever(object(), similarity_top_k=k)
    assert HipColbertRetriever(object(), similarity_top_k=1024).similarity_top_k == 1024
    assert HipColbertRetriever(object()).similarity_top_k == 10


def _host_store(dim=32, docs=2, tokens=4):
    """A ``TokenVectorStore`` whose arrays are host tensors (its constructor wants a HIP device; the bookkeeping does not)."""
    from tensor_truth_amd._stored import IdTable
    from tensor_truth_amd.colbert import TokenVectorStore

    st = object.__new__(TokenVectorStore)
    st.dim, st.dtype, st.device = dim, torch.bfloat16, torch.device("cpu")
    st.vectors = torch.empty((tokens, dim), dtype=torch.bfloat16)
    st.d_start = torch.zeros(docs, dtype=torch.int64)
    st.d_len = torch.zeros(docs, dtype=torch.int32)
    st.alive = torch.zeros(docs, dtype=torch.uint8)
    st.n_tokens = st.n_docs = 0
    st._ids, st._ws = IdTable(), None
    return st


def test_alive_follows_add_remove_and_re_add():
    st = _host_store()

    def add(ids, lens):
        return st.add(ids, torch.ones(int(sum(lens)), st.dim, dtype=torch.bfloat16), lens).tolist()

    def alive():
        return st.alive[: st.n_docs].tolist()

    assert add(["a", "b", "c"], [3, 0, 5]) == [0, 1, 2] and alive() == [1, 1, 1]          # (the arrays grew past their capacity)
    assert st.alive.dtype == torch.uint8 and st.alive.shape[0] >= 3 and not st.alive[st.n_docs:].any()
    assert st.remove("b") and not st.remove("b") and not st.remove("nope")
    assert alive() == [1, 0, 1] and st.node_id(1) is None and st.node_id(2) == "c" and st.node_id(7) is None
    # a re-add appends a new copy and kills the older number; an id given twice in one call keeps its last copy
    assert add(["a", "d", "d"], [2, 1, 1]) == [3, 4, 5]
    assert alive() == [0, 0, 1, 1, 0, 1]
    assert st.lookup(["a", "b", "c", "d"]).tolist() == [3, -1, 2, 5] and len(st) == 3
    assert [st.node_id(i) for i in range(6)] == [None, None, "c", "a", None, "d"]
    # the arrays the rerank path reads are untouched by a removal: the rows stay where they are
    assert st.d_len[: st.n_docs].tolist() == [3, 0, 5, 2, 1, 1] and st.d_start[: st.n_docs].tolist() == [0, 3, 3, 8, 10, 11]
    assert add(["b"], [4]) == [6] and alive()[-1] == 1 and st.n_tokens == 16
    assert st.nbytes == sum(t.numel() * t.element_size() for t in (st.vectors, st.d_start, st.d_len, st.alive))
    assert add([], []) == [] and st.n_docs == 7


def test_the_wide_store_is_a_rerank_stage_store():
    """``search`` refuses before it looks at a device or the library: the scan serves dim <= 128 and passages of <= 512 vectors."""
    from tensor_truth_amd.colbert import MAX_DIM, MAX_DOC_LEN, TokenVectors, TokenVectorStore
    from tensor_truth_amd.multivec import MultiVectorStore

    assert (TokenVectorStore.DIM_LIMIT, TokenVectorStore.DOC_LIMIT) == (MAX_DIM, MAX_DOC_LEN) == (128, 512)
    st = object.__new__(MultiVectorStore)
    st.dim = 1024
    with pytest.raises(NotImplementedError, match="rerank-stage"):
        st.search(TokenVectors(torch.zeros(1, 1024), np.zeros(1, np.int64), np.ones(1, np.int32)), 1)


def test_wrapper_refuses_bad_host_arguments_before_the_device():
    from tensor_truth_amd import colbert

    v = torch.zeros(8, 32, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        colbert.maxsim_scan_topk(v, [0], [4], v, [0], [4], 1)
