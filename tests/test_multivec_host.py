"""CPU: the host side of BGE-M3's multi-vector head (tensor_truth_amd/multivec.py).

Checked here: ``colbert_linear.pt`` is loaded strictly (a missing file, an extra key, a non-dict, a wrong shape are refused by name;
``dim`` is read from the tensor; a ``sparse_linear.pt`` beside it is untouched); ``m3_weights`` is required and three sound numbers;
the encoder is refused for anything but an XLM-R embedder with CLS pooling whose directory ships both head files; the host wrappers
refuse lengths, widths and types outside the kernels' limits before anything is launched (CPU tensors reach the refusal);
``MultiVectorStore`` is ``TokenVectorStore`` with the wide limits, whose own checks stay; and what
tests/golden/make_m3_multivec_golden.py wrote obeys its own semantics.
"""
import os
import shutil
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M3 = os.path.join(GOLDEN, "m3_mv_l2")
HIDDEN, DIM = 128, 128


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(GOLDEN, "m3_mv_l2_expected.npz"))


@pytest.fixture
def m3_copy(tmp_path):
    return shutil.copytree(M3, str(tmp_path / "m3"))


def test_the_loader_is_strict(m3_copy, tmp_path):
    from tensor_truth_amd import lexical, multivec

    assert multivec.has_multivector_head(M3) and not multivec.has_multivector_head(os.path.join(GOLDEN, "m3_l2"))
    assert not multivec.has_multivector_head(None) and not multivec.has_multivector_head(str(tmp_path / "nowhere"))
    W, b = multivec.load_colbert_head(M3, HIDDEN)
    assert W.dtype == torch.float32 and tuple(W.shape) == (DIM, HIDDEN) and b.dtype == torch.float32 and tuple(b.shape) == (DIM,)
    assert float(b.abs().max()) > 0.5, "the fixture's bias is large enough that dropping it shows"
    path = os.path.join(m3_copy, multivec.COLBERT_FILE)
    good = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(good) == ["bias", "weight"]
    sparse_before = open(os.path.join(m3_copy, lexical.SPARSE_FILE), "rb").read()

    os.remove(path)
    with pytest.raises(FileNotFoundError, match="colbert_linear.pt"):
        multivec.load_colbert_head(m3_copy, HIDDEN)
    torch.save({**good, "sparse_linear.weight": torch.zeros(1, 2)}, path)
    with pytest.raises(NotImplementedError, match="sparse_linear.weight"):
        multivec.load_colbert_head(m3_copy, HIDDEN)
    torch.save({"weight": good["weight"]}, path)
    with pytest.raises(ValueError, match="bias"):
        multivec.load_colbert_head(m3_copy, HIDDEN)
    torch.save([good["weight"], good["bias"]], path)
    with pytest.raises(ValueError, match="state dict"):
        multivec.load_colbert_head(m3_copy, HIDDEN)
    torch.save({"weight": good["weight"][0], "bias": good["bias"]}, path)
    with pytest.raises(ValueError, match=r"weight \(128,\) does not match \[dim\]\[128\]"):
        multivec.load_colbert_head(m3_copy, HIDDEN)
    torch.save(good, path)
    with pytest.raises(ValueError, match=r"does not match \[dim\]\[1024\]"):
        multivec.load_colbert_head(m3_copy, 1024)
    torch.save({"weight": good["weight"], "bias": torch.zeros(2)}, path)
    with pytest.raises(ValueError, match=r"bias \(2,\) does not match \[128\]"):
        multivec.load_colbert_head(m3_copy, HIDDEN)
    torch.save({"weight": good["weight"], "bias": good["bias"][None]}, path)
    with pytest.raises(ValueError, match=r"bias \(1, 128\) does not match \[128\]"):
        multivec.load_colbert_head(m3_copy, HIDDEN)
    # dim is the tensor's
    torch.save({"weight": good["weight"][:96], "bias": good["bias"][:96]}, path)
    assert tuple(multivec.load_colbert_head(m3_copy, HIDDEN)[0].shape) == (96, HIDDEN)
    # the lexical head beside it is untouched and still loads
    assert open(os.path.join(m3_copy, lexical.SPARSE_FILE), "rb").read() == sparse_before
    w, _ = lexical.load_sparse_head(m3_copy, HIDDEN)
    assert tuple(w.shape) == (HIDDEN,)


def test_m3_weights_are_required_and_never_defaulted():
    from tensor_truth_amd import lexical, multivec

    for mk in (None, {}, {"torch_dtype": "bfloat16"}, {"hybrid_weights": (0.4, 0.2)}):
        with pytest.raises(ValueError, match="m3_weights"):
            multivec.HipM3AllRerank(model=M3, model_kwargs=mk)           # (refused before any weight or device is touched)
    for bad in ((0.4, 0.2), (0.4, 0.2, 0.4, 0.1), "abc", (0, 0, 0), (-1, 2, 1), (1, 1, -0.5), (float("nan"), 1, 1),
                (float("inf"), 1, 1), 3):
        with pytest.raises(ValueError, match="m3_weights"):
            multivec.check_m3_weights({"m3_weights": bad})
    assert multivec.check_m3_weights({"m3_weights": (0.4, 0.2, 0.4)}) == (0.4, 0.2, 0.4)
    assert multivec.check_m3_weights({"m3_weights": [0, 0, 1]}) == (0.0, 0.0, 1.0)
    # the two-weight check of the hybrid path stays what it was
    with pytest.raises(ValueError, match="hybrid_weights"):
        lexical.check_hybrid_weights({"hybrid_weights": (0.4, 0.2, 0.4)})


def _embedder(arch="xlmr", pooling="cls", hidden=HIDDEN, model_dir=M3):
    return types.SimpleNamespace(config=types.SimpleNamespace(arch=arch, hidden=hidden), pooling=pooling, model_dir=model_dir,
                                 model_name="fixture")


def test_anything_but_an_xlmr_cls_embedder_with_both_heads_is_refused(m3_copy):
    from tensor_truth_amd import lexical, multivec

    with pytest.raises(NotImplementedError, match="'bert'"):
        multivec.M3MultiVectorEncoder(_embedder(arch="bert"))
    with pytest.raises(NotImplementedError, match="'qwen3'"):
        multivec.M3MultiVectorEncoder(_embedder(arch="qwen3"))
    with pytest.raises(NotImplementedError, match="pooling 'mean'"):
        multivec.M3MultiVectorEncoder(_embedder(pooling="mean"))
    with pytest.raises(NotImplementedError):
        multivec.M3MultiVectorEncoder(object())
    with pytest.raises(FileNotFoundError, match="colbert_linear.pt"):
        multivec.M3MultiVectorEncoder(_embedder(model_dir=os.path.join(GOLDEN, "m3_l2")))       # (only the lexical head)
    with pytest.raises(FileNotFoundError, match="sparse_linear.pt"):
        multivec.M3MultiVectorEncoder(_embedder(model_dir=None))
    os.remove(os.path.join(m3_copy, lexical.SPARSE_FILE))
    with pytest.raises(FileNotFoundError, match="sparse_linear.pt"):
        multivec.M3MultiVectorEncoder(_embedder(model_dir=m3_copy))                             # (only the multi-vector head)


def test_a_query_of_more_than_512_vectors_is_refused_before_any_forward():
    from tensor_truth_amd import multivec

    enc = object.__new__(multivec.M3MultiVectorEncoder)          # (no embedder, no device: the refusal comes first)
    enc.max_length = 8192
    enc._tokens = lambda items, is_query: list(items)
    with pytest.raises(ValueError, match=r"query vectors\[1\]=513 is outside 0 \.\. 512"):
        enc.encode([[0, 5, 2], [0] + [5] * 512 + [2]], is_query=True)
    with pytest.raises(ValueError, match="nothing to encode"):
        enc.encode([], is_query=True)


def test_host_wrappers_refuse_before_any_launch():
    from tensor_truth_amd import multivec

    def vecs(n, dim=128, dtype=torch.bfloat16):
        return torch.zeros((n, dim), dtype=dtype)

    ok_q, ok_d = vecs(8), vecs(16)
    for q_len, msg in ((0, r"q_len\[0\]=0 is outside 1 \.\. 512"), (513, r"q_len\[0\]=513 is outside 1 \.\. 512")):
        with pytest.raises(ValueError, match=msg):
            multivec.maxsim_wide(vecs(600), [0], [q_len], ok_d, [0], [16])
    for d_len, msg in ((-1, r"d_len\[0\]=-1 is outside 0 \.\. 8192"), (8193, r"d_len\[0\]=8193 is outside 0 \.\. 8192")):
        with pytest.raises(ValueError, match=msg):
            multivec.maxsim_wide(ok_q, [0], [8], vecs(8200), [0], [d_len])
    with pytest.raises(ValueError, match="q_start"):
        multivec.maxsim_wide(ok_q, [1], [8], ok_d, [0], [16])                 # (rows past the buffer)
    with pytest.raises(ValueError, match="d_start"):
        multivec.maxsim_wide(ok_q, [0], [8], ok_d, [8], [16])
    with pytest.raises(NotImplementedError, match="dim=96"):
        multivec.maxsim_wide(vecs(8, 96), [0], [8], vecs(16, 96), [0], [16])
    with pytest.raises(NotImplementedError, match="dim=1152"):
        multivec.maxsim_wide(vecs(8, 1152), [0], [8], vecs(16, 1152), [0], [16])
    with pytest.raises(ValueError, match="one 16-bit type"):
        multivec.maxsim_wide(ok_q, [0], [8], vecs(16, dtype=torch.float16), [0], [16])
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        multivec.maxsim_wide(vecs(8, dtype=torch.float32), [0], [8], vecs(16, dtype=torch.float32), [0], [16])
    with pytest.raises(ValueError, match="document number 1"):
        multivec.maxsim_wide(ok_q, [0], [8], ok_d, [0], [16], cand=[[0, 1]])
    # within the limits the only thing missing is a device
    with pytest.raises(RuntimeError, match="no CPU path"):
        multivec.maxsim_wide(ok_q, [0], [8], ok_d, [0], [16], mean=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        multivec.maxsim_wide(vecs(512, 1024), [0], [512], vecs(8192, 1024), [0], [8192])

    h, W, b = torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(128, 128, dtype=torch.bfloat16), torch.zeros(128)
    with pytest.raises(ValueError, match="must be one of"):
        multivec.project(h, W.to(torch.float16), b, [0])
    with pytest.raises(ValueError, match="must be one of"):
        multivec.project(h.to(torch.float64), W.to(torch.float64), b, [0])
    with pytest.raises(NotImplementedError, match="dim=96"):
        multivec.project(h, W[:96].contiguous(), b[:96].contiguous(), [0])
    with pytest.raises(NotImplementedError, match="hidden size 100"):
        multivec.project(h[:, :100].contiguous(), W[:, :100].contiguous(), b, [0])
    with pytest.raises(ValueError, match="bias"):
        multivec.project(h, W, b.to(torch.float16), [0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        multivec.project(h, W, b, [0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        multivec.project(h.float(), W.float(), b, [0])
    s = torch.zeros(3)
    with pytest.raises(ValueError, match="m3_weights"):
        multivec.m3_mix(s, s, s, (0, 0, 0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        multivec.m3_mix(s, s, s, (0.4, 0.2, 0.4))


def test_the_store_carries_the_wide_limits_and_the_narrow_store_keeps_its_own():
    from tensor_truth_amd import colbert, multivec

    assert issubclass(multivec.MultiVectorStore, colbert.TokenVectorStore)
    assert (multivec.MultiVectorStore.DIM_LIMIT, multivec.MultiVectorStore.DOC_LIMIT) == (1024, 8192)
    assert (colbert.TokenVectorStore.DIM_LIMIT, colbert.TokenVectorStore.DOC_LIMIT) == (128, 512)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match=r"MultiVectorStore: dim=96 \(a multiple of 128 up to 1024\)"):
        multivec.MultiVectorStore(96, torch.bfloat16, cpu)
    with pytest.raises(ValueError, match=r"MultiVectorStore: dim=1152"):
        multivec.MultiVectorStore(1152, torch.bfloat16, cpu)
    with pytest.raises(RuntimeError, match="MultiVectorStore lives on a HIP device"):
        multivec.MultiVectorStore(1024, torch.float16, cpu)
    with pytest.raises(ValueError, match=r"TokenVectorStore: dim=160 \(a multiple of 32 up to 128\)"):
        colbert.TokenVectorStore(160, torch.bfloat16, cpu)
    with pytest.raises(ValueError, match=r"TokenVectorStore: dim=1024"):
        colbert.TokenVectorStore(1024, torch.bfloat16, cpu)
    with pytest.raises(RuntimeError, match="TokenVectorStore lives on a HIP device"):
        colbert.TokenVectorStore(128, torch.bfloat16, cpu)


def _mv(q, d, mean=True):
    m = (q @ d.T).max(1)
    return m.mean() if mean else m.sum()


def test_the_fixture_obeys_its_own_semantics(expected):
    z = expected
    n_q, lens = int(z["n_queries"]), z["lens"].astype(np.int64)
    n = len(lens)
    assert n_q == 4 and n == 28
    vstart = z["vec_start"]
    assert len(z["vec"]) == int((lens - 1).sum()), "len - 1 vectors per text"
    assert np.array_equal(vstart, np.concatenate([[0], np.cumsum(lens - 1)[:-1]]))
    vec = [z["vec"][vstart[i]:vstart[i] + lens[i] - 1] for i in range(n)]
    assert np.abs(np.linalg.norm(z["vec"], axis=1) - 1).max() < 1e-12, "unit vectors"
    mv = np.asarray([[_mv(vec[q], vec[n_q + d]) for d in range(n - n_q)] for q in range(n_q)])
    assert np.abs(mv - z["mv"]).max() < 1e-12
    wd, wl, wm = (float(v) for v in z["m3_weights"])
    assert (wd, wl, wm) == (0.4, 0.2, 0.4)
    assert np.abs(z["dense"][:n_q] @ z["dense"][n_q:].T - z["dense_score"]).max() < 1e-12
    assert np.abs((wd * z["dense_score"] + wl * z["lex"] + wm * z["mv"]) / (wd + wl + wm) - z["all"]).max() < 1e-12
    # the lexical and dense parts are m3_l2's
    z0 = np.load(os.path.join(GOLDEN, "m3_l2_expected.npz"))
    assert np.array_equal(z0["ids"], z["ids"]) and np.abs(z0["lex"] - z["lex"]).max() < 1e-9
    assert np.abs(z0["dense_score"] - z["dense_score"]).max() < 1e-9
    for q in ("vec", "mv", "all"):
        assert 0 < float(z[f"e_{q}_fp16"]) < float(z[f"e_{q}_bf16"]) < 1
    # every defect differs, by more than 4 e of every type it is listed for
    names = [str(d) for d in z["defects"]]
    assert names == ["keepbos", "dropeos", "sum", "nonorm", "nobias", "nomv"]
    fp16_only = {str(d) for d in z["defects_fp16_only"]}
    assert fp16_only <= set(names)
    for dn in names:
        d = np.load(os.path.join(GOLDEN, f"m3_mv_l2_defect_{dn}.npz"))
        assert "all" in d.files
        for q in d.files:
            gap = float(np.abs(d[q].astype(np.float64) - z[q]).max())
            for t in ("fp16",) if dn in fp16_only else ("fp16", "bf16"):
                assert gap > 4 * float(z[f"e_{q}_{t}"]), f"defect {dn}: {q} is {gap} from fp64, inside 4 e_{t}"
    # the sum defect is the mean times the query's vector count; the left-out term gives the hybrid score
    cnt = (lens[:n_q] - 1)[:, None]
    assert np.abs(np.load(os.path.join(GOLDEN, "m3_mv_l2_defect_sum.npz"))["mv"] - z["mv"] * cnt).max() < 1e-4
    hyb = (wd * z["dense_score"] + wl * z["lex"]) / (wd + wl)
    assert np.abs(np.load(os.path.join(GOLDEN, "m3_mv_l2_defect_nomv.npz"))["all"] - hyb).max() < 1e-4
    # consecutive top-5 scores stand more than 4 e of the coarser type apart
    top = -np.sort(-z["all"], 1)[:, :5]
    assert float(np.min(top[:, :-1] - top[:, 1:])) > 4 * float(z["e_all_bf16"])
    for fn in os.listdir(GOLDEN):
        if fn.startswith("m3_mv_l2"):
            p = os.path.join(GOLDEN, fn)
            for f in ([p] if os.path.isfile(p) else [os.path.join(p, x) for x in os.listdir(p)]):
                assert os.path.getsize(f) < 1 << 20, f


def test_the_lexical_module_says_where_the_third_head_is_read():
    from tensor_truth_amd import lexical, multivec

    assert "multivec.py" in lexical.__doc__ and "[UPSTREAM-K]" in multivec.__doc__
