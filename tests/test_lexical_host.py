"""CPU: the host side of the hybrid (dense + lexical) path (tensor_truth_amd/lexical.py).

Checked here: ``sparse_linear.pt`` is loaded strictly (a missing file, an extra key, a wrong shape are refused by name); the lexical
head is refused for anything but an XLM-R embedder with CLS pooling; ``hybrid_weights`` is required; the four ids a lexical vector
leaves out are read from the tokenizer; what tests/golden/make_m3_golden.py restates (token layout, the head's tensors, the
semantics of a lexical vector) is what the package's helpers give; the host wrappers refuse lengths outside the kernels' limits
before anything is launched (no device is needed to get that far).
"""
import os
import shutil
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
M3 = os.path.join(GOLDEN, "m3_l2")
HIDDEN, VOCAB, MAX_LEN = 128, 600, 64
BOS, PAD, EOS, UNK = 0, 1, 2, 3


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(GOLDEN, "m3_l2_expected.npz"))


@pytest.fixture
def m3_copy(tmp_path):
    return shutil.copytree(M3, str(tmp_path / "m3"))


def _sequences(z):
    off = np.concatenate([[0], np.cumsum(z["lens"])])
    return [z["ids"][off[i]:off[i + 1]].tolist() for i in range(len(z["lens"]))]


def test_the_loader_is_strict(m3_copy, tmp_path):
    from tensor_truth_amd import lexical

    assert lexical.has_lexical_head(M3) and not lexical.has_lexical_head(os.path.join(GOLDEN, "colbert_l2"))
    assert not lexical.has_lexical_head(None) and not lexical.has_lexical_head(str(tmp_path / "nowhere"))
    w, b = lexical.load_sparse_head(M3, HIDDEN)
    assert w.dtype == torch.float32 and tuple(w.shape) == (HIDDEN,) and isinstance(b, float) and b < 0
    path = os.path.join(m3_copy, lexical.SPARSE_FILE)
    good = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(good) == ["bias", "weight"] and tuple(good["weight"].shape) == (1, HIDDEN) and tuple(good["bias"].shape) == (1,)

    os.remove(path)
    with pytest.raises(FileNotFoundError, match="sparse_linear.pt"):
        lexical.load_sparse_head(m3_copy, HIDDEN)
    torch.save({**good, "colbert_linear.weight": torch.zeros(2, 2)}, path)
    with pytest.raises(NotImplementedError, match="colbert_linear.weight"):
        lexical.load_sparse_head(m3_copy, HIDDEN)
    torch.save({"weight": good["weight"]}, path)
    with pytest.raises(ValueError, match="bias"):
        lexical.load_sparse_head(m3_copy, HIDDEN)
    torch.save({"weight": good["weight"][0], "bias": good["bias"]}, path)
    with pytest.raises(ValueError, match=r"weight \(128,\) does not match \[1\]\[128\]"):
        lexical.load_sparse_head(m3_copy, HIDDEN)
    torch.save({"weight": good["weight"], "bias": torch.zeros(2)}, path)
    with pytest.raises(ValueError, match=r"bias \(2,\) does not match \[1\]"):
        lexical.load_sparse_head(m3_copy, HIDDEN)
    torch.save(good, path)
    with pytest.raises(ValueError, match=r"does not match \[1\]\[1024\]"):
        lexical.load_sparse_head(m3_copy, 1024)
    torch.save([good["weight"], good["bias"]], path)
    with pytest.raises(ValueError, match="state dict"):
        lexical.load_sparse_head(m3_copy, HIDDEN)
    # a colbert_linear.pt beside it is not read
    torch.save(good, path)
    torch.save({"weight": torch.zeros(4, HIDDEN), "bias": torch.zeros(4)}, os.path.join(m3_copy, "colbert_linear.pt"))
    w2, b2 = lexical.load_sparse_head(m3_copy, HIDDEN)
    assert torch.equal(w2, w) and b2 == b


def _embedder(arch="xlmr", pooling="cls", hidden=HIDDEN, model_dir=M3):
    return types.SimpleNamespace(config=types.SimpleNamespace(arch=arch, hidden=hidden), pooling=pooling, model_dir=model_dir,
                                 model_name="fixture")


def test_anything_but_an_xlmr_embedder_with_the_head_is_refused(tmp_path):
    from tensor_truth_amd import lexical

    with pytest.raises(NotImplementedError, match="'bert'"):
        lexical.M3Encoder(_embedder(arch="bert"))
    with pytest.raises(NotImplementedError, match="'qwen3'"):
        lexical.M3Encoder(_embedder(arch="qwen3"))
    with pytest.raises(NotImplementedError, match="pooling 'mean'"):
        lexical.M3Encoder(_embedder(pooling="mean"))
    with pytest.raises(NotImplementedError, match="hidden size 192"):
        lexical.M3Encoder(_embedder(hidden=192))
    with pytest.raises(FileNotFoundError, match="sparse_linear.pt"):
        lexical.M3Encoder(_embedder(model_dir=os.path.join(GOLDEN, "colbert_l2")))
    with pytest.raises(FileNotFoundError, match="sparse_linear.pt"):
        lexical.M3Encoder(_embedder(model_dir=None))
    with pytest.raises(NotImplementedError):
        lexical.M3Encoder(object())


def test_hybrid_weights_are_required_and_never_defaulted():
    from tensor_truth_amd import lexical

    for mk in (None, {}, {"torch_dtype": "bfloat16"}):
        with pytest.raises(ValueError, match="hybrid_weights"):
            lexical.HipM3HybridRerank(model=M3, model_kwargs=mk)        # (refused before any weight or device is touched)
    for bad in ((0.4,), (0.4, 0.2, 0.1), "ab", (0, 0), (-1, 2), (float("nan"), 1), (float("inf"), 1), 3):
        with pytest.raises(ValueError, match="hybrid_weights"):
            lexical.check_hybrid_weights({"hybrid_weights": bad})
    assert lexical.check_hybrid_weights({"hybrid_weights": (0.4, 0.2)}) == (0.4, 0.2)
    assert lexical.check_hybrid_weights({"hybrid_weights": [0, 1]}) == (0.0, 1.0)
    assert lexical.check_hybrid_weights({"hybrid_weights": (1, 0)}) == (1.0, 0.0)


def test_the_special_ids_are_read_from_the_tokenizer(tmp_path):
    from tokenizers import Tokenizer, models, pre_tokenizers

    from tensor_truth_amd import lexical
    from tensor_truth_amd.tokenization import HFTokenizer, HashTokenizer, load_tokenizer

    assert lexical.special_ids(load_tokenizer(M3, "xlmr", VOCAB)) == (BOS, EOS, PAD, UNK)

    def tokenizer(specials):
        vocab = {t: i for i, t in enumerate(specials)}
        vocab.update({f"w{i}": len(specials) + i for i in range(8)})
        tk = Tokenizer(models.WordLevel(vocab, unk_token=specials[0]))
        tk.pre_tokenizer = pre_tokenizers.WhitespaceSplit()
        p = str(tmp_path / ("_".join(s.strip("<>/") or "e" for s in specials) + ".json"))
        tk.save(p)
        return HFTokenizer(p, "xlmr")

    # another order: nothing is assumed
    assert lexical.special_ids(tokenizer(["<unk>", "</s>", "<s>", "[X]", "<pad>"])) == (2, 1, 4, 0)
    with pytest.raises(ValueError, match="<pad>"):
        lexical.special_ids(tokenizer(["<unk>", "<s>", "</s>"]))
    # the hashing stand-in of synthetic weights names its own
    sp = HashTokenizer("xlmr", 1000).sp
    assert lexical.special_ids(HashTokenizer("xlmr", 1000)) == (sp.bos, sp.eos, sp.pad, sp.unk)


def test_the_fixture_restates_what_the_package_computes(expected):
    """make_m3_golden.py's layout, head and lexical-vector semantics against the package's helpers and the stored fp64 results."""
    from tensor_truth_amd import lexical
    from tensor_truth_amd.encoder import KNOWN_CONFIGS
    from tensor_truth_amd.tokenization import load_tokenizer
    from tensor_truth_amd.weights import _config_from_hf
    import json

    z = expected
    seqs = _sequences(z)
    n_q = int(z["n_queries"])
    assert (n_q, len(seqs)) == (4, 28) and max(len(s) for s in seqs) == MAX_LEN
    tk = load_tokenizer(M3, "xlmr", VOCAB)
    assert [tk.encode(str(t), MAX_LEN) for t in z["texts"]] == seqs
    assert all(s[0] == BOS and s[-1] == EOS and PAD not in s for s in seqs) and any(UNK in s for s in seqs[:n_q])
    with open(os.path.join(M3, "config.json")) as f:
        cfg = _config_from_hf(json.load(f))
    assert (cfg.arch, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.vocab_size, cfg.max_pos, cfg.pad_id, cfg.max_seq_len) == \
        ("xlmr", HIDDEN, 2, 2, 256, VOCAB, 66, PAD, MAX_LEN)
    assert KNOWN_CONFIGS["BAAI/bge-m3"].max_seq_len == lexical.MAX_SEQ_LEN == 8192      # the kernels' limit is the model's
    # the stored fp64 results obey the semantics: specials and <unk> never held, weights >= 0, only ids of the text held
    W = z["weights"]
    assert W.shape == (28, VOCAB) and (W >= 0).all() and (W[:, [BOS, PAD, EOS, UNK]] == 0).all()
    for s, row in zip(seqs, W):
        assert set(np.flatnonzero(row)) <= set(s)
    assert any((row[list(set(s) - {BOS, EOS, UNK})] == 0).any() for s, row in zip(seqs, W)), "no token of weight 0"
    assert any(len(set(s)) < len(s) for s in seqs), "no repeated token"
    lex = W[:n_q] @ W[n_q:].T
    assert np.allclose(lex, z["lex"], rtol=0, atol=1e-9) and (z["lex"] == 0).any()
    wd, wl = z["hybrid_weights"]
    assert np.allclose((wd * z["dense_score"] + wl * z["lex"]) / (wd + wl), z["hybrid"], rtol=0, atol=1e-9)
    assert np.allclose(z["dense"][:n_q] @ z["dense"][n_q:].T, z["dense_score"], rtol=0, atol=1e-9)
    assert np.allclose(np.linalg.norm(z["dense"], axis=1), 1.0, atol=1e-9)
    # LexicalWeights.as_dicts is upstream's {token id: weight} form of the same thing
    ids = [np.flatnonzero(r).astype(np.int32) for r in W]
    nnz = np.asarray([len(i) for i in ids], dtype=np.int32)
    starts = np.concatenate([[0], np.cumsum(nnz)[:-1]]).astype(np.int64)
    lw = lexical.LexicalWeights(torch.from_numpy(np.concatenate(ids)), torch.from_numpy(np.concatenate([r[i] for r, i in zip(W, ids)])
                                                                                       .astype(np.float32)), starts, nnz)
    dicts = lw.as_dicts()
    assert len(lw) == 28 and [sorted(d) for d in dicts] == [i.tolist() for i in ids]
    assert all(d[int(t)] == np.float32(r[t]) for d, r, i in zip(dicts, W, ids) for t in i)
    # every defect file differs from the expected results
    for dn in z["defects"]:
        d = np.load(os.path.join(GOLDEN, f"m3_l2_defect_{dn}.npz"))
        assert sorted(d.files) == ["hybrid", "lex", "weights"] and np.abs(d["weights"] - W).max() > 4 * float(z["e_weights_bf16"])


def test_length_arrays_are_refused_on_the_host():
    """The kernels read their length arrays from device memory and clamp; the host wrappers, which hold the values, refuse a length
    outside the documented range before anything is launched (CPU tensors get as far as the refusal)."""
    from tensor_truth_amd import lexical

    assert (lexical.MAX_SEQ_LEN, lexical.MAX_QUERY_NNZ, lexical.MAX_DOC_NNZ, lexical.MAX_HIDDEN) == (8192, 512, 8192, 1024)
    h = torch.zeros(16, 128, dtype=torch.bfloat16)
    w = torch.zeros(128, dtype=torch.bfloat16)
    ids = np.zeros(16, dtype=np.int32)
    skip = (0, 2, 1, 3)
    with pytest.raises(ValueError, match=r"seq_len\[1\]=0"):
        lexical.lexical_weights(h, w, 0.0, ids, [0, 8], [8, 0], skip)
    with pytest.raises(ValueError, match=r"seq_len\[0\]=8193"):
        lexical.lexical_weights(h, w, 0.0, ids, [0], [8193], skip)
    with pytest.raises(ValueError, match=r"seq_start\[1\]=9"):
        lexical.lexical_weights(h, w, 0.0, ids, [0, 9], [8, 8], skip)
    with pytest.raises(ValueError, match=r"seq_start\[0\]=-1"):
        lexical.lexical_weights(h, w, 0.0, ids, [-1], [8], skip)
    with pytest.raises(ValueError, match="max_len=9000"):
        lexical.lexical_weights(h, w, 0.0, ids, [0], [8], skip, max_len=9000)
    with pytest.raises(NotImplementedError, match="hidden size 192"):
        lexical.lexical_weights(torch.zeros(16, 192, dtype=torch.bfloat16), torch.zeros(192, dtype=torch.bfloat16), 0.0, ids, [0], [8], skip)
    with pytest.raises(ValueError, match="bfloat16, float16, float32"):
        lexical.lexical_weights(h, w.float(), 0.0, ids, [0], [8], skip)
    with pytest.raises(ValueError, match="four ids"):
        lexical.lexical_weights(h, w, 0.0, ids, [0], [8], (0, 1, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        lexical.lexical_weights(h, w, 0.0, ids, [0, 8], [8, 8], skip)

    t = torch.zeros(9000, dtype=torch.int32)
    v = torch.zeros(9000, dtype=torch.float32)
    args = lambda qn, dn, qs=(0,), ds=(0,): (t, v, list(qs), list(qn), t, v, list(ds), list(dn))  # noqa: E731
    with pytest.raises(ValueError, match=r"q_nnz\[0\]=513"):
        lexical.lexical_score(*args([513], [4]))
    with pytest.raises(ValueError, match=r"q_nnz\[0\]=-1"):
        lexical.lexical_score(*args([-1], [4]))
    with pytest.raises(ValueError, match=r"d_nnz\[1\]=8193"):
        lexical.lexical_score(*args([4], [-1, 8193], ds=(0, 0)))
    with pytest.raises(ValueError, match=r"d_nnz\[0\]=-2"):
        lexical.lexical_score(*args([4], [-2]))
    with pytest.raises(ValueError, match=r"d_start\[0\]=8999"):
        lexical.lexical_score(*args([4], [4], ds=(8999,)))
    with pytest.raises(ValueError, match=r"q_start\[0\]=8999"):
        lexical.lexical_score(*args([4], [4], qs=(8999,)))
    with pytest.raises(ValueError, match="document number 1 with 1 documents"):
        lexical.lexical_score(*args([4], [4]), cand=[[0, 1]])
    with pytest.raises(ValueError, match="n_cand=2"):
        lexical.lexical_score(*args([4], [4]), n_cand=2)
    qd = torch.zeros(1, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="hybrid_weights"):
        lexical.lexical_score(*args([4], [4]), q_dense=qd, d_dense=qd)
    with pytest.raises(NotImplementedError, match="dim=192"):
        lexical.lexical_score(*args([4], [4]), q_dense=torch.zeros(1, 192, dtype=torch.bfloat16),
                              d_dense=torch.zeros(1, 192, dtype=torch.bfloat16), hybrid_weights=(0.4, 0.2))
    with pytest.raises(ValueError, match="bfloat16"):
        lexical.lexical_score(*args([4], [4]), q_dense=qd.float(), d_dense=qd.float(), hybrid_weights=(0.4, 0.2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        lexical.lexical_score(*args([4], [-1]))                     # (-1: a tombstone is inside the range)

    with pytest.raises(ValueError, match="65 queries"):
        lexical.lexical_scan_topk(*args([1] * 65, [4], qs=[0] * 65), k=10)
    with pytest.raises(ValueError, match="0 queries"):
        lexical.lexical_scan_topk(*args([], [4], qs=[]), k=10)
    for k in (0, 1025):
        with pytest.raises(ValueError, match=f"k={k}"):
            lexical.lexical_scan_topk(*args([4], [4]), k=k)
    with pytest.raises(ValueError, match=r"d_nnz\[0\]=9000"):
        lexical.lexical_scan_topk(*args([4], [9000]), k=10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lexical.lexical_scan_topk(*args([4], [4]), k=10)

    with pytest.raises(RuntimeError, match="no CPU path"):
        lexical.LexicalStore(128, torch.device("cpu"))
    with pytest.raises(ValueError, match="dim=96"):
        lexical.LexicalStore(96, torch.device("cpu"))


def test_the_store_takes_dense_rows_exactly_when_it_has_them():
    """What ``LexicalStore`` (and ``SpladeStore``, the same store without dense rows) refuses before a device is touched."""
    from tensor_truth_amd import lexical
    from tensor_truth_amd.splade import SpladeStore

    cpu = torch.device("cpu")
    for make in (lambda **kw: lexical.LexicalStore(128, cpu, **kw), lambda **kw: lexical.LexicalStore(0, cpu, **kw),
                 lambda **kw: SpladeStore(cpu, **kw)):
        with pytest.raises(ValueError, match="postings=True needs vocab_size"):
            make(postings=True)
        with pytest.raises(ValueError, match="vocab_size"):
            make(postings=True, vocab_size=0)
        with pytest.raises(RuntimeError, match="lives on a HIP device"):
            make(postings=True, vocab_size=VOCAB)
    assert SpladeStore.add is lexical.LexicalStore.add and "nbytes" not in vars(SpladeStore)

    def store(cls, dim):          # (no device: ``add`` refuses before it reads an array of the store)
        st = object.__new__(cls)
        st.dim = dim
        return st

    lw = lexical.LexicalWeights(torch.zeros(1, dtype=torch.int32), torch.ones(1), np.array([0, 1]), np.array([1, 0], dtype=np.int32))
    ids = ["a", "b"]
    for st in (store(SpladeStore, 0), store(lexical.LexicalStore, 0)):
        with pytest.raises(ValueError, match="dense rows are not taken"):
            st.add(ids, lw, torch.zeros(2, 128))
        with pytest.raises(ValueError, match="3 node ids, 2 lexical vectors"):
            st.add(ids + ["c"], lw)
    st = store(lexical.LexicalStore, 128)
    with pytest.raises(ValueError, match="dense rows are needed"):
        st.add(ids, lw)
    with pytest.raises(ValueError, match=r"dense \(2, 256\) do not match \[n\]\[128\]"):
        st.add(ids, lw, torch.zeros(2, 256))
    with pytest.raises(ValueError, match=r"nnz\[0\]=8193"):
        st.add(ids, lexical.LexicalWeights(lw.terms, lw.weights, lw.starts, np.array([8193, 0])), torch.zeros(2, 128))
    with pytest.raises(ValueError, match="packed lexical vectors"):
        st.add(ids, lexical.LexicalWeights(lw.terms, lw.weights, np.array([0, 0]), lw.nnz), torch.zeros(2, 128))
