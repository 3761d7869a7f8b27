"""CPU: the host side of the late-interaction path (tensor_truth_amd/colbert.py and its dispatch in model_manager.py).

Checked here: both checkpoint layouts (stanford ``artifact.metadata``, PyLate modules) parse to the same configuration and the
same tensors; every refusal names its field; the token layout -- query ids, ``key_len``, document ids and the kept-row list -- on the
fixture's edge cases; ``model_kwargs`` overrides; the host-side limits of the kernels' length arrays; ``ModelManager``'s choice of
class for a ColBERT directory and for a cross-encoder directory.
"""
import json
import os
import shutil
import string

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STANFORD = os.path.join(GOLDEN, "colbert_l2")
PYLATE = os.path.join(GOLDEN, "colbert_l2_pylate")
CLS, SEP, MASK, QMARK, DMARK, FIRST_PUNCT, FIRST_WORD = 2, 3, 4, 5, 6, 7, 39


def _edit_json(path, **changes):
    with open(path) as f:
        d = json.load(f)
    for k, v in changes.items():
        if v is None:
            d.pop(k, None)
        else:
            d[k] = v
    with open(path, "w") as f:
        json.dump(d, f)


@pytest.fixture
def stanford_copy(tmp_path):
    return shutil.copytree(STANFORD, str(tmp_path / "st"))


@pytest.fixture
def pylate_copy(tmp_path):
    return shutil.copytree(PYLATE, str(tmp_path / "pl"))


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(GOLDEN, "colbert_l2_expected.npz"))


def _bodies(z, which):
    ids, lens = z[which + "_ids"], z[which + "_lens"]
    off = np.concatenate([[0], np.cumsum(lens)])
    return [ids[off[i]:off[i + 1]].tolist() for i in range(len(lens))]


def test_both_layouts_parse_to_the_same_configuration():
    from tensor_truth_amd import colbert

    assert colbert.detect_layout(STANFORD) == "stanford" and colbert.detect_layout(PYLATE) == "pylate"
    assert colbert.detect_layout(os.path.join(GOLDEN, "jinabert_l2")) is None      # modules.json with a Pooling: an embedder
    cfg_s, bert_s, lin_s, cc_s, _ = colbert.load_checkpoint(STANFORD)
    cfg_p, bert_p, lin_p, cc_p, _ = colbert.load_checkpoint(PYLATE)
    assert cc_s == cc_p and (cc_s.layout, cc_p.layout) == ("stanford", "pylate")
    assert cfg_s == cfg_p and (cfg_s.arch, cfg_s.hidden, cfg_s.layers, cfg_s.heads, cfg_s.ffn, cfg_s.vocab_size, cfg_s.max_pos,
                               cfg_s.num_labels) == ("bert", 128, 2, 2, 256, 600, 64, 0)
    assert (cc_s.query_length, cc_s.document_length, cc_s.dim, cc_s.attend_to_expansion_tokens) == (32, 64, 96, False)
    assert (cc_s.cls_id, cc_s.sep_id, cc_s.mask_id, cc_s.query_marker, cc_s.document_marker) == (CLS, SEP, MASK, QMARK, DMARK)
    assert cc_s.skiplist == tuple(range(FIRST_PUNCT, FIRST_WORD)) and len(cc_s.skiplist) == len(string.punctuation)
    assert sorted(bert_s) == sorted(bert_p) and all(torch.equal(bert_s[k], bert_p[k]) for k in bert_s)
    assert torch.equal(lin_s, lin_p) and tuple(lin_s.shape) == (96, 128)
    assert not any(k.startswith("pooler.") for k in bert_s)             # bert.pooler.* is tolerated and unused


def test_settings_refusals_name_the_field(stanford_copy, pylate_copy):
    from tensor_truth_amd import colbert

    meta = os.path.join(stanford_copy, "artifact.metadata")
    for field in ("query_maxlen", "doc_maxlen", "dim", "mask_punctuation", "attend_to_mask_tokens", "similarity"):
        shutil.copy(os.path.join(STANFORD, "artifact.metadata"), meta)
        _edit_json(meta, **{field: None})
        with pytest.raises(ValueError, match=f"'{field}'"):          # a missing setting is never defaulted
            colbert.load_checkpoint(stanford_copy)
    shutil.copy(os.path.join(STANFORD, "artifact.metadata"), meta)
    _edit_json(meta, similarity="l2")
    with pytest.raises(NotImplementedError, match="similarity='l2'"):
        colbert.load_checkpoint(stanford_copy)
    _edit_json(meta, similarity="cosine", brand_new_switch=True)
    with pytest.raises(NotImplementedError, match="brand_new_switch"):
        colbert.load_checkpoint(stanford_copy)
    _edit_json(meta, brand_new_switch=None, dim=48)
    with pytest.raises(ValueError, match="dim=48 does not match"):
        colbert.load_checkpoint(stanford_copy)

    cst = os.path.join(pylate_copy, "config_sentence_transformers.json")
    for field in ("query_prefix", "document_prefix", "query_length", "document_length", "attend_to_expansion_tokens", "skiplist_words"):
        shutil.copy(os.path.join(PYLATE, "config_sentence_transformers.json"), cst)
        _edit_json(cst, **{field: None})
        with pytest.raises(ValueError, match=f"'{field}'"):
            colbert.load_checkpoint(pylate_copy)
    shutil.copy(os.path.join(PYLATE, "config_sentence_transformers.json"), cst)
    _edit_json(cst, query_prefix="w1 w2 ")                             # not a single token
    with pytest.raises(ValueError, match="query_prefix='w1 w2 ' is not a single token"):
        colbert.load_checkpoint(pylate_copy)
    _edit_json(cst, query_prefix="[unused0]", pooling="mean")
    with pytest.raises(NotImplementedError, match="pooling"):
        colbert.load_checkpoint(pylate_copy)


def test_dense_backbone_dtype_and_tensor_refusals(stanford_copy, pylate_copy):
    from safetensors.torch import load_file, save_file

    from tensor_truth_amd import colbert

    dense = os.path.join(pylate_copy, "1_Dense", "config.json")
    _edit_json(dense, bias=True)
    with pytest.raises(NotImplementedError, match="bias=true"):
        colbert.load_checkpoint(pylate_copy)
    _edit_json(dense, bias=False, activation_function="torch.nn.modules.activation.Tanh")
    with pytest.raises(NotImplementedError, match="activation_function='torch.nn.modules.activation.Tanh'"):
        colbert.load_checkpoint(pylate_copy)
    shutil.copy(os.path.join(PYLATE, "1_Dense", "config.json"), dense)
    # a biased Dense by its tensors
    dst = os.path.join(pylate_copy, "1_Dense", "model.safetensors")
    t = load_file(dst)
    save_file(dict(t, **{"linear.bias": torch.zeros(96, dtype=torch.float16)}), dst)
    with pytest.raises(NotImplementedError, match="linear.bias"):
        colbert.load_checkpoint(pylate_copy)
    save_file(t, dst)
    colbert.load_checkpoint(pylate_copy)

    # backbones that are not BERT
    for mt, extra in (("modernbert", {}), ("xlm-roberta", {}), ("bert", {"position_embedding_type": "alibi"})):
        cj = os.path.join(stanford_copy, "config.json")
        shutil.copy(os.path.join(STANFORD, "config.json"), cj)
        _edit_json(cj, model_type=mt, **extra)
        with pytest.raises(NotImplementedError, match="model_type="):
            colbert.load_checkpoint(stanford_copy)
    shutil.copy(os.path.join(STANFORD, "config.json"), os.path.join(stanford_copy, "config.json"))

    # torch_dtype: bfloat16 (the default) or float16
    assert colbert.resolve_dtype(None) == torch.bfloat16 and colbert.resolve_dtype({"torch_dtype": "float16"}) == torch.float16
    assert colbert.resolve_dtype({"torch_dtype": torch.bfloat16}) == torch.bfloat16 and colbert.resolve_dtype({"precision": "fp16"}) == torch.float16
    with pytest.raises(NotImplementedError, match="torch_dtype='float32'"):
        colbert.load_checkpoint(stanford_copy, {"torch_dtype": "float32"})
    with pytest.raises(NotImplementedError, match="precision='reference'"):
        colbert.resolve_dtype({"precision": "reference"})

    # tensors: an unknown one is refused by name, a missing one too
    src = os.path.join(stanford_copy, "model.safetensors")
    t = load_file(src)
    save_file(dict(t, **{"bert.encoder.layer.0.attention.self.layer_norm_q.weight": torch.ones(128, dtype=torch.float16)}), src)
    with pytest.raises(NotImplementedError, match="layer_norm_q"):
        colbert.load_checkpoint(stanford_copy)
    save_file(dict(t, **{"cls.predictions.bias": torch.zeros(600, dtype=torch.float16)}), src)
    with pytest.raises(NotImplementedError, match="cls.predictions.bias"):      # stanford: everything but linear.weight sits under bert.
        colbert.load_checkpoint(stanford_copy)
    save_file({k: v for k, v in t.items() if k != "linear.weight"}, src)
    with pytest.raises(ValueError, match="linear.weight"):
        colbert.load_checkpoint(stanford_copy)
    save_file({k: v for k, v in t.items() if k != "bert.encoder.layer.1.output.dense.bias"}, src)
    with pytest.raises(ValueError, match="encoder.layer.1.output.dense.bias"):
        colbert.load_checkpoint(stanford_copy)


def test_token_layout(expected):
    from tensor_truth_amd import colbert

    _, _, _, cc, tk = colbert.load_checkpoint(STANFORD)
    qs, ds = _bodies(expected, "q"), _bodies(expected, "d")
    assert [len(b) for b in qs] == [1, 5, 29, 40]
    # the one-token query: [CLS] Q w [SEP], then 28 [MASK]; only the first four rows are keys
    ids, key_len = colbert.layout_query(qs[0], cc)
    assert ids == [CLS, QMARK, qs[0][0], SEP] + [MASK] * 28 and key_len == 4
    # 29 tokens fill the 32 rows exactly; 40 are cut to the same 29
    ids, key_len = colbert.layout_query(qs[2], cc)
    assert ids == [CLS, QMARK] + qs[2] + [SEP] and key_len == 32
    ids, key_len = colbert.layout_query(qs[3], cc)
    assert ids == [CLS, QMARK] + qs[3][:29] + [SEP] and key_len == 32 and len(ids) == 32
    # documents: [CLS] D body [SEP], truncated to 64; punctuation rows are dropped, the three specials never
    punct = set(range(FIRST_PUNCT, FIRST_WORD))
    all_punct = [i for i, b in enumerate(ds) if set(b) <= punct]
    assert len(all_punct) == 2
    for i in all_punct:
        ids, kept = colbert.layout_document(ds[i], cc)
        assert ids == [CLS, DMARK] + ds[i] + [SEP] and kept == [0, 1, len(ids) - 1]
    lens = []
    for b, n_kept in zip(ds, expected["d_kept"]):
        ids, kept = colbert.layout_document(b, cc)
        lens.append(len(ids))
        assert ids[:2] == [CLS, DMARK] and ids[-1] == SEP and ids[2:-1] == b[:61]
        assert kept == [i for i, t in enumerate(ids) if i in (0, 1, len(ids) - 1) or t not in punct] and len(kept) == n_kept
    assert min(lens) == 4 and max(lens) == 64 and sum(len(b) > 61 for b in ds) == 2
    # a punctuation id standing where the marker would never drops the marker row; a skiplisted [SEP] would not drop it either
    odd = colbert.ColbertConfig(**{**cc.__dict__, "skiplist": (DMARK, SEP, 40)})
    assert colbert.layout_document([40, 41], odd) == ([CLS, DMARK, 40, 41, SEP], [0, 1, 3, 4])

    # text goes through the checkpoint's tokenizer: the same ids
    enc_vocab = colbert._Vocabulary(tk)
    assert enc_vocab.body("w1 , w2!") == [FIRST_WORD + 1, FIRST_PUNCT + string.punctuation.index(","), FIRST_WORD + 2,
                                           FIRST_PUNCT + string.punctuation.index("!")]
    assert enc_vocab.single_token("[unused0]") == QMARK and enc_vocab.single_token("w1 w2") is None


def test_model_kwargs_win_over_the_files(stanford_copy):
    from tensor_truth_amd import colbert

    _, _, _, cc, _ = colbert.load_checkpoint(STANFORD, {"query_length": 16, "attend_to_expansion_tokens": True, "mask_punctuation": False})
    assert (cc.query_length, cc.attend_to_expansion_tokens, cc.skiplist, cc.document_length) == (16, True, (), 64)
    _, _, _, cc, _ = colbert.load_checkpoint(PYLATE, {"document_length": 48, "skiplist_words": [",", "w3"], "query_prefix": "w7"})
    assert (cc.document_length, cc.skiplist, cc.query_marker) == (48, (FIRST_PUNCT + string.punctuation.index(","), FIRST_WORD + 3),
                                                                  FIRST_WORD + 7)
    # the stanford spelling is an alias; and an override fills in for a field the file lacks
    _edit_json(os.path.join(stanford_copy, "artifact.metadata"), doc_maxlen=None)
    assert colbert.load_checkpoint(stanford_copy, {"doc_maxlen": 40})[3].document_length == 40
    with pytest.raises(NotImplementedError, match="query_length=200"):
        colbert.load_checkpoint(STANFORD, {"query_length": 200})
    with pytest.raises(ValueError, match="max_position_embeddings"):
        colbert.load_checkpoint(STANFORD, {"document_length": 128})


def test_length_arrays_are_refused_on_the_host():
    """The kernels read their length arrays from device memory and clamp; the host wrappers, which hold the values, refuse a length
    outside the documented range before anything is launched (no device is needed to get that far)."""
    from tensor_truth_amd import colbert

    colbert.check_key_len([32, 17], [1, 17])
    with pytest.raises(ValueError, match=r"key_len\[1\]=0"):
        colbert.check_key_len([32, 17], [5, 0])
    with pytest.raises(ValueError, match=r"key_len\[0\]=33"):
        colbert.check_key_len([32, 17], [33, 1])
    with pytest.raises(ValueError, match=r"seq_len\[0\]=129"):
        colbert.check_key_len([129], [1])
    with pytest.raises(ValueError, match=r"q_len\[1\]=129"):
        colbert._check_range("q_len", np.array([1, 129]), 1, colbert.MAX_QUERY_LEN)
    with pytest.raises(RuntimeError, match="no CPU path"):
        colbert.maxsim(torch.zeros(4, 32, dtype=torch.bfloat16), [0], [4], torch.zeros(4, 32, dtype=torch.bfloat16), [0], [4])
    with pytest.raises(RuntimeError, match="no CPU path"):
        colbert.TokenVectorStore(96, torch.bfloat16, torch.device("cpu"))


def test_model_manager_picks_the_class_by_directory(tmp_path, monkeypatch):
    from tensor_truth_amd.colbert import HipColbertRerank
    from tensor_truth_amd.model_manager import ModelManager
    from tensor_truth_amd.rerank import HipSentenceTransformerRerank

    pick = ModelManager._reranker_class
    assert pick(STANFORD, None) is HipColbertRerank and pick(PYLATE, None) is HipColbertRerank
    assert pick("colbert-ir/colbertv2.0", {"model_dir": STANFORD}) is HipColbertRerank
    # a cross-encoder directory, an embedder directory and a name without a directory go where they went
    ce = tmp_path / "ce"
    ce.mkdir()
    (ce / "config.json").write_text(json.dumps({"model_type": "bert", "architectures": ["BertForSequenceClassification"]}))
    (ce / "model.safetensors").write_bytes(b"")
    assert pick(str(ce), None) is HipSentenceTransformerRerank
    assert pick(os.path.join(GOLDEN, "jinabert_l2"), None) is HipSentenceTransformerRerank
    assert pick("BAAI/bge-reranker-v2-m3", {"synthetic_seed": 1}) is HipSentenceTransformerRerank
    # and the loader hands the class what it handed the cross-encoder class (no GPU here: stop at the constructor)
    seen = {}

    class Probe:
        def __init__(self, **kw):
            seen.update(kw)

    monkeypatch.setattr(ModelManager, "_reranker_class", staticmethod(lambda name, mk: Probe))
    mm = ModelManager()
    try:
        mm._load_reranker(STANFORD, 7, "cuda")
        assert seen["model"] == STANFORD and seen["top_n"] == 7 and seen["device"] == "cuda" and isinstance(mm._reranker, Probe)
    finally:
        ModelManager.reset_instance()
