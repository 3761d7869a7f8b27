"""CPU: the SPLADE loader (tensor_truth_amd/splade.py) on copies of the fixture tests/golden/splade_l2 edited in ``tmp_path`` -- what
it accepts (the plain Hugging Face directory, the sentence-transformers ``SparseEncoder`` directory, a tied and an untied decoder,
tensors it ignores by name) and everything it refuses by name.  No GPU, no library call."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "golden", "splade_l2")
HEAD = "cls.predictions."
ST_MODULES = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.sparse_encoder.models.MLMTransformer"},
              {"idx": 1, "name": "1", "path": "1_SpladePooling", "type": "sentence_transformers.sparse_encoder.models.SpladePooling"}]
ST_POOLING = {"pooling_strategy": "max", "activation_function": "relu", "word_embedding_dimension": 600}


@pytest.fixture
def ts():
    from tensor_truth_amd import splade

    return splade


@pytest.fixture
def plain(tmp_path):
    d = str(tmp_path / "splade")
    shutil.copytree(SRC, d)
    return d


def _edit_json(path, **fields):
    with open(path) as f:
        d = json.load(f)
    for k, v in fields.items():
        if v is None:
            d.pop(k, None)
        else:
            d[k] = v
    with open(path, "w") as f:
        json.dump(d, f)


def _edit_state(d, fn):
    p = os.path.join(d, "model.safetensors")
    sd = dict(load_file(p))
    fn(sd)
    save_file({k: v.contiguous() for k, v in sd.items()}, p, metadata={"format": "pt"})


def _as_sparse_encoder(d, pooling=None, modules=None, sbert=None):
    """The three JSON files that make the plain directory a sentence-transformers SparseEncoder directory."""
    with open(os.path.join(d, "modules.json"), "w") as f:
        json.dump(ST_MODULES if modules is None else modules, f)
    os.makedirs(os.path.join(d, "1_SpladePooling"), exist_ok=True)
    with open(os.path.join(d, "1_SpladePooling", "config.json"), "w") as f:
        json.dump(ST_POOLING if pooling is None else pooling, f)
    with open(os.path.join(d, "sentence_bert_config.json"), "w") as f:
        json.dump({"max_seq_length": 48, "do_lower_case": False} if sbert is None else sbert, f)


# ---- acceptance ---------------------------------------------------------------------------------------------------------------------
def test_plain_directory_loads_with_a_tied_decoder(ts, plain):
    assert ts.detect_layout(plain) == "hf"
    cfg, bert, head, tk, max_seq = ts.load_checkpoint(plain)
    assert (cfg.arch, cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.max_pos, cfg.num_labels) == ("bert", 600, 128, 2, 2, 66, 0)
    assert max_seq is None
    sd = load_file(os.path.join(plain, "model.safetensors"))
    assert HEAD + "decoder.weight" not in sd, "the fixture's decoder is tied"
    assert torch.equal(head["decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])
    assert torch.equal(head["bias"], sd[HEAD + "bias"])
    assert torch.equal(head["dense.weight"], sd[HEAD + "transform.dense.weight"])
    assert torch.equal(head["LayerNorm.bias"], sd[HEAD + "transform.LayerNorm.bias"])
    assert set(bert) == set(ts.bert_state_names(cfg)) and not any(k.startswith("bert.") for k in bert)
    assert tk.encode("w0 w1", 64) == [2, 5, 6, 3]


def test_unprefixed_body_and_ignored_tensors(ts, plain):
    def edit(sd):
        for k in [k for k in sd if k.startswith("bert.")]:
            sd[k[len("bert."):]] = sd.pop(k)
        sd["pooler.dense.weight"] = torch.zeros(128, 128)
        sd["pooler.dense.bias"] = torch.zeros(128)
        sd["cls.seq_relationship.weight"] = torch.zeros(2, 128)
        sd["cls.seq_relationship.bias"] = torch.zeros(2)
        sd["embeddings.position_ids"] = torch.arange(66)[None]

    want = ts.load_checkpoint(plain)
    _edit_state(plain, edit)
    got = ts.load_checkpoint(plain)
    assert all(torch.equal(got[1][k], want[1][k]) for k in want[1]) and all(torch.equal(got[2][k], want[2][k]) for k in want[2])

    def edit2(sd):
        sd["bert.pooler.dense.weight"] = sd.pop("pooler.dense.weight")

    _edit_state(plain, edit2)
    ts.load_checkpoint(plain)


def test_untied_decoder_weight_is_used_when_present(ts, plain):
    other = torch.randn(600, 128, generator=torch.Generator().manual_seed(1)).half()
    _edit_state(plain, lambda sd: sd.update({HEAD + "decoder.weight": other, HEAD + "decoder.bias": sd[HEAD + "bias"].clone()}))
    head = ts.load_checkpoint(plain)[2]
    assert torch.equal(head["decoder.weight"], other)


def test_sparse_encoder_directory_loads(ts, plain):
    want = ts.load_checkpoint(plain)
    _as_sparse_encoder(plain)
    assert ts.detect_layout(plain) == "sparse_encoder"
    cfg, bert, head, _, max_seq = ts.load_checkpoint(plain)
    assert cfg == want[0] and max_seq == 48
    assert all(torch.equal(head[k], want[2][k]) for k in head)
    _edit_json(os.path.join(plain, "1_SpladePooling", "config.json"), chunk_size=64)          # a memory option: tolerated
    with open(os.path.join(plain, "config_sentence_transformers.json"), "w") as f:
        json.dump({"__version__": {"sentence_transformers": "5.0.0"}, "model_type": "SparseEncoder", "prompts": {},
                   "default_prompt_name": None, "similarity_fn_name": "dot"}, f)
    ts.load_checkpoint(plain)


def test_vocabulary_is_padded_to_a_multiple_of_128(ts, plain):
    head = ts.load_checkpoint(plain)[2]
    E, b = ts.pad_vocabulary(head["decoder.weight"].to(torch.bfloat16), head["bias"])
    assert tuple(E.shape) == (640, 128) and tuple(b.shape) == (640,) and b.dtype == torch.float32
    assert torch.equal(E[:600], head["decoder.weight"].to(torch.bfloat16)) and torch.equal(b[:600], head["bias"].float())
    assert not E[600:].any() and not b[600:].any()
    E2, _ = ts.pad_vocabulary(torch.ones(640, 128), torch.ones(640))
    assert tuple(E2.shape) == (640, 128)


def test_dtype_names(ts):
    assert ts.resolve_dtype(None) == torch.bfloat16 and ts.resolve_dtype({"torch_dtype": "float16"}) == torch.float16
    assert ts.resolve_dtype({"torch_dtype": torch.bfloat16}) == torch.bfloat16 and ts.resolve_dtype({"precision": "fp16"}) == torch.float16
    for mk in ({"torch_dtype": "float32"}, {"precision": "f16x3"}, {"precision": "reference"}, {"torch_dtype": torch.float64}):
        with pytest.raises(NotImplementedError, match="bfloat16.*float16"):
            ts.resolve_dtype(mk)


def test_exports():
    import tensor_truth_amd as t

    assert t.HipSpladeRetriever.__name__ == "HipSpladeRetriever" and t.SpladeStore.__name__ == "SpladeStore"
    assert t.SpladeEncoder.__name__ == "SpladeEncoder"
    with pytest.raises(AttributeError):
        t.no_such_name


def test_no_cpu_path(ts):
    with pytest.raises(RuntimeError, match="HIP device"):
        ts.SpladeStore(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ts.HipSpladeRetriever(model=SRC, device="cpu")
    with pytest.raises(ValueError, match="similarity_top_k"):
        ts.HipSpladeRetriever(model=SRC, similarity_top_k=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.sparse_compact(torch.zeros(1, 8), 8, 4)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooling,match", [
    (dict(ST_POOLING, pooling_strategy="sum"), "pooling_strategy='sum'"),
    (dict(ST_POOLING, activation_function="log1p_relu"), "activation_function='log1p_relu'"),
    (dict(ST_POOLING, temperature=2.0), "temperature"),
    ({"activation_function": "relu"}, "pooling_strategy"),
    (dict(ST_POOLING, word_embedding_dimension=30522), "word_embedding_dimension=30522"),
])
def test_pooling_settings_refused(ts, plain, pooling, match):
    _as_sparse_encoder(plain, pooling=pooling)
    with pytest.raises((NotImplementedError, ValueError), match=match):
        ts.load_checkpoint(plain)


def test_other_module_lists_refused(ts, plain):
    router = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Router"}]
    _as_sparse_encoder(plain, modules=router)
    with pytest.raises(NotImplementedError, match="Router"):
        ts.load_checkpoint(plain)
    _as_sparse_encoder(plain, modules=ST_MODULES + [{"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}])
    with pytest.raises(NotImplementedError, match="Normalize"):
        ts.load_checkpoint(plain)
    _as_sparse_encoder(plain, sbert={"max_seq_length": 48, "model_args": {}})
    with pytest.raises(NotImplementedError, match="model_args"):
        ts.load_checkpoint(plain)


@pytest.mark.parametrize("fields,match", [
    (dict(vocab_size=65537), "vocab_size=65537"),
    (dict(model_type="distilbert"), "DistilBERT"),
    (dict(model_type="roberta"), "model_type='roberta'"),
    (dict(position_embedding_type="relative_key"), "relative_key"),
    (dict(hidden_act="relu"), "hidden_act='relu'"),
])
def test_config_refused(ts, plain, fields, match):
    _edit_json(os.path.join(plain, "config.json"), **fields)
    with pytest.raises(NotImplementedError, match=match):
        ts.load_checkpoint(plain)


def test_state_refused(ts, plain):
    keep = os.path.join(plain, "model.safetensors")
    shutil.copy(keep, keep + ".orig")

    def with_edit(fn):
        shutil.copy(keep + ".orig", keep)
        _edit_state(plain, fn)

    with_edit(lambda sd: sd.update({HEAD + "decoder.bias": sd[HEAD + "bias"] + 1}))
    with pytest.raises(NotImplementedError, match="decoder.bias differs"):
        ts.load_checkpoint(plain)
    with_edit(lambda sd: sd.update({"classifier.weight": torch.zeros(1, 128)}))
    with pytest.raises(NotImplementedError, match="classifier.weight"):
        ts.load_checkpoint(plain)
    with_edit(lambda sd: sd.update({HEAD + "transform.extra.weight": torch.zeros(1)}))
    with pytest.raises(NotImplementedError, match="transform.extra.weight"):
        ts.load_checkpoint(plain)
    with_edit(lambda sd: sd.pop(HEAD + "transform.LayerNorm.weight"))
    with pytest.raises(ValueError, match="transform.LayerNorm.weight"):
        ts.load_checkpoint(plain)
    with_edit(lambda sd: sd.pop("bert.encoder.layer.1.output.dense.bias"))
    with pytest.raises(ValueError, match="encoder.layer.1.output.dense.bias"):
        ts.load_checkpoint(plain)
    with_edit(lambda sd: sd.update({HEAD + "decoder.weight": torch.zeros(599, 128)}))
    with pytest.raises(ValueError, match="decoder.weight"):
        ts.load_checkpoint(plain)
    with_edit(lambda sd: None)
    with pytest.raises(NotImplementedError, match="bfloat16.*float16"):
        ts.load_checkpoint(plain, {"torch_dtype": "float32"})


def test_fixture_is_what_its_generator_describes():
    z = np.load(os.path.join(ROOT, "tests", "golden", "splade_l2_expected.npz"))
    lens = z["lens"]
    assert int(z["n_queries"]) == 4 and len(lens) == 28 and lens.min() == 3 and lens.max() == 64 == int(z["max_length"])
    assert z["weights"].shape == (28, 600) and z["lex"].shape == (4, 24) and z["pre"].shape == (28, 600)
    assert np.allclose(z["weights"], np.log1p(np.maximum(z["pre"], 0)), rtol=0, atol=1e-12)
    assert np.allclose(z["lex"], z["weights"][:4] @ z["weights"][4:].T, rtol=0, atol=1e-12)
    assert ((z["weights"] > 0).sum(1) >= 8).all()
    for t in ("bf16", "fp16"):
        band = (np.abs(z["pre"]) <= 2 * float(z[f"e_pre_{t}"])).mean(1)
        assert band.max() <= 0.05 and z[f"prune8_{t}"].any()
    for name in z["defects"]:
        d = np.load(os.path.join(ROOT, "tests", "golden", f"splade_l2_defect_{name}.npz"))
        for q in ("weights", "lex"):
            assert np.abs(d[q] - z[q]).max() > 4 * max(float(z[f"e_{q}_bf16"]), float(z[f"e_{q}_fp16"])), (name, q)
