"""CPU: the host side of the ModernBERT path -- config.json parsing (both fixtures, an older-style export), every refusal by field
name, the checkpoint's tensor names, the precision refusal, the pair template and truncation of the fixture tokenizer."""
import dataclasses
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = {"modernbert_cls_l4": ("cls", 4, ("full_attention", "sliding_attention", "sliding_attention", "full_attention")),
            "modernbert_mean_l5": ("mean", 5, ("full_attention", "sliding_attention") * 2 + ("full_attention",))}


def _raw(name):
    with open(os.path.join(GOLDEN, name, "config.json")) as f:
        return json.load(f)


def _cfg(d):
    from tensor_truth_amd import weights

    return weights._config_from_hf(d, 1)


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_config_is_parsed(name):
    from tensor_truth_amd.modernbert import ModernBertConfig, check_config

    pooling, layers, types = FIXTURES[name]
    cfg = _cfg(_raw(name))
    assert isinstance(cfg, ModernBertConfig) and cfg.arch == "modernbert"
    assert (cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos) == (384, 256, layers, 4, 192, 1024)
    assert cfg.layer_types == types and cfg.local_attention == 32 and cfg.classifier_pooling == pooling
    assert (cfg.global_rope_theta, cfg.local_rope_theta) == (160000.0, 10000.0)
    assert cfg.ln_eps == 1e-5 and cfg.num_labels == 1 and cfg.type_vocab == 1 and cfg.pad_id == 0
    assert cfg.max_seq_len == 1024            # positions are 0-based: no XLM-R offset
    check_config(cfg)


def test_an_embedder_export_has_no_head():
    d = _raw("modernbert_cls_l4")
    d["architectures"] = ["ModernBertModel"]
    assert _cfg(d).num_labels == 0            # (want_head's default of the XLM-R branch does not apply: architectures decides)
    d["architectures"] = ["ModernBertForMaskedLM"]
    assert _cfg(d).num_labels == 0


def test_older_export_without_layer_types_and_rope_parameters():
    d = _raw("modernbert_mean_l5")
    for k in ("layer_types", "rope_parameters"):
        del d[k]
    d.update(global_attn_every_n_layers=3, global_rope_theta=160000.0, local_rope_theta=10000.0, num_hidden_layers=7)
    cfg = _cfg(d)
    assert cfg.layer_types == ("full_attention", "sliding_attention", "sliding_attention") * 2 + ("full_attention",)
    assert (cfg.global_rope_theta, cfg.local_rope_theta) == (160000.0, 10000.0)
    d["global_rope_theta"], d["local_rope_theta"] = 5e5, 2e4
    assert (_cfg(d).global_rope_theta, _cfg(d).local_rope_theta) == (5e5, 2e4)
    # the list is read, not derived, where it is there
    d["layer_types"] = ["sliding_attention"] * 6 + ["full_attention"]
    assert _cfg(d).layer_types == ("sliding_attention",) * 6 + ("full_attention",)


@pytest.mark.parametrize("field,value", [("attention_bias", True), ("mlp_bias", True), ("norm_bias", True), ("classifier_bias", True),
                                         ("hidden_activation", "silu"), ("classifier_activation", "tanh")])
def test_variants_are_refused_by_field_name(field, value):
    d = _raw("modernbert_cls_l4")
    d[field] = value
    with pytest.raises(NotImplementedError, match=field):
        _cfg(d)


def test_rope_types_and_label_counts_are_refused():
    d = _raw("modernbert_cls_l4")
    d["rope_parameters"]["full_attention"] = {"rope_type": "yarn", "rope_theta": 160000.0, "factor": 4.0}
    with pytest.raises(NotImplementedError, match="rope_type"):
        _cfg(d)
    d = _raw("modernbert_cls_l4")
    d["id2label"] = {"0": "a", "1": "b", "2": "c"}
    d.pop("num_labels", None)
    with pytest.raises(NotImplementedError, match="num_labels=3"):
        _cfg(d)


def test_shapes_and_pooling_outside_the_kernels_are_refused():
    from tensor_truth_amd.modernbert import MODERNBERT_BASE, MODERNBERT_LARGE, check_config

    for cfg in (MODERNBERT_BASE, MODERNBERT_LARGE):
        check_config(cfg)
        assert cfg.hidden == 64 * cfg.heads and cfg.layer_types[:4] == ("full_attention", "sliding_attention", "sliding_attention",
                                                                          "full_attention")
    base = _cfg(_raw("modernbert_cls_l4"))
    rep = lambda **kw: dataclasses.replace(base, **kw)  # noqa: E731
    for kw, text in ((dict(hidden=320, heads=5), "hidden_size=320"), (dict(hidden=1152, heads=18), "hidden_size=1152"),
                     (dict(heads=8), "head_dim must be 64"), (dict(ffn=200), "intermediate_size=200"),
                     (dict(classifier_pooling="max"), "classifier_pooling")):
        with pytest.raises(NotImplementedError, match=text):
            check_config(rep(**kw))
    with pytest.raises(ValueError, match="layer_types"):
        check_config(rep(layer_types=("full_attention",)))


@pytest.mark.parametrize("name", list(FIXTURES))
def test_state_names_are_the_checkpoints_tensors(name):
    from tensor_truth_amd import weights
    from tensor_truth_amd.encoder import _strip_prefix
    from tensor_truth_amd.modernbert import state_names, synthetic_state

    cfg = _cfg(_raw(name))
    sd = _strip_prefix(weights.load_state(os.path.join(GOLDEN, name)))
    assert sorted(sd) == sorted(state_names(cfg))
    assert "layers.0.attn_norm.weight" not in sd and "layers.1.attn_norm.weight" in sd
    synth = synthetic_state(cfg, 3)
    assert sorted(synth) == sorted(sd) and all(tuple(synth[k].shape) == tuple(sd[k].shape) for k in sd)
    emb = dataclasses.replace(cfg, num_labels=0)
    assert sorted(state_names(emb)) == sorted(k for k in sd if not k.startswith(("head.", "classifier.")))


def test_tensors_the_forward_would_not_read_are_refused():
    from tensor_truth_amd.modernbert import check_state, synthetic_state

    cfg = _cfg(_raw("modernbert_cls_l4"))
    sd = {"model." + k if not k.startswith(("head.", "classifier.")) else k: v for k, v in synthetic_state(cfg, 1).items()}
    assert "layers.3.mlp.Wo.weight" in check_state(cfg, sd)
    for extra in ("model.layers.1.attn.Wqkv.bias", "model.layers.0.attn_norm.weight", "model.final_norm.bias", "head.dense.bias"):
        with pytest.raises(NotImplementedError, match=re.escape(extra.replace("model.", ""))):
            check_state(cfg, dict(sd, **{extra: torch.zeros(1)}))
    # a masked-LM export's decoder is ignored, as lm_head.weight is for Qwen3; an embedder's config ignores the head
    check_state(cfg, dict(sd, **{"decoder.weight": torch.zeros(1), "decoder.bias": torch.zeros(1)}))
    check_state(dataclasses.replace(cfg, num_labels=0), sd)
    short = dict(sd)
    del short["model.layers.2.mlp_norm.weight"]
    with pytest.raises(ValueError, match=re.escape("missing ['layers.2.mlp_norm.weight']")):
        check_state(cfg, short)
    with pytest.raises(ValueError, match="classifier.bias"):
        check_state(cfg, {k: v for k, v in sd.items() if k != "classifier.bias"})


def test_weights_refuse_a_cpu_device_and_fp32():
    from tensor_truth_amd.modernbert import ModernBertWeights, synthetic_state

    cfg = _cfg(_raw("modernbert_cls_l4"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ModernBertWeights(cfg, synthetic_state(cfg, 1), torch.device("cpu"))
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        ModernBertWeights(cfg, synthetic_state(cfg, 1), torch.device("cuda"), dtype=torch.float32)


def test_reference_precision_is_refused(monkeypatch):
    from tensor_truth_amd import precision
    from tensor_truth_amd.modernbert import synthetic_state

    monkeypatch.delenv("TT_PRECISION", raising=False)
    cfg = _cfg(_raw("modernbert_cls_l4"))
    for mk in (None, {"torch_dtype": "float32"}, {"precision": "fp8"}):
        with pytest.raises(NotImplementedError, match="ModernBERT.*bfloat16.*float16"):
            precision.build_encoder(cfg, synthetic_state(cfg, 1), torch.device("cuda"), mk, "reranker fixture")


@pytest.mark.parametrize("name", list(FIXTURES))
def test_pair_template_and_truncation(name):
    from tensor_truth_amd.tokenization import HFTokenizer, load_tokenizer

    tk = load_tokenizer(os.path.join(GOLDEN, name), "modernbert", 384)
    assert isinstance(tk, HFTokenizer)
    z = np.load(os.path.join(GOLDEN, f"{name}_expected.npz"))
    q, p = z["pair_query"].tolist()[0], z["pair_passage"].tolist()[0]
    ids, types = tk.encode_pair_batch([(q, p)], 512)[0]
    assert types is None                                   # no token type ids
    nq, npass = len(q.split()), len(p.split())
    assert ids[0] == 1 and ids[1 + nq] == 2 and ids[-1] == 2 and len(ids) == nq + npass + 3      # [CLS] q [SEP] p [SEP]
    assert ids[1:1 + nq] == [4 + int(w[1:]) for w in q.split()]
    assert tk.encode(q, None) == [1] + [4 + int(w[1:]) for w in q.split()] + [2]
    # longest-first truncation keeps the specials
    q, p = z["pair_query"].tolist()[5], z["pair_passage"].tolist()[5]          # 40 + 150 words
    ids, _ = tk.encode_pair_batch([(q, p)], 64)[0]
    assert len(ids) == 64 and ids[0] == 1 and ids[-1] == 2 and ids.count(2) == 2
    cfg = _cfg(_raw(name))
    assert min(512, cfg.max_seq_len) == 512 and min(4096, cfg.max_seq_len) == 1024      # what the reranker truncates to
