"""CPU: the host side of the JinaBERT path (tensor_truth_amd/jinabert.py, its dispatch in weights.py, precision.py and
embedding.py).

A JinaBERT ``config.json`` says ``"model_type": "bert"``; before this path existed ``weights._config_from_hf`` built a plain BERT
``EncoderConfig`` for it and the weights died on the missing position table.  Checked here: the dispatch on
``position_embedding_type: "alibi"`` (and that every other ``bert`` config still takes the BERT path); each refusal with its
message; the slopes against their literal values; the state mapping (Q | K | V concatenation, the ``bert.`` prefix, ``pooler.*`` /
``cls.*`` dropped, everything else refused by name); the refused reference precision; and the ctypes mirrors of
``tt_jinabert_weights`` / ``tt_jinabert_layer_weights`` against the header (the way tests/test_struct_layouts.py checks the encoder
structs).
"""
import ctypes
import dataclasses
import json
import os
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "jinabert_l2")


def _config_json(d=FIXTURE):
    with open(os.path.join(d, "config.json")) as f:
        return json.load(f)


def test_a_jinabert_config_becomes_arch_jina_bert():
    from tensor_truth_amd import jinabert, weights

    d = _config_json()
    assert d["model_type"] == "bert" and d["position_embedding_type"] == "alibi" and d["feed_forward_type"] == "geglu" and "auto_map" in d
    cfg = weights._config_from_hf(d)
    assert isinstance(cfg, jinabert.JinaBertConfig) and cfg.arch == "jina_bert"
    assert (cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.vocab_size, cfg.max_pos) == (384, 2, 6, 512, 600, 8192)
    assert (cfg.type_vocab, cfg.pad_id, cfg.num_labels, cfg.ln_eps) == (2, 0, 0, 1e-12)
    assert cfg.max_seq_len == 8192                     # max_position_embeddings: no position is reserved, there is no table
    jinabert.check_config(cfg)
    # a want_head caller's default changes nothing: these checkpoints are embedders
    assert weights._config_from_hf(d, 1).num_labels == 0
    # the published geometries
    for base, (h, l, nh, f) in ((jinabert.JINA_V2_SMALL, (512, 4, 8, 2048)), (jinabert.JINA_V2_BASE, (768, 12, 12, 3072))):
        jinabert.check_config(base)
        assert (base.arch, base.hidden, base.layers, base.heads, base.ffn, base.max_seq_len) == ("jina_bert", h, l, nh, f, 8192)
        assert base.hidden == 64 * base.heads and base.vocab_size == 30528 and base.type_vocab == 2


def test_a_plain_bert_config_still_becomes_bert():
    from tensor_truth_amd import weights
    from tensor_truth_amd.encoder import EncoderConfig

    plain = dict(model_type="bert", vocab_size=30522, hidden_size=384, num_hidden_layers=12, num_attention_heads=12,
                 intermediate_size=1536, max_position_embeddings=512, type_vocab_size=2, pad_token_id=0, layer_norm_eps=1e-12)
    for extra in ({}, {"position_embedding_type": "absolute"}, {"position_embedding_type": None}):
        cfg = weights._config_from_hf(dict(plain, **extra))
        assert type(cfg) is EncoderConfig and cfg.arch == "bert" and cfg.max_pos == 512
    head = weights._config_from_hf(dict(plain, architectures=["BertForSequenceClassification"]))
    assert head.arch == "bert" and head.num_labels == 1


def test_refusals_name_the_field():
    from tensor_truth_amd import jinabert, weights

    base = _config_json()
    with pytest.raises(NotImplementedError, match="feed_forward_type='original'"):
        weights._config_from_hf(dict(base, feed_forward_type="original"))
    with pytest.raises(NotImplementedError, match="feed_forward_type='reglu'"):
        weights._config_from_hf(dict(base, feed_forward_type="reglu"))
    missing = dict(base)
    del missing["feed_forward_type"]
    with pytest.raises(NotImplementedError, match="feed_forward_type='original'"):
        weights._config_from_hf(missing)
    with pytest.raises(NotImplementedError, match="hidden_act='relu'"):
        weights._config_from_hf(dict(base, hidden_act="relu"))
    with pytest.raises(NotImplementedError, match="hidden_act='gelu_new'"):
        weights._config_from_hf(dict(base, hidden_act="gelu_new"))
    with pytest.raises(NotImplementedError, match="head_dim=32"):           # jina-reranker-v1's head width
        weights._config_from_hf(dict(base, num_attention_heads=12))
    with pytest.raises(NotImplementedError, match="hidden_size=2048"):
        weights._config_from_hf(dict(base, hidden_size=2048, num_attention_heads=32))
    for arch in ("JinaBertForSequenceClassification", "BertForSequenceClassification"):
        with pytest.raises(ValueError, match="jina_bert checkpoints are served as embedders only"):
            weights._config_from_hf(dict(base, architectures=[arch]))
    cfg = weights._config_from_hf(base)
    for kw, text in ((dict(hidden=320, heads=5), "hidden_size=320"), (dict(hidden=1152, heads=18), "hidden_size=1152"),
                     (dict(heads=12), "head_dim must be 64"), (dict(ffn=192), "intermediate_size=192"),
                     (dict(num_labels=1), "classification heads")):
        with pytest.raises(NotImplementedError, match=text):
            jinabert.check_config(dataclasses.replace(cfg, **kw))


def test_alibi_slopes_literal_values():
    from tensor_truth_amd.jinabert import alibi_slopes

    assert alibi_slopes(8) == [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625]
    r = 2.0 ** -0.5
    want12 = [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125, 0.00390625, r, r / 2, r / 4, r / 8]
    got12 = alibi_slopes(12)
    assert len(got12) == 12 and got12[:8] == want12[:8] and all(abs(a - b) <= 1e-15 * b for a, b in zip(got12, want12))
    assert [round(x, 6) for x in got12[8:]] == [0.707107, 0.353553, 0.176777, 0.088388]
    # 6 heads (the fixture): the series of 4, then every other term of the series of 8
    assert alibi_slopes(6) == [0.25, 0.0625, 0.015625, 0.00390625, 0.5, 0.125]
    assert alibi_slopes(1) == [2.0 ** -8] and alibi_slopes(4) == [0.25, 0.0625, 0.015625, 0.00390625]
    with pytest.raises(ValueError):
        alibi_slopes(0)


def test_state_mapping_and_strict_loading():
    from tensor_truth_amd import jinabert, weights

    cfg = weights._config_from_hf(_config_json())
    raw = weights.load_state(FIXTURE)
    assert "pooler.dense.weight" in raw and "encoder.layer.1.mlp.gated_layers.weight" in raw
    assert "embeddings.position_embeddings.weight" not in raw and "encoder.layer.0.mlp.gated_layers.bias" not in raw
    names = jinabert.state_names(cfg)
    assert len(names) == 4 + 2 * 15
    sd = jinabert.check_state(cfg, raw)
    assert sorted(sd) == sorted(names) and all(torch.equal(sd[k], raw[k]) for k in names)       # pooler.* dropped, nothing renamed
    assert sd["encoder.layer.0.mlp.gated_layers.weight"].shape == (1024, 384) and sd["encoder.layer.0.mlp.wo.weight"].shape == (384, 512)
    # one optional bert. prefix; cls.* plays no part either
    pre = {"bert." + k: v for k, v in raw.items()}
    pre["cls.predictions.bias"] = torch.zeros(600)
    sp = jinabert.check_state(cfg, pre)
    assert sorted(sp) == sorted(names) and all(torch.equal(sp[k], sd[k]) for k in names)
    with pytest.raises(ValueError, match=r"missing \['embeddings\.word_embeddings\.weight'"):
        jinabert.check_state(cfg, {"bert.bert." + k: v for k, v in raw.items()})               # only ONE prefix is stripped
    # unknown tensors are refused by name: the qk-post-norm variant, a position table, a gate bias, a classifier
    H = cfg.hidden
    for name, shape in (("encoder.layer.0.attention.self.layer_norm_q.weight", (H,)), ("encoder.layer.1.attention.self.layer_norm_k.bias", (H,)),
                        ("embeddings.position_embeddings.weight", (512, H)), ("encoder.layer.0.mlp.gated_layers.bias", (1024,)),
                        ("classifier.weight", (1, H)), ("embeddings.position_ids", (1, 512))):
        with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
            jinabert.check_state(cfg, dict(raw, **{name: torch.zeros(shape)}))
    short = dict(raw)
    del short["encoder.layer.1.mlp.wo.bias"]
    with pytest.raises(ValueError, match=r"missing \['encoder\.layer\.1\.mlp\.wo\.bias'\]"):
        jinabert.check_state(cfg, short)
    # synthetic weights carry exactly the names the forward reads
    tiny = dataclasses.replace(cfg, vocab_size=32, layers=1)
    syn = jinabert.synthetic_state(tiny, seed=1)
    assert sorted(syn) == sorted(jinabert.state_names(tiny)) and syn["encoder.layer.0.mlp.gated_layers.weight"].shape == (1024, 384)
    cfg2, state, mdir = weights.resolve("some/jina-v2", {"synthetic_seed": 3, "encoder_config": tiny}, torch.device("cpu"), want_head=False)
    assert cfg2 is tiny and mdir is None and sorted(state) == sorted(syn)


def test_resolve_pooling_tokenizer_and_the_reranker_loader():
    from tensor_truth_amd import weights
    from tensor_truth_amd.tokenization import HFTokenizer, load_tokenizer

    cfg, state, mdir = weights.resolve(FIXTURE, None, torch.device("cpu"), want_head=False)
    assert cfg.arch == "jina_bert" and mdir == FIXTURE and state
    assert weights.pooling_mode(FIXTURE, "mean") == "mean_tokens" and weights.prompts(FIXTURE) == {}
    with pytest.raises(ValueError, match="jina_bert checkpoints are served as embedders only"):
        weights.resolve(FIXTURE, None, torch.device("cpu"), want_head=True)
    tk = load_tokenizer(FIXTURE, cfg.arch, cfg.vocab_size)
    assert isinstance(tk, HFTokenizer) and tk.encode("w0 w5 w595") == [2, 4, 9, 599, 3]
    assert (tk.sp.bos, tk.sp.eos, tk.sp.pad) == (101, 102, 0)          # the bert-base-uncased ids of the published checkpoints


@pytest.mark.default_precision
def test_reference_precision_is_refused():
    """No torch_dtype (the reference's own call) and float32 resolve to the reference precision, which these encoders do not have:
    refused before anything touches a device, naming the two types that exist."""
    from tensor_truth_amd import precision, weights

    cfg = weights._config_from_hf(_config_json())
    for mk in (None, {"torch_dtype": "float32"}, {"torch_dtype": torch.float32}, {"precision": "fp8"}):
        with pytest.raises(NotImplementedError, match="JinaBERT.*bfloat16.*float16"):
            precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "embedder fixture")
    for mk in ({"torch_dtype": "bfloat16"}, {"torch_dtype": "float16"}):
        with pytest.raises(RuntimeError, match="HIP device"):
            precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "embedder fixture")


def test_ctypes_mirrors_match_tt_hip_h(tmp_path):
    from test_struct_layouts import INCLUDE, _c_fields, _c_layouts

    from tensor_truth_amd.jinabert import _JbLayerW, _JbW

    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.fail("no host C compiler")
    header = open(os.path.join(INCLUDE, "tt_hip.h")).read()
    mirrors = {"tt_jinabert_weights": _JbW, "tt_jinabert_layer_weights": _JbLayerW}
    assert dict(_JbW._fields_)["layer"]._type_ is _JbLayerW
    fields = {s: _c_fields(header, s) for s in mirrors}
    assert fields["tt_jinabert_weights"][:7] == ["hidden", "layers", "heads", "ffn", "vocab", "type_vocab", "ln_eps"]
    assert fields["tt_jinabert_layer_weights"] == ["qkv_w", "qkv_b", "o_w", "o_b", "ln1_g", "ln1_b", "gate_w", "down_w", "down_b",
                                                   "ln2_g", "ln2_b"]
    layouts = _c_layouts(tmp_path, cc, fields)
    for s, S in mirrors.items():
        size, layout = layouts[s]
        assert fields[s] == [f for f, _ in S._fields_], s
        assert (ctypes.sizeof(S), [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_]) == (size, layout), s


def test_library_binds_the_new_entry_points(built_lib):
    from tensor_truth_amd import _lib
    from tensor_truth_amd.encoder import JINABERT_BF16_PATH, JINABERT_FP16_PATH

    lib = _lib.load_library()
    for p in (JINABERT_BF16_PATH, JINABERT_FP16_PATH):
        assert p.cls_forward is None and p.head is None and p.no_fp8 and p.pool_last is None and p.pooled_head is None
        for name in (p.forward, p.workspace, p.pool, p.pool_mean):
            assert hasattr(lib, name)
    for name in ("tt_jinabert_forward", "tt_jinabert_workspace_bytes", "tt_attention_alibi"):
        assert name in _lib.SIGNATURES and name + "_f16" in _lib.SIGNATURES and hasattr(lib, name) and hasattr(lib, name + "_f16")
