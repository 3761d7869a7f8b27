"""CPU: the host side of the NomicBERT / Jina-embeddings-v3 path (tensor_truth_amd/ropebert.py, its dispatch in weights.py,
precision.py and embedding.py).

Config parsing from the fixture directories (tests/golden/make_ropebert_golden.py) and the installed config classes' defaults; each
refusal with its message; the two tensor layouts loading to identical arrays (the renamings of transformers/conversion_mapping.py);
unread tensors refused by name; pooling and prompt files; the reranker's loader; the refused reference precision; and the ctypes
mirrors of ``tt_ropebert_weights`` / ``tt_ropebert_layer_weights`` against the header (the way tests/test_struct_layouts.py checks
the encoder structs).  Before this path existed a ``nomic_bert`` or ``jina_embeddings_v3`` config.json was parsed as XLM-R -- an
unknown model_type -- and its weights died with ``KeyError: 'embeddings.position_embeddings.weight'``.
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
NOMIC, JINA, NOMIC_ORIG = (os.path.join(GOLDEN, n) for n in ("ropebert_nomic", "ropebert_jina", "ropebert_nomic_orig"))


def _config_json(d):
    with open(os.path.join(d, "config.json")) as f:
        return json.load(f)


def test_fixture_configs_parse():
    from tensor_truth_amd import ropebert, weights

    n = weights._config_from_hf(_config_json(NOMIC))
    assert isinstance(n, ropebert.RopeBertConfig)
    assert (n.arch, n.hidden, n.layers, n.heads, n.ffn, n.vocab_size, n.max_pos) == ("nomic_bert", 256, 2, 4, 512, 600, 2048)
    assert (n.type_vocab, n.pad_id, n.num_labels, n.ln_eps, n.rope_theta, n.mlp, n.biases) == (2, 0, 0, 1e-12, 1000.0, "swiglu", False)
    assert n.max_seq_len == 2048                       # RoPE: every position is usable, none reserved
    j = weights._config_from_hf(_config_json(JINA))
    assert (j.arch, j.hidden, j.layers, j.heads, j.ffn, j.vocab_size, j.max_pos) == ("jina_embeddings_v3", 256, 2, 4, 512, 600, 2048)
    assert (j.type_vocab, j.pad_id, j.num_labels, j.ln_eps, j.rope_theta, j.mlp, j.biases) == (1, 1, 0, 1e-5, 20000.0, "gelu", True)
    for cfg in (n, j):
        ropebert.check_config(cfg)
    # a want_head caller's default changes nothing: these types are embedders
    assert weights._config_from_hf(_config_json(NOMIC), 1).num_labels == 0
    assert _config_json(NOMIC_ORIG) == _config_json(NOMIC)


def test_defaults_are_the_installed_config_classes():
    from transformers import JinaEmbeddingsV3Config, NomicBertConfig

    from tensor_truth_amd import ropebert, weights

    for mt, cls, base in (("nomic_bert", NomicBertConfig, ropebert.NOMIC_BASE), ("jina_embeddings_v3", JinaEmbeddingsV3Config, ropebert.JINA_V3)):
        hf = cls()
        cfg = weights._config_from_hf({"model_type": mt})
        assert cfg == base
        assert (cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.type_vocab, cfg.ln_eps, cfg.pad_id) == (
            hf.vocab_size, hf.hidden_size, hf.num_hidden_layers, hf.num_attention_heads, hf.intermediate_size, hf.max_position_embeddings,
            hf.type_vocab_size, hf.layer_norm_eps, hf.pad_token_id)
        assert cfg.rope_theta == hf.rope_parameters["rope_theta"] == cls.default_theta and hf.rope_parameters["rope_type"] == "default"
        assert ropebert.DEFAULTS[mt]["hidden_act"] == hf.hidden_act
    # rope_parameters is read; a null value means the default
    d = dict(_config_json(NOMIC), rope_parameters={"rope_type": "default", "rope_theta": 5000.0})
    assert weights._config_from_hf(d).rope_theta == 5000.0
    assert weights._config_from_hf(dict(_config_json(JINA), rope_parameters=None, layer_norm_eps=None)).rope_theta == 20000.0


def test_positions_are_zero_based():
    """``position_ids = torch.arange(seq_length)`` in both modelling files: no offset, and no token types in an embedder call."""
    import inspect

    from transformers.models.jina_embeddings_v3 import modeling_jina_embeddings_v3 as mj
    from transformers.models.nomic_bert import modeling_nomic_bert as mn

    from tensor_truth_amd import weights
    from tensor_truth_amd.encoder import pack_tokens

    for mod, cls in ((mn, "NomicBertModel"), (mj, "JinaEmbeddingsV3Model")):
        assert "position_ids = torch.arange(seq_length, dtype=torch.long, device=device)[None, :]" in inspect.getsource(getattr(mod, cls).forward)
    for d in (NOMIC, JINA):
        cfg = weights._config_from_hf(_config_json(d))
        b = pack_tokens([[2, 5, 6, 3], [2, 7, 3]], cfg)
        assert b.pos[:4].tolist() == [0, 1, 2, 3] and b.pos[8:11].tolist() == [0, 1, 2] and b.types is None
        assert b.ids[4] == cfg.pad_id


def test_refusals_name_the_field():
    from tensor_truth_amd import ropebert, weights

    for d, act in ((NOMIC, "silu"), (JINA, "gelu")):
        base = _config_json(d)
        with pytest.raises(NotImplementedError, match="rope_type='dynamic'"):
            weights._config_from_hf(dict(base, rope_parameters={"rope_type": "dynamic", "rope_theta": 1000.0, "factor": 2.0}))
        with pytest.raises(NotImplementedError, match="rope_type='linear'"):
            weights._config_from_hf(dict(base, rope_scaling={"type": "linear", "factor": 2.0}))
        with pytest.raises(NotImplementedError, match="head_dim=32"):
            weights._config_from_hf(dict(base, head_dim=32))
        with pytest.raises(NotImplementedError, match="head_dim=32"):
            weights._config_from_hf(dict(base, num_attention_heads=8, head_dim=None))
        with pytest.raises(NotImplementedError, match="hidden_act='relu'"):
            weights._config_from_hf(dict(base, hidden_act="relu"))
        other = "gelu" if act == "silu" else "silu"
        with pytest.raises(NotImplementedError, match=f"hidden_act='{other}'"):
            weights._config_from_hf(dict(base, hidden_act=other))
        with pytest.raises(NotImplementedError, match="hidden_size=2048"):
            weights._config_from_hf(dict(base, hidden_size=2048, num_attention_heads=32))
        with pytest.raises(ValueError, match="ForSequenceClassification.*no such cross-encoder"):
            weights._config_from_hf(dict(base, architectures=["NomicBertForSequenceClassification"]))
    # the original remote-code config: refused, no mapping guessed
    with pytest.raises(ValueError, match=r"remote-code keys \['n_embd', 'n_layer', 'rotary_emb_base'\].*transformers-format config.json"):
        weights._config_from_hf({"model_type": "nomic_bert", "n_embd": 768, "n_layer": 12, "rotary_emb_base": 1000})
    cfg = weights._config_from_hf(_config_json(NOMIC))
    for kw, text in ((dict(hidden=320, heads=5), "hidden_size=320"), (dict(hidden=1152, heads=18), "hidden_size=1152"),
                     (dict(heads=8), "head_dim must be 64"), (dict(ffn=100), "intermediate_size=100"),
                     (dict(num_labels=1), "classification heads"), (dict(mlp="relu"), "intermediate_size|mlp=")):
        with pytest.raises(NotImplementedError, match=text):
            ropebert.check_config(dataclasses.replace(cfg, **kw))
    # the GELU MLP's up-projection is F columns wide: whole 128-column GEMM tiles
    with pytest.raises(NotImplementedError, match="intermediate_size=192"):
        ropebert.check_config(dataclasses.replace(weights._config_from_hf(_config_json(JINA)), ffn=192))
    ropebert.check_config(dataclasses.replace(cfg, ffn=192))


def test_both_layouts_load_to_identical_arrays():
    from tensor_truth_amd import ropebert, weights

    cfg = weights._config_from_hf(_config_json(NOMIC))
    a, b = weights.load_state(NOMIC), weights.load_state(NOMIC_ORIG)
    assert "layers.0.self_attn.q_proj.weight" in a and "encoder.layers.0.attn.Wqkv.weight" in b and "emb_ln.weight" in b
    assert {"encoder.layers.1.mlp.fc11.weight", "encoder.layers.1.mlp.fc12.weight", "encoder.layers.1.mlp.fc2.weight",
            "encoder.layers.1.norm1.bias", "encoder.layers.1.norm2.weight", "encoder.layers.1.attn.out_proj.weight"} <= set(b)
    assert not set(a) & set(b) - {"embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight"}
    sa, sb = ropebert.check_state(cfg, a), ropebert.check_state(cfg, b)
    names = ropebert.state_names(cfg)
    assert sorted(sa) == sorted(sb) == sorted(names) and len(names) == 4 + 2 * (7 + 4)
    assert all(torch.equal(sa[k], sb[k]) for k in names)
    # fc11 is up_proj and fc12 gate_proj (conversion_mapping.py), not the other way round
    assert torch.equal(sb["layers.0.mlp.up_proj.weight"], b["encoder.layers.0.mlp.fc11.weight"])
    assert torch.equal(sb["layers.0.mlp.gate_proj.weight"], b["encoder.layers.0.mlp.fc12.weight"])
    assert torch.equal(torch.cat([sb[f"layers.1.self_attn.{n}_proj.weight"] for n in "qkv"]), b["encoder.layers.1.attn.Wqkv.weight"])
    # prefixes of the *For... exports
    for pre in ("nomic_bert.", "bert.", "0.auto_model."):
        assert sorted(ropebert.check_state(cfg, {pre + k: v for k, v in b.items()})) == sorted(names)
    # Jina: the fixture's own names, and the original layout (mixer.Wqkv with its bias, mixer.out_proj; mlp.fc1 / fc2 keep their names)
    jcfg = weights._config_from_hf(_config_json(JINA))
    j = weights.load_state(JINA)
    sj = ropebert.check_state(jcfg, j)
    assert "pooler.dense.weight" in j and "layers.0.mlp.fc2.bias" in sj and len(ropebert.state_names(jcfg)) == 4 + 2 * (12 + 4)
    orig = {}
    for k, v in j.items():
        if "self_attn.k_proj" in k or "self_attn.v_proj" in k:
            continue
        if "self_attn.q_proj" in k:
            orig["roberta.encoder." + k.replace("self_attn.q_proj", "mixer.Wqkv")] = torch.cat([j[k.replace("q_proj", n + "_proj")] for n in "qkv"])
            continue
        for new, old in (("embeddings.LayerNorm", "emb_ln"), ("self_attn.o_proj", "mixer.out_proj"), ("post_attention_layernorm", "norm1"),
                         ("post_mlp_layernorm", "norm2")):
            k = k.replace(new, old)
        orig["roberta." + ("encoder." if k.startswith("layers.") else "") + k] = v
    assert "roberta.encoder.layers.0.mixer.Wqkv.bias" in orig and "roberta.encoder.layers.1.mlp.fc2.weight" in orig
    so = ropebert.check_state(jcfg, orig)
    assert sorted(so) == sorted(sj) and all(torch.equal(so[k], sj[k]) for k in sj)


def test_unread_tensors_are_refused_by_name():
    from tensor_truth_amd import ropebert, weights

    cfg = dataclasses.replace(weights._config_from_hf(_config_json(NOMIC)), vocab_size=32, layers=1)
    sd = ropebert.synthetic_state(cfg, seed=1)
    assert sorted(sd) == sorted(ropebert.state_names(cfg))
    H = cfg.hidden
    ok = dict(sd, **{"cls.predictions.bias": torch.zeros(32), "cls.predictions.transform.dense.weight": torch.zeros(H, H),
                     "pooler.dense.weight": torch.zeros(H, H), "pooler.dense.bias": torch.zeros(H), "lm_head.decoder.weight": torch.zeros(32, H),
                     "rotary_emb.inv_freq": torch.zeros(32), "layers.0.self_attn.rotary_emb.inv_freq": torch.zeros(32)})
    assert set(sd) <= set(ropebert.check_state(cfg, ok))
    with pytest.raises(NotImplementedError, match=r"layers\.0\.self_attn\.q_proj\.bias"):       # a bias under a NomicBERT config
        ropebert.check_state(cfg, dict(ok, **{"layers.0.self_attn.q_proj.bias": torch.zeros(H)}))
    with pytest.raises(NotImplementedError, match=r"classifier\.weight"):
        ropebert.check_state(cfg, dict(ok, **{"classifier.weight": torch.zeros(1, H)}))
    with pytest.raises(NotImplementedError, match=r"embeddings\.position_embeddings\.weight"):
        ropebert.check_state(cfg, dict(ok, **{"embeddings.position_embeddings.weight": torch.zeros(8, H)}))
    missing = dict(sd)
    del missing["layers.0.mlp.gate_proj.weight"]
    with pytest.raises(ValueError, match=r"missing \['layers\.0\.mlp\.gate_proj\.weight'\]"):
        ropebert.check_state(cfg, missing)
    # the LoRA tensors of an unmerged Jina checkpoint
    jcfg = dataclasses.replace(weights._config_from_hf(_config_json(JINA)), vocab_size=32, layers=1)
    jsd = ropebert.synthetic_state(jcfg, seed=2)
    assert sorted(jsd) == sorted(ropebert.state_names(jcfg))
    lora = "roberta.encoder.layers.0.mixer.Wqkv.parametrizations.weight.0.lora_A"
    with pytest.raises(NotImplementedError, match=r"mixer\.Wqkv\.parametrizations\.weight\.0\.lora_A"):
        ropebert.check_state(jcfg, dict(jsd, **{lora: torch.zeros(5, 4, H)}))
    with pytest.raises(NotImplementedError, match=r"layers\.0\.mlp\.fc1\.parametrizations\.weight\.0\.lora_B"):
        ropebert.check_state(jcfg, dict(jsd, **{"layers.0.mlp.fc1.parametrizations.weight.0.lora_B": torch.zeros(5, H, 4)}))


def test_pooling_and_prompt_files(tmp_path):
    from tensor_truth_amd import weights

    for d in (NOMIC, JINA, NOMIC_ORIG):
        assert weights.pooling_mode(d, "mean") == "mean_tokens" and weights.prompts(d) == {}        # no prompt file: nothing prepended
    assert weights.pooling_mode(str(tmp_path), "mean") == "mean"                                      # no 1_Pooling: the default
    os.makedirs(tmp_path / "1_Pooling")
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_cls_token": True, "pooling_mode_mean_tokens": False}))
    assert weights.pooling_mode(str(tmp_path), "mean") == "cls"
    (tmp_path / "config_sentence_transformers.json").write_text(json.dumps(
        {"prompts": {"query": "search_query: ", "document": "search_document: ", "classification": "classification: "}}))
    assert weights.prompts(str(tmp_path))["query"] == "search_query: " and weights.prompts(str(tmp_path))["document"] == "search_document: "


def test_the_reranker_surface_refuses_these_types():
    """``HipSentenceTransformerRerank`` loads through ``weights.resolve(want_head=True)``: a clear ValueError, before the weights
    are read."""
    from tensor_truth_amd import weights

    for d, mt in ((NOMIC, "nomic_bert"), (JINA, "jina_embeddings_v3"), (NOMIC_ORIG, "nomic_bert")):
        with pytest.raises(ValueError, match=f"{mt} checkpoints are served as embedders only.*no such cross-encoder"):
            weights.resolve(d, None, torch.device("cpu"), want_head=True)
        cfg, state, mdir = weights.resolve(d, None, torch.device("cpu"), want_head=False)
        assert cfg.arch == mt and mdir == d and state


@pytest.mark.default_precision
def test_reference_precision_is_refused():
    """No torch_dtype (the reference's own call) and float32 resolve to the reference precision, which these encoders do not have:
    refused before anything touches a device, naming the two types that exist."""
    from tensor_truth_amd import precision, weights

    for d in (NOMIC, JINA):
        cfg = weights._config_from_hf(_config_json(d))
        for mk in (None, {"torch_dtype": "float32"}, {"torch_dtype": torch.float32}, {"precision": "fp8"}):
            with pytest.raises(NotImplementedError, match="NomicBERT / Jina-v3.*bfloat16.*float16"):
                precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "embedder fixture")
        for mk in ({"torch_dtype": "bfloat16"}, {"torch_dtype": "float16"}):
            with pytest.raises(RuntimeError, match="HIP device"):
                precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "embedder fixture")


def test_synthetic_weights_resolve():
    from tensor_truth_amd import ropebert, weights

    tiny = dataclasses.replace(ropebert.JINA_V3, vocab_size=50, layers=1)
    cfg, state, mdir = weights.resolve("some/jina", {"synthetic_seed": 3, "encoder_config": tiny}, torch.device("cpu"), want_head=False)
    assert cfg is tiny and mdir is None and sorted(state) == sorted(ropebert.state_names(tiny))
    assert state["layers.0.mlp.fc1.weight"].shape == (4096, 1024) and state["layers.0.self_attn.q_proj.bias"].shape == (1024,)


def test_ctypes_mirrors_match_tt_hip_h(tmp_path):
    from test_struct_layouts import INCLUDE, _c_fields, _c_layouts

    from tensor_truth_amd.ropebert import _RbLayerW, _RbW

    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.fail("no host C compiler")
    header = open(os.path.join(INCLUDE, "tt_hip.h")).read()
    mirrors = {"tt_ropebert_weights": _RbW, "tt_ropebert_layer_weights": _RbLayerW}
    assert dict(_RbW._fields_)["layer"]._type_ is _RbLayerW
    fields = {s: _c_fields(header, s) for s in mirrors}
    assert fields["tt_ropebert_weights"][:7] == ["hidden", "layers", "heads", "ffn", "vocab", "type_vocab", "mlp_kind"]
    layouts = _c_layouts(tmp_path, cc, fields)
    for s, S in mirrors.items():
        size, layout = layouts[s]
        assert fields[s] == [f for f, _ in S._fields_], s
        assert (ctypes.sizeof(S), [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_]) == (size, layout), s


def test_library_binds_the_new_entry_points(built_lib):
    from tensor_truth_amd import _lib
    from tensor_truth_amd.encoder import ROPEBERT_BF16_PATH, ROPEBERT_FP16_PATH

    lib = _lib.load_library()
    for p in (ROPEBERT_BF16_PATH, ROPEBERT_FP16_PATH):
        assert p.cls_forward is None and p.head is None and p.no_fp8 and p.pool_last is None and p.pooled_head is None
        for name in (p.forward, p.workspace, p.pool, p.pool_mean):
            assert hasattr(lib, name)
