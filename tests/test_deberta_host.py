"""CPU: the host side of the DeBERTa-v2 / v3 path (tensor_truth_amd/deberta.py, weights._deberta_config_from_hf,
precision._build_deberta, tokenization.SpecialTokens("deberta-v2")).

Config parsing from the fixture directory (tests/golden/make_deberta_golden.py) and each refusal by field name; the extra-tensor
rule; the host-built distance table against the fixture's stored one and against a fresh call of transformers' own function; the
tensor list; the pair layout; the refused reference precision; the published geometry; the ctypes mirror of ``tt_deberta_weights``
against the header.  Before the DeBERTa path existed the fixture's config was parsed as XLM-R and its weights died with a KeyError.
"""
import ctypes
import dataclasses
import json
import os
import shutil

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "deberta_v3_ce")


def _config_json():
    with open(os.path.join(FIXTURE, "config.json")) as f:
        return json.load(f)


def _expected():
    return np.load(os.path.join(GOLDEN, "deberta_v3_ce_expected.npz"))


def test_fixture_config_parses_as_deberta():
    from tensor_truth_amd import deberta, weights

    cfg = weights._config_from_hf(_config_json(), 1)
    assert cfg.arch == "deberta-v2" and isinstance(cfg, deberta.DebertaConfig)
    assert (cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.vocab_size, cfg.max_pos) == (256, 2, 4, 512, 600, 512)
    assert (cfg.pad_id, cfg.type_vocab, cfg.num_labels, cfg.ln_eps) == (0, 1, 1, 1e-7)
    assert (cfg.position_buckets, cfg.max_relative_positions, cfg.max_seq_len) == (256, 512, 512)      # -1 resolves to the positions
    deberta.check_config(cfg)
    # the head comes from ``architectures``, not from who asks
    assert weights._config_from_hf(_config_json(), 0).num_labels == 1
    assert weights._config_from_hf(dict(_config_json(), architectures=["DebertaV2Model"]), 1).num_labels == 0
    # both spellings of pos_att_type, in either order
    for pat in (["c2p", "p2c"], ["p2c", "c2p"], "p2c|c2p", "c2p|p2c"):
        assert weights._config_from_hf(dict(_config_json(), pos_att_type=pat)).arch == "deberta-v2"
    assert weights._config_from_hf(dict(_config_json(), max_relative_positions=512)).max_relative_positions == 512


def test_other_model_types_parse_as_before():
    from tensor_truth_amd import weights

    d = dict(vocab_size=100, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
             max_position_embeddings=66)
    assert weights._config_from_hf(dict(d, model_type="xlm-roberta")).arch == "xlmr"
    assert weights._config_from_hf(dict(d, model_type="bert")).arch == "bert"
    assert weights._config_from_hf(dict(d, model_type="something-else")).arch == "xlmr"
    assert weights._config_from_hf(dict(d, model_type="mpnet")).arch == "mpnet"


@pytest.mark.parametrize("change, text", [
    (dict(relative_attention=False), "relative_attention=False"),
    (dict(pos_att_type=["c2p"]), "pos_att_type="), (dict(pos_att_type="p2c"), "pos_att_type="),
    (dict(pos_att_type=["c2p", "p2c", "p2p"]), "pos_att_type="), (dict(pos_att_type=None), "pos_att_type="),
    (dict(share_att_key=False), "share_att_key=False"),
    (dict(norm_rel_ebd="none"), "norm_rel_ebd='none'"),
    (dict(position_biased_input=True), "position_biased_input=True"),
    (dict(type_vocab_size=2), "type_vocab_size=2"),
    (dict(conv_kernel_size=3), "conv_kernel_size=3"),
    (dict(embedding_size=128), "embedding_size=128"),
    (dict(pooler_hidden_size=128), "pooler_hidden_size=128"),
    (dict(pooler_hidden_act="tanh"), "pooler_hidden_act='tanh'"),
    (dict(hidden_act="relu"), "hidden_act='relu'"),
    (dict(position_buckets=-1), "position_buckets=-1"), (dict(position_buckets=0), "position_buckets=0"),
    (dict(max_relative_positions=1024), "max_relative_positions=1024"),
    (dict(id2label={"0": "a", "1": "b"}), "num_labels=2"),
    (dict(hidden_size=320, num_attention_heads=5, pooler_hidden_size=320), "hidden_size=320"),
    (dict(hidden_size=1152, num_attention_heads=18, pooler_hidden_size=1152), "hidden_size=1152"),
    (dict(num_attention_heads=8), "head_dim must be 64"),
])
def test_refusals_name_the_field(change, text):
    from tensor_truth_amd import weights

    with pytest.raises(NotImplementedError, match=text):
        weights._config_from_hf(dict(_config_json(), **change))


def test_shape_refusals_of_the_weights_class():
    from tensor_truth_amd import deberta, weights

    cfg = weights._config_from_hf(_config_json())
    for kw, text in ((dict(hidden=320, heads=5), "hidden_size=320"), (dict(heads=8), "head_dim must be 64"),
                     (dict(ffn=200), "intermediate_size=200"), (dict(position_buckets=255), "position_buckets=255"),
                     (dict(max_pos=1024), "max_position_embeddings=1024"), (dict(num_labels=2), "num_labels=2"),
                     (dict(num_labels=0), "out of scope")):        # a DebertaV2Model without a head: an embedder
        with pytest.raises(NotImplementedError, match=text):
            deberta.check_config(dataclasses.replace(cfg, **kw))


def test_state_names_match_the_fixture_and_the_extra_tensor_rule():
    from tensor_truth_amd import deberta, weights

    cfg = weights._config_from_hf(_config_json())
    with open(os.path.join(FIXTURE, "model.safetensors.index.json")) as f:
        stored = sorted(json.load(f)["weight_map"])
    assert all(n.startswith("deberta.") or n.split(".")[0] in ("pooler", "classifier") for n in stored)
    stripped = sorted(n[len("deberta."):] if n.startswith("deberta.") else n for n in stored)
    assert sorted(deberta.state_names(cfg)) == stripped and len(stripped) == 6 + 2 * 16 + 4
    state = weights.load_state(FIXTURE)
    sd = deberta.check_state(cfg, state)          # the fixture is a DeBERTa of its own config: nothing missing, nothing refused
    assert sorted(sd) == stripped
    small = dataclasses.replace(cfg, vocab_size=32, layers=1)
    syn = deberta.synthetic_state(small, seed=1)
    assert sorted(syn) == sorted(deberta.state_names(small))
    H = small.hidden
    ok = dict(syn, **{"embeddings.position_ids": torch.arange(small.max_pos)[None]})
    assert sorted(deberta.check_state(small, ok)) == sorted(ok)
    for name in ("encoder.layer.0.attention.self.pos_key_proj.weight", "encoder.layer.0.attention.self.pos_query_proj.weight"):
        with pytest.raises(NotImplementedError, match="pos_key_proj / pos_query_proj"):
            deberta.check_state(small, dict(ok, **{name: torch.zeros(H, H)}))
    for name in ("embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight", "encoder.conv.conv.weight",
                 "embeddings.embed_proj.weight", "lm_predictions.lm_head.dense.weight"):
        with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
            deberta.check_state(small, dict(ok, **{name: torch.zeros(4, H)}))
    missing = dict(syn)
    del missing["encoder.rel_embeddings.weight"]
    with pytest.raises(ValueError, match="rel_embeddings"):
        deberta.check_state(small, missing)


def test_dist_index_is_transformers_bucket_of_every_distance():
    from transformers.models.deberta_v2.modeling_deberta_v2 import build_relative_position

    from tensor_truth_amd import deberta

    z = _expected()
    got = deberta.build_dist_index(256, 512)
    assert got.dtype == torch.int32 and got.shape == (1023,)
    assert got.tolist() == z["dist_index"].tolist()                     # entry for entry
    rel = build_relative_position(torch.zeros(512, 1), torch.zeros(512, 1), bucket_size=256, max_position=512)[0]
    fresh = torch.clamp(torch.cat([rel[0, 1:].flip(0), rel[:, 0]]) + 256, 0, 511)        # d = -511 .. 511
    assert got.tolist() == fresh.tolist()
    # what the kernels rely on: the identity up to +-128, logarithmic and monotone beyond, inside the table
    c = 511
    assert [int(got[c + d]) for d in (-128, -1, 0, 1, 128)] == [128, 255, 256, 257, 384]
    assert int(got[c + 129]) == 385 and int(got[c + 511]) == 511 and int(got[c - 511]) == 1 and int(got[c + 300]) < 256 + 300
    assert (got[1:] >= got[:-1]).all() and int(got.min()) >= 0 and int(got.max()) <= 511
    # another max_relative_positions changes the log part only
    other = deberta.build_dist_index(256, 512, 384)
    assert other[c - 128:c + 129].tolist() == got[c - 128:c + 129].tolist() and other.tolist() != got.tolist()
    with pytest.raises(ValueError):
        deberta.build_dist_index(0, 512)


def test_pair_layout_of_the_tokenizer():
    from tensor_truth_amd.tokenization import HashTokenizer, SpecialTokens, load_tokenizer

    sp = SpecialTokens("deberta-v2")
    assert (sp.bos, sp.pad, sp.eos, sp.unk, sp.first_free, sp.pair_sep) == (1, 0, 2, 3, 4, [2])
    tk = load_tokenizer(None, "deberta-v2", 600)
    assert isinstance(tk, HashTokenizer)
    ids = tk.encode("a few words")
    assert ids[0] == 1 and ids[-1] == 2 and min(ids[1:-1]) >= 4 and max(ids) < 600
    pair, types = tk.encode_pair("a b", "c d e")
    assert len(pair) == 8 and pair[0] == 1 and pair[3] == 2 and pair[-1] == 2 and pair.count(2) == 2 and set(types) == {0}
    assert all(4 <= t < 600 for i, t in enumerate(pair) if i not in (0, 3, 7))
    long_pair, _ = tk.encode_pair("q " * 40, "d " * 900, 512)
    assert len(long_pair) == 512 and long_pair[0] == 1 and long_pair[-1] == 2
    # the layouts the other families have always had
    assert SpecialTokens("xlmr").pair_sep == [2, 2] and SpecialTokens("bert").bos == 101


def test_packing_has_no_position_offset():
    from tensor_truth_amd import weights
    from tensor_truth_amd.encoder import pack_tokens

    cfg = weights._config_from_hf(_config_json())
    b = pack_tokens([[1, 5, 6, 2], [1, 7, 2]], cfg)
    assert b.pos[:4].tolist() == [0, 1, 2, 3] and b.ids[4] == cfg.pad_id == 0 and b.types is None
    long = pack_tokens([[1] + [5] * 700], cfg)
    assert long.max_len == 512


@pytest.mark.default_precision
def test_reference_precision_is_refused():
    """No torch_dtype (the reference's own call) and float32 resolve to the reference precision, which DeBERTa does not have: refused
    before anything touches a device, naming the two types that exist."""
    from tensor_truth_amd import precision, weights

    cfg = weights._config_from_hf(_config_json())
    for mk in (None, {"torch_dtype": "float32"}, {"torch_dtype": torch.float32}, {"precision": "fp8"}):
        with pytest.raises(NotImplementedError, match="DeBERTa.*bfloat16.*float16"):
            precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "reranker fixture")
    # the two modes that exist get as far as the weights class, which has no CPU path
    for mk in ({"torch_dtype": "bfloat16"}, {"torch_dtype": "float16"}):
        with pytest.raises(RuntimeError, match="HIP device"):
            precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "reranker fixture")


def test_known_names_resolve_to_the_published_geometry():
    from tensor_truth_amd import deberta, weights

    want = {"mixedbread-ai/mxbai-rerank-xsmall-v1": (384, 6, 12, 1536), "mixedbread-ai/mxbai-rerank-base-v1": (768, 12, 12, 3072),
            "mixedbread-ai/mxbai-rerank-large-v1": (1024, 16, 24, 4096)}
    assert sorted(deberta.KNOWN_CONFIGS) == sorted(want)
    for name, (hidden, heads, layers, ffn) in want.items():
        cfg = deberta.KNOWN_CONFIGS[name]
        assert (cfg.arch, cfg.hidden, cfg.heads, cfg.layers, cfg.ffn) == ("deberta-v2", hidden, heads, layers, ffn)
        assert (cfg.vocab_size, cfg.max_pos, cfg.max_seq_len, cfg.ln_eps, cfg.num_labels, cfg.pad_id) == (128100, 512, 512, 1e-7, 1, 0)
        assert (cfg.position_buckets, cfg.max_relative_positions) == (256, 512)
        deberta.check_config(cfg)
    tiny = dataclasses.replace(deberta.MXBAI_RERANK_XSMALL, vocab_size=50, layers=1)
    cfg, state, mdir = weights.resolve("mixedbread-ai/mxbai-rerank-xsmall-v1", {"synthetic_seed": 3, "encoder_config": tiny},
                                       torch.device("cpu"), want_head=True)
    assert cfg is tiny and mdir is None and sorted(state) == sorted(deberta.state_names(tiny))
    got = weights.resolve("mixedbread-ai/mxbai-rerank-base-v1", {"state_dict": {}}, torch.device("cpu"), want_head=True)[0]
    assert got is deberta.MXBAI_RERANK_BASE
    # the fixture directory resolves from its own config.json
    cfg, state, mdir = weights.resolve(FIXTURE, None, torch.device("cpu"), want_head=True)
    assert cfg.arch == "deberta-v2" and mdir == FIXTURE and "deberta.encoder.rel_embeddings.weight" in state
    assert weights.head_activation(FIXTURE, FIXTURE, None) == "sigmoid"


def test_ctypes_mirror_matches_tt_hip_h(tmp_path):
    from test_struct_layouts import INCLUDE, _c_fields, _c_layouts

    from tensor_truth_amd.deberta import _DbW
    from tensor_truth_amd.encoder import _EncW

    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    header = open(os.path.join(INCLUDE, "tt_hip.h")).read()
    fields = _c_fields(header, "tt_deberta_weights")
    assert fields == [f for f, _ in _DbW._fields_] == ["enc", "pos_key", "pos_query", "dist_index", "n_pos", "max_pos",
                                                       "pooler_dense_wt", "pooler_dense_b", "cls_w", "cls_b"]
    size, layout = _c_layouts(tmp_path, cc, {"tt_deberta_weights": fields})["tt_deberta_weights"]
    assert (ctypes.sizeof(_DbW), [(f, getattr(_DbW, f).offset, getattr(_DbW, f).size) for f, _ in _DbW._fields_]) == (size, layout)
    assert dict(_DbW._fields_)["enc"] is _EncW          # the encoder's struct by value


def test_library_binds_the_new_entry_points(built_lib):
    from tensor_truth_amd import _lib
    from tensor_truth_amd.encoder import DEBERTA_BF16_PATH, DEBERTA_FP16_PATH

    lib = _lib.load_library()
    for p in (DEBERTA_BF16_PATH, DEBERTA_FP16_PATH):
        assert p.cls_forward is None and p.head is None and p.no_fp8 and p.pool_last is None
        for name in (p.forward, p.workspace, p.pooled_head):
            assert hasattr(lib, name)
    assert hasattr(lib, "tt_attention_disentangled") and hasattr(lib, "tt_attention_disentangled_f16")
