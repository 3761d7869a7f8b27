"""CPU: the host side of the MPNet path (tensor_truth_amd/mpnet.py, weights._mpnet_config_from_hf, precision._build_mpnet).

Config parsing from the fixture directory (tests/golden/make_mpnet_golden.py) and each refusal by field name; the extra-tensor rule;
the refused reference precision; positions and the usable length; the ctypes mirror of ``tt_mpnet_weights`` against the header (the
way tests/test_struct_layouts.py checks the encoder structs); and the host-built distance table against transformers' own
``MPNetEncoder.relative_position_bucket`` for every distance in [-300, 300].  Before the MPNet path existed the fixture's config was
parsed as XLM-R and its weights died with ``KeyError: 'embeddings.token_type_embeddings.weight'`` / ``attention.self.query.weight``.
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
FIXTURE = os.path.join(GOLDEN, "mpnet_mean_l2")


def _config_json():
    with open(os.path.join(FIXTURE, "config.json")) as f:
        return json.load(f)


def test_fixture_config_and_state_load():
    from tensor_truth_amd import mpnet, weights

    cfg = weights._config_from_hf(_config_json())
    assert (cfg.arch, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.vocab_size, cfg.max_pos) == ("mpnet", 256, 2, 4, 512, 600, 514)
    assert (cfg.pad_id, cfg.type_vocab, cfg.num_labels, cfg.ln_eps) == (1, 1, 0, 1e-5)
    assert weights.pooling_mode(FIXTURE) == "mean_tokens"        # (the embedder maps it to "mean")
    mpnet.check_config(cfg)
    state = weights.load_state(FIXTURE)
    assert "pooler.dense.weight" in state and "encoder.layer.0.attention.attn.q.weight" in state
    sd = mpnet.check_state(cfg, state)          # the fixture is an MPNet of its own config: nothing missing, nothing refused
    assert set(mpnet.state_names(cfg)) <= set(sd) and len(mpnet.state_names(cfg)) == 5 + 2 * 16
    # a want_head caller (the reranker's loader) gets no head either: MPNet is an embedder here
    assert weights._config_from_hf(_config_json(), 1).num_labels == 0
    # layer_norm_eps comes from the config; transformers' default where it names none
    d = _config_json()
    del d["layer_norm_eps"]
    assert weights._config_from_hf(d).ln_eps == 1e-12


def test_other_model_types_parse_as_before():
    from tensor_truth_amd import weights

    d = dict(vocab_size=100, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
             max_position_embeddings=66)
    assert weights._config_from_hf(dict(d, model_type="xlm-roberta")).arch == "xlmr"
    assert weights._config_from_hf(dict(d, model_type="bert")).arch == "bert"
    assert weights._config_from_hf(dict(d, model_type="something-else")).arch == "xlmr"


def test_refusals_name_the_field():
    from tensor_truth_amd import mpnet, weights

    with pytest.raises(NotImplementedError, match="relative_attention_num_buckets=64"):
        weights._config_from_hf(dict(_config_json(), relative_attention_num_buckets=64))
    with pytest.raises(NotImplementedError, match="hidden_act='relu'"):
        weights._config_from_hf(dict(_config_json(), hidden_act="relu"))
    with pytest.raises(NotImplementedError, match="MPNetForSequenceClassification.*ForSequenceClassification"):
        weights._config_from_hf(dict(_config_json(), architectures=["MPNetForSequenceClassification"]))
    cfg = weights._config_from_hf(_config_json())
    for kw, text in ((dict(hidden=320, heads=5), "hidden_size=320"), (dict(hidden=1152, heads=18), "hidden_size=1152"),
                     (dict(heads=8), "head_dim must be 64"), (dict(ffn=200), "intermediate_size=200"),
                     (dict(num_labels=1), "classification heads")):
        with pytest.raises(NotImplementedError, match=text):
            mpnet.check_config(dataclasses.replace(cfg, **kw))


def test_extra_tensor_rule():
    from tensor_truth_amd import mpnet, weights

    cfg = dataclasses.replace(weights._config_from_hf(_config_json()), vocab_size=32, layers=1)
    sd = mpnet.synthetic_state(cfg, seed=1)
    assert sorted(sd) == sorted(mpnet.state_names(cfg))
    H = cfg.hidden
    ok = dict(sd, **{"pooler.dense.weight": torch.zeros(H, H), "pooler.dense.bias": torch.zeros(H),
                     "embeddings.position_ids": torch.arange(cfg.max_pos)[None]})
    assert sorted(mpnet.check_state(cfg, ok)) == sorted(ok)
    # the ``mpnet.`` prefix of the *For... exports is stripped
    assert sorted(mpnet.check_state(cfg, {"mpnet." + k: v for k, v in ok.items()})) == sorted(ok)
    with pytest.raises(NotImplementedError, match=r"lm_head\.decoder\.weight"):
        mpnet.check_state(cfg, dict(ok, **{"lm_head.decoder.weight": torch.zeros(32, H)}))
    with pytest.raises(NotImplementedError, match=r"classifier\.dense\.weight"):
        mpnet.check_state(cfg, dict(ok, **{"classifier.dense.weight": torch.zeros(H, H)}))
    missing = dict(sd)
    del missing["encoder.relative_attention_bias.weight"]
    with pytest.raises(ValueError, match="relative_attention_bias"):
        mpnet.check_state(cfg, missing)


@pytest.mark.default_precision
def test_reference_precision_is_refused():
    """No torch_dtype (the reference's own call) and float32 resolve to the reference precision, which MPNet does not have: refused
    before anything touches a device, naming the two types that exist."""
    from tensor_truth_amd import precision, weights

    cfg = weights._config_from_hf(_config_json())
    for mk in (None, {"torch_dtype": "float32"}, {"torch_dtype": torch.float32}, {"precision": "fp8"}):
        with pytest.raises(NotImplementedError, match="MPNet.*bfloat16.*float16"):
            precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "embedder fixture")
    # the two modes that exist get as far as the weights class, which has no CPU path
    for mk in ({"torch_dtype": "bfloat16"}, {"torch_dtype": "float16"}):
        with pytest.raises(RuntimeError, match="HIP device"):
            precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "embedder fixture")


def test_positions_and_usable_length():
    from tensor_truth_amd import weights
    from tensor_truth_amd.encoder import pack_flat, pack_token_matrix, pack_tokens

    cfg = weights._config_from_hf(_config_json())
    assert cfg.max_seq_len == 512                     # 514 positions, the first two reserved as in XLM-R
    seqs = [[0, 5, 6, 2], [0, 7, 2]]
    b = pack_tokens(seqs, cfg)
    assert b.pos[:4].tolist() == [2, 3, 4, 5] and b.pos[8:11].tolist() == [2, 3, 4] and b.types is None
    assert b.ids[4] == cfg.pad_id and b.pos[4] == 0   # filler rows
    flat = np.asarray(sum(seqs, []), dtype=np.int32)
    f = pack_flat(flat, np.asarray([0, 4]), np.asarray([4, 3]), np.asarray([0, 1]), cfg)
    assert np.array_equal(f.pos, b.pos) and np.array_equal(f.ids, b.ids)
    m = pack_token_matrix(np.asarray([[0, 5, 2], [0, 6, 2]], dtype=np.int32), cfg)
    assert m.pos[:3].tolist() == [2, 3, 4] and m.pos[8:11].tolist() == [2, 3, 4]
    long = pack_tokens([list(range(4, 604 - 4)) * 2], dataclasses.replace(cfg, vocab_size=1000))
    assert long.max_len == 512 and int(long.pos.max()) == 513


def test_hash_tokenizer_uses_the_roberta_layout():
    from tensor_truth_amd.tokenization import HashTokenizer, load_tokenizer

    tk = load_tokenizer(None, "mpnet", 600)
    assert isinstance(tk, HashTokenizer) and (tk.sp.bos, tk.sp.pad, tk.sp.eos) == (0, 1, 2)
    ids = tk.encode("a few words")
    assert ids[0] == 0 and ids[-1] == 2 and min(ids[1:-1]) >= 4 and max(ids) < 600
    pair, types = tk.encode_pair("a b", "c d e")
    assert pair[0] == 0 and pair[3:5] == [2, 2] and pair[-1] == 2 and set(types) == {0}
    x = load_tokenizer(None, "xlmr", 600)
    assert x.encode("a few words") == ids               # the layout "xlmr" has always had


def test_known_names_resolve_to_the_base_geometry():
    from tensor_truth_amd import mpnet, weights

    for name in ("sentence-transformers/all-mpnet-base-v2", "sentence-transformers/multi-qa-mpnet-base-dot-v1",
                 "sentence-transformers/multi-qa-mpnet-base-cos-v1", "sentence-transformers/all-mpnet-base-v1"):
        cfg = mpnet.KNOWN_CONFIGS[name]
        assert (cfg.arch, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.max_seq_len) == ("mpnet", 768, 12, 12, 3072, 514, 512)
    tiny = dataclasses.replace(mpnet.MPNET_BASE, vocab_size=50, layers=1)
    cfg, state, mdir = weights.resolve("sentence-transformers/all-mpnet-base-v2", {"synthetic_seed": 3, "encoder_config": tiny},
                                       torch.device("cpu"), want_head=False)
    assert cfg is tiny and mdir is None and sorted(state) == sorted(mpnet.state_names(tiny))
    got = weights.resolve("sentence-transformers/all-mpnet-base-v2", {"state_dict": {}}, torch.device("cpu"), want_head=False)[0]
    assert got is mpnet.MPNET_BASE


def test_distance_table_is_the_models_bucket_function():
    """Every distance in [-300, 300]: the host's bucket equals ``MPNetEncoder.relative_position_bucket(key - query)``; the table
    over the clamped distance holds ``rel_bias[bucket][h] * log2(e)``; and the facts the kernel's clamp relies on."""
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder

    from tensor_truth_amd import mpnet

    d = torch.arange(-300, 301, dtype=torch.long)
    want = MPNetEncoder.relative_position_bucket(d, num_buckets=32).tolist()
    got = [mpnet.bucket_of_distance(int(x)) for x in d]
    assert got == want
    assert mpnet.bucket_of_distance(1) == 17 and mpnet.bucket_of_distance(-1) == 1      # a key one row after / before its query
    f = [mpnet.bucket_of_distance(-m) for m in range(0, 301)]
    assert [m for m in range(1, 301) if f[m] != f[m - 1]] == list(range(1, 9)) + [12, 16, 23, 32, 46, 64, 91]
    buckets = mpnet.distance_buckets()
    assert buckets.shape == (257,) and buckets.tolist() == want[300 - 128: 300 + 129]
    # beyond +-128 every distance shares the bucket of the clamped one
    assert set(want[: 300 - 128]) == {want[300 - 128]} == {15} and set(want[300 + 129:]) == {want[300 + 128]} == {31}
    rel = torch.randn(32, 4, generator=torch.Generator().manual_seed(2)) * 3
    table = mpnet.distance_table(rel)
    assert table.shape == (4, 257) and table.dtype == torch.float32
    for h in range(4):
        for dist in (-300, -129, -128, -91, -8, -1, 0, 1, 7, 8, 90, 128, 300):
            c = min(max(dist, -128), 128)
            assert table[h, c + 128].item() == pytest.approx(rel[want[dist + 300], h].item() * 1.4426950408889634, rel=1e-6)
    with pytest.raises(ValueError, match="relative_attention_bias"):
        mpnet.distance_table(torch.zeros(16, 4))


def test_ctypes_mirror_matches_tt_hip_h(tmp_path):
    from test_struct_layouts import INCLUDE, _c_fields, _c_layouts

    from tensor_truth_amd.encoder import _EncW
    from tensor_truth_amd.mpnet import _MpW

    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host C compiler")
    header = open(os.path.join(INCLUDE, "tt_hip.h")).read()
    fields = _c_fields(header, "tt_mpnet_weights")
    assert fields == [f for f, _ in _MpW._fields_] == ["enc", "rel_bias", "bias_table"]
    size, layout = _c_layouts(tmp_path, cc, {"tt_mpnet_weights": fields})["tt_mpnet_weights"]
    assert (ctypes.sizeof(_MpW), [(f, getattr(_MpW, f).offset, getattr(_MpW, f).size) for f, _ in _MpW._fields_]) == (size, layout)
    assert dict(_MpW._fields_)["enc"] is _EncW          # the encoder's struct by value


def test_library_binds_the_new_entry_points(built_lib):
    from tensor_truth_amd import _lib
    from tensor_truth_amd.encoder import MPNET_BF16_PATH, MPNET_FP16_PATH

    lib = _lib.load_library()
    for p in (MPNET_BF16_PATH, MPNET_FP16_PATH):
        assert p.cls_forward is None and p.head is None and p.no_fp8 and p.pool_last is None
        for name in (p.forward, p.workspace, p.pool, p.pool_mean):
            assert hasattr(lib, name)
    assert hasattr(lib, "tt_attention_relbias") and hasattr(lib, "tt_attention_relbias_f16")
