"""CPU: the host side of the T5 encoder path (tensor_truth_amd/t5.py and its dispatch in weights.py, precision.py, embedding.py).

Config parsing and each refusal by field name, the checkpoint's tensor names, the ctypes mirrors against include/tt_hip.h, the
distance table against transformers' own bucket function, the exactness of the x 8 on the q rows, the precision and reranker
refusals, and the ``include_prompt`` range arithmetic.  No GPU."""
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
RELU, GATED = os.path.join(GOLDEN, "t5_mean_dense_l2"), os.path.join(GOLDEN, "t5_gated_mean_dense_l2")
REL = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def _config_json(d):
    with open(os.path.join(d, "config.json")) as f:
        return json.load(f)


def test_fixture_configs_parse():
    from tensor_truth_amd import t5, weights

    for d, layers, kind in ((RELU, 2, 0), (GATED, 1, 1)):
        cfg = weights._config_from_hf(_config_json(d))
        assert isinstance(cfg, t5.T5Config) and cfg.arch == "t5"
        assert (cfg.hidden, cfg.heads, cfg.ffn, cfg.layers, cfg.vocab_size, cfg.d_kv, cfg.mlp_kind) == (256, 4, 512, layers, 600, 64, kind)
        assert (cfg.pad_id, cfg.ln_eps, cfg.num_buckets, cfg.max_distance, cfg.max_seq_len, cfg.num_labels) == (0, 1e-6, 32, 128, 512, 0)
        t5.check_config(cfg)
    # the published geometries, by name
    for name, (H, nh, L, F) in {"sentence-transformers/sentence-t5-base": (768, 12, 12, 3072), "sentence-transformers/gtr-t5-large": (1024, 16, 24, 4096),
                                "hkunlp/instructor-base": (768, 12, 12, 3072), "hkunlp/instructor-large": (1024, 16, 24, 4096),
                                "sentence-transformers/sentence-t5-large": (1024, 16, 24, 4096), "sentence-transformers/gtr-t5-base": (768, 12, 12, 3072)}.items():
        c = t5.KNOWN_CONFIGS[name]
        assert (c.hidden, c.heads, c.layers, c.ffn, c.vocab_size, c.mlp_kind, c.pad_id) == (H, nh, L, F, 32128, 0, 0)
        t5.check_config(c)
    # the defaults a config.json may leave out are transformers' own
    from transformers import T5Config as HF

    hf = HF()
    assert (hf.feed_forward_proj, hf.relative_attention_num_buckets, hf.relative_attention_max_distance, hf.d_kv, hf.layer_norm_epsilon,
            hf.pad_token_id) == ("relu", 32, 128, 64, 1e-6, 0)
    bare = t5.config_from_hf({"model_type": "t5", "vocab_size": 100, "d_model": 512, "num_layers": 6, "num_heads": 8, "d_ff": 2048})
    assert (bare.mlp_kind, bare.d_kv, bare.ln_eps, bare.pad_id) == (0, 64, 1e-6, 0)


def test_refusals_name_the_field():
    from tensor_truth_amd import t5, weights

    base = _config_json(RELU)
    for patch, text in ((dict(feed_forward_proj="gelu"), "feed_forward_proj='gelu'"), (dict(feed_forward_proj="gated-silu"), "feed_forward_proj"),
                        (dict(is_decoder=True), "is_decoder=True"), (dict(relative_attention_num_buckets=64), "relative_attention_num_buckets=64"),
                        (dict(relative_attention_max_distance=256), "relative_attention_max_distance=256"),
                        (dict(architectures=["T5ForSequenceClassification"]), "classification")):
        with pytest.raises(NotImplementedError, match=text):
            weights._config_from_hf({**base, **patch})
    with pytest.raises(NotImplementedError, match="umt5.*every block"):
        weights._config_from_hf({**base, "model_type": "umt5"})
    good = weights._config_from_hf(base)
    for patch, text in ((dict(hidden=1152, heads=18), "d_model=1152"), (dict(hidden=320, heads=5), "d_model=320"), (dict(heads=8), "num_heads=8"),
                        (dict(d_kv=32, heads=8), "d_kv=32"), (dict(ffn=1100), "d_ff=1100"), (dict(num_buckets=16), "relative_attention_num_buckets=16"),
                        (dict(max_distance=64), "relative_attention_max_distance=64"), (dict(mlp_kind=2), "mlp_kind=2"),
                        (dict(num_labels=1), "classification")):
        with pytest.raises(NotImplementedError, match=text):
            t5.check_config(dataclasses.replace(good, **patch))


def test_state_names_and_refusals():
    from tensor_truth_amd import t5, weights

    for d in (RELU, GATED):
        cfg = weights._config_from_hf(_config_json(d))
        state = weights.load_state(d)
        names = t5.state_names(cfg)
        sd = t5.check_state(cfg, state)
        assert set(names) <= set(sd) and REL in names and ("encoder.block.0.layer.1.DenseReluDense.wi_0.weight" in names) == (cfg.mlp_kind == 1)
        # the sentence-transformers prefix, a bare encoder stack and the tied copy of the table are the same checkpoint
        pre = t5.check_state(cfg, {"0.auto_model." + k: v for k, v in state.items()})
        bare = t5.check_state(cfg, {(k[len("encoder."):] if k.startswith("encoder.") else k): v for k, v in state.items()})
        assert all(torch.equal(pre[n], sd[n]) and torch.equal(bare[n], sd[n]) for n in names)
        tied = {("encoder.embed_tokens.weight" if k == "shared.weight" else k): v for k, v in sd.items() if k in names}
        assert torch.equal(t5.check_state(cfg, tied)["shared.weight"], sd["shared.weight"])
        both = dict(sd, **{"encoder.embed_tokens.weight": sd["shared.weight"]})
        assert t5.check_state(cfg, both)
        dense = dict(sd, **t5.dense_module(d))
        assert t5.check_state(cfg, dense)[t5.DENSE_NAME].shape == (128, 256)
        for extra, text in (("decoder.block.0.layer.0.SelfAttention.q.weight", "a decoder stack"), ("lm_head.weight", "language-model head"),
                            ("classification_head.dense.weight", "a classifier"), ("classifier.weight", "a classifier"),
                            ("encoder.block.1.layer.0.SelfAttention.relative_attention_bias.weight", "block other than 0"),
                            ("encoder.block.0.layer.0.SelfAttention.q.bias", "does not compute")):
            with pytest.raises(NotImplementedError, match=text) as ei:
                t5.check_state(cfg, dict(sd, **{extra: torch.zeros(1)}))
            assert extra in str(ei.value)
        short = {k: v for k, v in sd.items() if k != "encoder.final_layer_norm.weight"}
        with pytest.raises(ValueError, match="missing.*final_layer_norm"):
            t5.check_state(cfg, short)
    wrong = weights._config_from_hf(_config_json(GATED))
    with pytest.raises(ValueError, match="missing.*wi_0"):
        t5.check_state(wrong, weights.load_state(RELU))


def test_directory_files(tmp_path):
    from tensor_truth_amd import t5, weights

    for d in (RELU, GATED):
        assert weights.pooling_mode(d, "mean") == "mean_tokens" and t5.include_prompt(d) and t5.max_seq_length(d) == 512
        cfg, state, mdir = weights.resolve(d, None, torch.device("cpu"), want_head=False)
        assert cfg.arch == "t5" and mdir == d and state[t5.DENSE_NAME].shape == (128, 256)
    assert t5.include_prompt(None) and t5.include_prompt(str(tmp_path)) and t5.max_seq_length(str(tmp_path)) == 512
    assert t5.dense_module(str(tmp_path)) == {}                                      # the bare transformer
    (tmp_path / "sentence_bert_config.json").write_text(json.dumps({"max_seq_length": 256}))
    assert t5.max_seq_length(str(tmp_path)) == 256
    (tmp_path / "sentence_bert_config.json").write_text(json.dumps({"max_seq_length": 4096}))
    assert t5.max_seq_length(str(tmp_path)) == 512                                   # capped
    os.makedirs(tmp_path / "1_Pooling")
    pool = {"pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True, "include_prompt": False}
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps(pool))
    assert not t5.include_prompt(str(tmp_path))
    mods = [{"idx": 0, "path": "", "type": "sentence_transformers.models.Transformer"},
            {"idx": 1, "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
            {"idx": 2, "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}]
    (tmp_path / "modules.json").write_text(json.dumps(mods))
    assert t5.dense_module(str(tmp_path)) == {}                                      # Pooling -> Normalize: no Dense
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps(dict(pool, pooling_mode_mean_tokens=False, pooling_mode_cls_token=True)))
    with pytest.raises(NotImplementedError, match="pooling_mode_cls_token"):
        t5.dense_module(str(tmp_path))
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps(pool))
    (tmp_path / "modules.json").write_text(json.dumps(mods[:2]))
    with pytest.raises(NotImplementedError, match="modules.json names"):
        t5.dense_module(str(tmp_path))
    # a Dense module with a bias or an activation is another tail
    dense = mods[:2] + [{"idx": 2, "path": "2_Dense", "type": "sentence_transformers.models.Dense"}, dict(mods[2], idx=3)]
    (tmp_path / "modules.json").write_text(json.dumps(dense))
    shutil.copytree(os.path.join(RELU, "2_Dense"), tmp_path / "2_Dense")
    assert t5.dense_module(str(tmp_path))[t5.DENSE_NAME].shape == (128, 256)
    ok = json.loads((tmp_path / "2_Dense" / "config.json").read_text())
    for patch, text in ((dict(bias=True), "bias=true"), (dict(activation_function="torch.nn.modules.activation.Tanh"), "activation_function")):
        (tmp_path / "2_Dense" / "config.json").write_text(json.dumps(dict(ok, **patch)))
        with pytest.raises(NotImplementedError, match=text):
            t5.dense_module(str(tmp_path))


def test_ctypes_mirrors_match_tt_hip_h(tmp_path):
    from test_struct_layouts import INCLUDE, _c_fields, _c_layouts

    from tensor_truth_amd.t5 import _T5LayerW, _T5W

    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.fail("no host C compiler")
    header = open(os.path.join(INCLUDE, "tt_hip.h")).read()
    mirrors = {"tt_t5_weights": _T5W, "tt_t5_layer_weights": _T5LayerW}
    assert dict(_T5W._fields_)["layer"]._type_ is _T5LayerW
    fields = {s: _c_fields(header, s) for s in mirrors}
    assert fields["tt_t5_layer_weights"] == ["ln_attn", "qkv_w", "o_w", "ln_ffn", "wi", "wo"]
    assert fields["tt_t5_weights"][:7] == ["d_model", "layers", "heads", "d_kv", "d_ff", "vocab", "mlp_kind"]
    layouts = _c_layouts(tmp_path, cc, fields)
    for s, S in mirrors.items():
        size, layout = layouts[s]
        assert fields[s] == [f for f, _ in S._fields_], s
        assert (ctypes.sizeof(S), [(f, getattr(S, f).offset, getattr(S, f).size) for f, _ in S._fields_]) == (size, layout), s


def test_library_binds_the_new_entry_points(built_lib):
    from tensor_truth_amd import _lib
    from tensor_truth_amd.encoder import T5_BF16_PATH as p

    lib = _lib.load_library()
    assert p.cls_forward is None and p.head is None and p.no_fp8 and p.pool_last is None and p.pooled_head is None
    assert p.pool_dense == "tt_t5_pool_dense" and p.hidden == torch.bfloat16
    for name in (p.forward, p.workspace, p.pool_dense):
        assert hasattr(lib, name)
    assert not hasattr(lib, "tt_t5_forward_f16")                 # bf16 only: no twin
    # a refused shape costs no workspace; the entry point needs no device for that
    from tensor_truth_amd.t5 import _T5W

    assert lib.tt_t5_workspace_bytes(ctypes.byref(_T5W(d_model=320)), 256) == 0
    assert b"d_model=320" in lib.tt_last_error()


def test_distance_table_is_transformers_bucket_function():
    """``mpnet.distance_table`` of block 0's tensor is T5's bias: the table's entry of a clamped distance is the row
    ``T5Attention._relative_position_bucket`` picks for the distance itself, for every key - query in [-600, 600]."""
    from transformers.models.t5.modeling_t5 import T5Attention

    from tensor_truth_amd.mpnet import LOG2E, distance_buckets, distance_table

    d = torch.arange(-600, 601)
    want = T5Attention._relative_position_bucket(d, bidirectional=True, num_buckets=32, max_distance=128)
    got = torch.from_numpy(distance_buckets())[d.clamp(-128, 128) + 128]
    assert torch.equal(got, want) and set(want.tolist()) == set(range(32)) - {16}      # (16 + 0: distance 0 is bucket 0)
    rel = torch.randn(32, 4, generator=torch.Generator().manual_seed(1))
    table = distance_table(rel)
    assert table.shape == (4, 257) and table.dtype == torch.float32
    assert torch.equal(table[:, d.clamp(-128, 128) + 128], (rel[want] * LOG2E).t())


def test_the_times_eight_on_the_q_rows_is_exact():
    """q rows x 8 is an exponent shift: exact in bf16, and x (8 W)^T = 8 (x W^T) bit for bit in fp32 accumulation, so
    (x (8 W)^T) / 8 -- what the attention kernel's 1 / 8 makes of it -- is T5's unscaled score."""
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(256, 256, generator=g) * 0.2).to(torch.bfloat16)
    x = torch.randn(64, 256, generator=g).to(torch.bfloat16)
    W8 = W * 8.0
    assert W8.dtype == torch.bfloat16 and torch.equal(W8.float(), W.float() * 8.0)
    assert torch.equal(x.float() @ W8.float().t(), (x.float() @ W.float().t()) * 8.0)
    assert torch.equal((x.float() @ W8.float().t()).to(torch.bfloat16), ((x.float() @ W.float().t()) * 8.0).to(torch.bfloat16))
    assert torch.equal(((x.float() @ W.float().t()).to(torch.bfloat16) * 8.0).float() * 0.125, (x.float() @ W.float().t()).to(torch.bfloat16).float())


@pytest.mark.default_precision
def test_other_precisions_are_refused():
    """No torch_dtype (the reference's own call) and float32 resolve to the reference precision; float16 and fp8 are named: none of
    them exists for T5, each refused with its reason before anything touches a device."""
    from tensor_truth_amd import precision, weights

    cfg = weights._config_from_hf(_config_json(RELU))
    for mk, why in ((None, "fp32-semantics"), ({"torch_dtype": "float32"}, "fp32-semantics"), ({"torch_dtype": torch.float16}, "clamps them"),
                    ({"torch_dtype": "float16"}, "float16's range"), ({"precision": "fp8"}, "fp8 projections exist")):
        with pytest.raises(NotImplementedError, match=f"T5 encoders.*{why}.*bfloat16"):
            precision.build_encoder(cfg, {}, torch.device("cpu"), mk, "embedder fixture")
    with pytest.raises(RuntimeError, match="HIP device"):
        precision.build_encoder(cfg, {}, torch.device("cpu"), {"torch_dtype": "bfloat16"}, "embedder fixture")
    from tensor_truth_amd.t5 import T5Weights

    with pytest.raises(NotImplementedError, match="bfloat16 only"):
        T5Weights(cfg, {}, torch.device("cpu"), dtype=torch.float16)


def test_the_reranker_surface_refuses_t5():
    """``HipSentenceTransformerRerank`` loads through ``weights.resolve(want_head=True)``: a clear ValueError, before the weights
    are read."""
    from tensor_truth_amd import weights

    for d in (RELU, GATED):
        with pytest.raises(ValueError, match="t5 checkpoints are served as embedders only"):
            weights.resolve(d, None, torch.device("cpu"), want_head=True)


def test_synthetic_weights_resolve():
    from tensor_truth_amd import t5, weights

    tiny = dataclasses.replace(t5.T5_BASE, vocab_size=50, layers=1)
    cfg, state, mdir = weights.resolve("sentence-transformers/gtr-t5-base", {"synthetic_seed": 3, "encoder_config": tiny}, torch.device("cpu"),
                                       want_head=False)
    assert cfg is tiny and mdir is None and sorted(state) == sorted(t5.state_names(tiny) + [t5.DENSE_NAME])
    assert state["encoder.block.0.layer.1.DenseReluDense.wi.weight"].shape == (3072, 768) and state[t5.DENSE_NAME].shape == (768, 768)
    cfg, _, _ = weights.resolve("hkunlp/instructor-large", {"state_dict": {}}, torch.device("cpu"), want_head=False)
    assert cfg is t5.T5_LARGE
    gated = t5.synthetic_state(dataclasses.replace(tiny, mlp_kind=1), dense=0)
    assert "encoder.block.0.layer.1.DenseReluDense.wi_1.weight" in gated and t5.DENSE_NAME not in gated


def test_tokens_end_with_the_closing_token_and_pad_with_zero():
    from tensor_truth_amd import t5
    from tensor_truth_amd.encoder import pack_tokens
    from tensor_truth_amd.tokenization import HashTokenizer

    tk = HashTokenizer("t5", 600)
    ids = tk.encode("three small words")
    assert len(ids) == 4 and ids[-1] == 1 and min(ids[:-1]) >= 3 and tk.encode("") == [1]
    assert tk.encode("one two three four five six", 4)[-1] == 1 and len(tk.encode("one two three four five six", 4)) == 4
    assert HashTokenizer("mpnet", 600).encode("a b", 3) == [0, HashTokenizer("mpnet", 600).encode("a b")[1], 2]      # the other layouts keep theirs
    cfg = dataclasses.replace(t5.T5_BASE, vocab_size=600)
    batch = pack_tokens([ids, tk.encode("x")], cfg)
    assert batch.seq_start.tolist() == [0, 8] and batch.ids[4] == 0 and batch.pos[:4].tolist() == [0, 1, 2, 3]
    assert t5.prompt_tokens(tk, "represent the sentence: ") == 4 and t5.prompt_tokens(tk, "") == 0


def test_include_prompt_range_arithmetic():
    from tensor_truth_amd import t5

    starts, lens = np.asarray([0, 16, 40], dtype=np.int32), np.asarray([9, 17, 5], dtype=np.int32)
    s, n = t5.pooled_ranges(starts, lens, 4)
    assert s.dtype == np.int32 and n.dtype == np.int32 and s.tolist() == [4, 20, 44] and n.tolist() == [5, 13, 1]
    s0, n0 = t5.pooled_ranges(starts, lens, 0)
    assert s0.tolist() == starts.tolist() and n0.tolist() == lens.tolist()
    for p, b in ((5, 2), (8, 2), (9, 0), (100, 0)):      # the first text that is left empty is the one named
        with pytest.raises(ValueError, match=f"text {b} has no token left behind its {p}-token prompt"):
            t5.pooled_ranges(starts, lens, p)
    with pytest.raises(ValueError):
        t5.pooled_ranges(starts, lens, -1)
