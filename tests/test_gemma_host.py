"""CPU: the host side of the EmbeddingGemma path (tensor_truth_amd/gemma.py, weights._config_from_hf, precision.build_encoder):
config parsing of the fixture and of the 300m values, the window rule on the value config.json holds, every refusal by field name,
extra and missing tensors, the sentence-transformers modules, prompts, the precision refusals, and the ctypes mirrors against the
header's structs.  No GPU is touched: everything refused is refused before a device tensor exists."""
import ctypes
import dataclasses
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemma_mean_l5")

# google/embeddinggemma-300m's config.json values (the model card's file), in the older spelling of the two RoPE bases
CONFIG_300M = dict(model_type="gemma3_text", architectures=["Gemma3TextModel"], vocab_size=262144, hidden_size=768,
                   intermediate_size=1152, num_hidden_layers=24, num_attention_heads=3, num_key_value_heads=1, head_dim=256,
                   max_position_embeddings=2048, sliding_window=512, query_pre_attn_scalar=256, rms_norm_eps=1e-6,
                   hidden_activation="gelu_pytorch_tanh", attention_bias=False, attn_logit_softcapping=None,
                   use_bidirectional_attention=True, rope_theta=1000000.0, rope_local_base_freq=10000.0, pad_token_id=0,
                   layer_types=(["sliding_attention"] * 5 + ["full_attention"]) * 4)


def _fixture_config():
    with open(os.path.join(FIXTURE, "config.json")) as f:
        return json.load(f)


def test_fixture_config_is_parsed():
    from tensor_truth_amd import gemma, weights

    cfg = weights._config_from_hf(_fixture_config())
    assert isinstance(cfg, gemma.GemmaConfig) and cfg.arch == "gemma3_text"
    assert (cfg.hidden, cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.ffn, cfg.layers, cfg.vocab_size) == (256, 2, 1, 256, 192, 5, 384)
    assert cfg.max_pos == cfg.max_seq_len == 1024 and cfg.ln_eps == 1e-6 and cfg.num_labels == 0
    assert cfg.layer_types == ("sliding_attention", "sliding_attention", "full_attention", "sliding_attention", "full_attention")
    assert (cfg.global_rope_theta, cfg.local_rope_theta) == (1e6, 1e4)
    gemma.check_config(cfg)


def test_300m_values_are_parsed():
    from tensor_truth_amd import gemma, weights

    cfg = weights._config_from_hf(dict(CONFIG_300M))
    assert cfg == gemma.EMBEDDINGGEMMA_300M
    assert cfg.window == 256 and cfg.layer_types.count("full_attention") == 4 and cfg.layer_types[5] == "full_attention"
    gemma.check_config(cfg)
    # the newer spelling of the bases, and a config without layer_types (derived from the pattern, as transformers derives it)
    d = dict(CONFIG_300M, rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": 5e5},
                                           "sliding_attention": {"rope_type": "default", "rope_theta": 2e4}})
    del d["layer_types"], d["rope_theta"], d["rope_local_base_freq"]
    cfg = weights._config_from_hf(d)
    assert (cfg.global_rope_theta, cfg.local_rope_theta) == (5e5, 2e4) and cfg.layer_types == gemma.EMBEDDINGGEMMA_300M.layer_types
    assert gemma.embed_scale(768) == 27.75 and gemma.embed_scale(256) == 16.0


@pytest.mark.parametrize("on_disk,window", [(512, 256), (33, 16), (32, 16), (1, 0), (4096, 2048)])
def test_window_rule_on_the_value_config_json_holds(on_disk, window):
    """transformers loads S as S // 2 + 1 and masks with |q - k| < that: |q - k| <= S // 2."""
    from tensor_truth_amd import weights

    assert weights._config_from_hf(dict(CONFIG_300M, sliding_window=on_disk)).window == window
    assert _fixture_config()["sliding_window"] == 33 and weights._config_from_hf(_fixture_config()).window == 16


@pytest.mark.parametrize("change,field", [
    (dict(use_bidirectional_attention=False), "use_bidirectional_attention"),
    (dict(use_bidirectional_attention=None), "use_bidirectional_attention"),
    (dict(attn_logit_softcapping=50.0), "attn_logit_softcapping"),
    (dict(attention_bias=True), "attention_bias"),
    (dict(hidden_activation="gelu"), "hidden_activation"),
    (dict(rope_parameters={"full_attention": {"rope_type": "linear", "factor": 8.0, "rope_theta": 1e6},
                           "sliding_attention": {"rope_type": "default", "rope_theta": 1e4}}), "rope_type"),
    (dict(rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": 1e6},
                           "sliding_attention": {"rope_type": "yarn", "rope_theta": 1e4}}), "rope_type"),
    (dict(rope_scaling={"rope_type": "linear", "factor": 8.0}), "rope_type"),
    (dict(query_pre_attn_scalar=128), "query_pre_attn_scalar"),
    (dict(layer_types=["sliding_attention", "chunked_attention"] * 12), "layer_types"),
    (dict(architectures=["Gemma3TextForSequenceClassification"]), "ForSequenceClassification"),
])
def test_variants_are_refused_by_field_name(change, field):
    from tensor_truth_amd import weights

    d = dict(CONFIG_300M)
    if change.get("use_bidirectional_attention", 0) is None:
        del d["use_bidirectional_attention"]
    else:
        d.update(change)
    with pytest.raises(NotImplementedError, match=field):
        weights._config_from_hf(d)


@pytest.mark.parametrize("change,text", [(dict(head_dim=128), "head_dim"), (dict(hidden=1152), "hidden_size"),
                                         (dict(hidden=320), "hidden_size"), (dict(ffn=1100), "intermediate_size"),
                                         (dict(heads=3, kv_heads=2), "num_key_value_heads"),
                                         (dict(layer_types=("full_attention",) * 3), "layer_types")])
def test_shapes_off_the_kernels_limits_are_refused(change, text):
    from tensor_truth_amd import gemma

    with pytest.raises((NotImplementedError, ValueError), match=text):
        gemma.check_config(dataclasses.replace(gemma.EMBEDDINGGEMMA_300M, **change))


def _small():
    from tensor_truth_amd import gemma

    cfg = dataclasses.replace(gemma.EMBEDDINGGEMMA_300M, vocab_size=64, hidden=128, ffn=64, heads=1, layers=2,
                              layer_types=("sliding_attention", "full_attention"))
    return cfg, gemma.synthetic_state(cfg, seed=3)


def test_state_names_and_the_checkpoint_walk():
    from tensor_truth_amd import gemma, weights

    cfg = weights._config_from_hf(_fixture_config())
    sd = weights.load_state(FIXTURE)
    assert sorted(gemma._strip_prefix(sd)) == sorted(gemma.state_names(cfg))
    assert all(t.dtype == torch.bfloat16 for t in sd.values())
    sd.update(gemma.dense_modules(FIXTURE))
    assert gemma.check_state(cfg, sd).keys() == gemma._strip_prefix(sd).keys()
    # a *ForCausalLM export: the model. prefix is stripped and the lm_head plays no part
    causal_lm = {"model." + k: v for k, v in sd.items() if not k.startswith("dense.")}
    causal_lm.update({k: sd[k] for k in gemma.DENSE_NAMES}, **{"lm_head.weight": sd["embed_tokens.weight"]})
    assert "layers.4.mlp.down_proj.weight" in gemma.check_state(cfg, causal_lm)


def test_extra_and_missing_tensors_are_refused():
    from tensor_truth_amd import gemma

    cfg, sd = _small()
    gemma.check_state(cfg, sd)
    for extra in ("layers.0.self_attn.q_proj.bias", "vision_tower.embeddings.weight", "layers.2.mlp.up_proj.weight"):
        with pytest.raises(NotImplementedError, match=re.escape(extra)):
            gemma.check_state(cfg, dict(sd, **{extra: torch.zeros(1)}))
    for gone in ("layers.1.pre_feedforward_layernorm.weight", "layers.0.self_attn.k_norm.weight", "norm.weight", "dense.1.weight"):
        with pytest.raises(ValueError, match=re.escape(gone)):
            gemma.check_state(cfg, {k: v for k, v in sd.items() if k != gone})
    # the synthetic state draws (1 + w) norms around 0 and the 300m's Dense shape H -> 4H -> H
    assert abs(float(sd["norm.weight"].mean())) < 0.05 and tuple(sd["dense.0.weight"].shape) == (512, 128)
    assert tuple(sd["dense.1.weight"].shape) == (128, 512)


def test_weights_need_a_device_and_bf16():
    from tensor_truth_amd import gemma

    cfg, sd = _small()
    with pytest.raises(RuntimeError, match="no CPU path"):
        gemma.GemmaWeights(cfg, sd, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="bfloat16"):
        gemma.GemmaWeights(cfg, sd, torch.device("cuda:0"), dtype=torch.float16)


def _copy_fixture(tmp_path):
    d = tmp_path / "ckpt"
    shutil.copytree(FIXTURE, d, ignore=shutil.ignore_patterns("model-*.safetensors"))
    return d


def _edit(path, **kw):
    with open(path) as f:
        d = json.load(f)
    d.update(kw)
    with open(path, "w") as f:
        json.dump(d, f)


def test_dense_modules_are_parsed(tmp_path):
    from safetensors.torch import load_file, save_file

    from tensor_truth_amd import gemma, weights

    got = gemma.dense_modules(FIXTURE)
    assert list(got) == list(gemma.DENSE_NAMES)
    assert tuple(got["dense.0.weight"].shape) == (512, 256) and tuple(got["dense.1.weight"].shape) == (256, 512)
    assert got["dense.0.weight"].dtype == torch.float32
    assert weights.pooling_mode(FIXTURE) == "mean_tokens"

    d = _copy_fixture(tmp_path)
    _edit(d / "2_Dense" / "config.json", bias=True)
    with pytest.raises(NotImplementedError, match="bias"):
        gemma.dense_modules(str(d))
    _edit(d / "2_Dense" / "config.json", bias=False, activation_function="torch.nn.modules.activation.Tanh")
    with pytest.raises(NotImplementedError, match="activation_function"):
        gemma.dense_modules(str(d))
    _edit(d / "2_Dense" / "config.json", activation_function="torch.nn.modules.linear.Identity")
    sd = load_file(str(d / "3_Dense" / "model.safetensors"))
    save_file(dict(sd, **{"linear.bias": torch.zeros(256)}), str(d / "3_Dense" / "model.safetensors"))
    with pytest.raises(NotImplementedError, match="linear.bias"):
        gemma.dense_modules(str(d))
    save_file(sd, str(d / "3_Dense" / "model.safetensors"))
    gemma.dense_modules(str(d))
    _edit(d / "1_Pooling" / "config.json", pooling_mode_mean_tokens=False, pooling_mode_cls_token=True)
    with pytest.raises(NotImplementedError, match="pooling_mode_cls_token"):
        gemma.dense_modules(str(d))
    _edit(d / "1_Pooling" / "config.json", pooling_mode_mean_tokens=True, pooling_mode_cls_token=False)
    _edit(d / "config_sentence_transformers.json", truncate_dim=128)
    with pytest.raises(NotImplementedError, match="truncate_dim"):
        gemma.dense_modules(str(d))
    _edit(d / "config_sentence_transformers.json", truncate_dim=None)
    with open(d / "modules.json") as f:
        mods = json.load(f)
    with open(d / "modules.json", "w") as f:
        json.dump(mods[:2] + mods[4:], f)
    with pytest.raises(NotImplementedError, match="modules.json"):
        gemma.dense_modules(str(d))
    os.remove(d / "modules.json")
    with pytest.raises(NotImplementedError, match="modules.json"):
        gemma.dense_modules(str(d))


def test_prompts_and_tokenizer():
    from tensor_truth_amd import weights
    from tensor_truth_amd.tokenization import load_tokenizer

    cfg = weights._config_from_hf(_fixture_config())
    assert cfg.arch == "gemma3_text"
    assert weights.prompts(FIXTURE) == {"query": "task: search result | query: ", "document": "title: none | text: "}
    tk = load_tokenizer(FIXTURE, cfg.arch, cfg.vocab_size)
    q = tk.encode(weights.prompts(FIXTURE)["query"] + "w5 w17", None)
    dcm = tk.encode(weights.prompts(FIXTURE)["document"] + "w5 w17", None)
    assert q[0] == dcm[0] == 1 and q[-1] == dcm[-1] == 2 and 3 not in q + dcm and q[-3:-1] == dcm[-3:-1] == [9, 21]
    assert len(q) == 2 + 5 + 2 and len(dcm) == 2 + 4 + 2 and q != dcm
    assert tk.encode(" ".join(["w1"] * 50), 16) == [1] + [5] * 14 + [2]


@pytest.mark.default_precision
@pytest.mark.parametrize("mk,why", [(None, "reference"), ({"torch_dtype": "float32"}, "reference"),
                                    ({"torch_dtype": "float16"}, "overflow"), ({"precision": "fp8"}, "fp8")])
def test_precisions_other_than_bf16_are_refused(mk, why):
    """Through precision.build_encoder, before any weight is moved: the device is never touched."""
    from tensor_truth_amd import precision

    cfg, sd = _small()
    with pytest.raises(NotImplementedError, match="bfloat16") as e:
        precision.build_encoder(cfg, sd, torch.device("cuda:0"), mk, "embedder x")
    assert why in str(e.value)


def test_the_reranker_surface_sees_no_head():
    """weights.resolve(want_head=True) gives the config of an embedder: num_labels 0, what HipSentenceTransformerRerank turns into its
    "has no classification head" ValueError (on the GPU: tests/test_gemma_gpu.py)."""
    from tensor_truth_amd import weights

    cfg, state, mdir = weights.resolve(FIXTURE, None, torch.device("cpu"), want_head=True)
    assert cfg.num_labels == 0 and mdir == FIXTURE and "dense.0.weight" not in state
    cfg, state, _ = weights.resolve(FIXTURE, None, torch.device("cpu"), want_head=False)
    assert "dense.0.weight" in state and "dense.1.weight" in state


def test_gemma_struct_layouts(tmp_path):
    from tensor_truth_amd.gemma import _GemmaLayerW, _GemmaW

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    header = open(os.path.join(INCLUDE, "tt_hip.h")).read()
    mirrors = {"tt_gemma_weights": _GemmaW, "tt_gemma_layer_weights": _GemmaLayerW}
    assert dict(_GemmaW._fields_)["layer"]._type_ is _GemmaLayerW
    fields = {}
    for s in mirrors:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (s, s), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields[s] = [re.findall(r"\w+", d)[-1] for decl in body.split(";") if decl.strip() for d in decl.split(",")]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tt_hip.h"', "int main(void) {"]
    for s, names in fields.items():
        lines.append(f'    printf("{s} - %zu\\n", sizeof({s}));')
        lines += [f'    printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f in names]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layouts.c", tmp_path / "layouts"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    got = {s: [None, []] for s in fields}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        s, f, *nums = line.split()
        if f == "-":
            got[s][0] = int(nums[0])
        else:
            got[s][1].append((f, int(nums[0]), int(nums[1])))
    for s, S in mirrors.items():
        size, flds = got[s]
        assert size == ctypes.sizeof(S), s
        assert [f for f, _, _ in flds] == [n for n, _ in S._fields_], s
        for f, off, width in flds:
            assert (getattr(S, f).offset, getattr(S, f).size) == (off, width), (s, f)
