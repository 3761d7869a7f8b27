"""CPU: the decoder embedder's host side -- Qwen3 ``config.json`` and checkpoint-name mapping, the precision refusal, and the
``tt_decoder_weights`` / ``tt_decoder_layer_weights`` layouts against their ctypes mirrors (compiled like
tests/test_struct_layouts.py).  No GPU needed."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("qwen3_d64_r1", "qwen3_d128_r2")


def _config(name):
    with open(os.path.join(GOLDEN, name, "config.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", FIXTURES)
def test_qwen3_config_json_maps_every_size(name):
    from tensor_truth_amd import weights

    d = _config(name)
    cfg = weights._config_from_hf(d)
    assert cfg.arch == "qwen3"
    assert (cfg.hidden, cfg.layers, cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.ffn, cfg.vocab_size) == (
        d["hidden_size"], d["num_hidden_layers"], d["num_attention_heads"], d["num_key_value_heads"], d["head_dim"],
        d["intermediate_size"], d["vocab_size"])
    assert cfg.ln_eps == d["rms_norm_eps"] and cfg.rope_theta == d["rope_parameters"]["rope_theta"]
    assert cfg.max_seq_len == d["max_position_embeddings"]
    assert weights.pooling_mode(os.path.join(GOLDEN, name)) == "last"
    assert weights.prompts(os.path.join(GOLDEN, name))["query"].startswith("Instruct:")


def test_qwen3_0_6b_config_and_older_key_names():
    """The published 0.6B config.json (transformers 4.x layout: rope_theta at the top level) -> the 0.6B geometry."""
    from tensor_truth_amd import weights
    from tensor_truth_amd.decoder import QWEN3_EMBEDDING_0_6B

    d = {"architectures": ["Qwen3ForCausalLM"], "model_type": "qwen3", "vocab_size": 151669, "hidden_size": 1024,
         "num_hidden_layers": 28, "num_attention_heads": 16, "num_key_value_heads": 8, "head_dim": 128,
         "intermediate_size": 3072, "max_position_embeddings": 32768, "rms_norm_eps": 1e-6, "rope_theta": 1000000,
         "torch_dtype": "bfloat16"}
    assert weights._config_from_hf(d) == QWEN3_EMBEDDING_0_6B


def test_other_model_types_unchanged():
    from tensor_truth_amd import weights
    from tensor_truth_amd.encoder import EncoderConfig

    base = {"vocab_size": 1000, "hidden_size": 256, "num_hidden_layers": 2, "num_attention_heads": 4, "intermediate_size": 512,
            "max_position_embeddings": 130}
    assert weights._config_from_hf(dict(base, model_type="bert")) == EncoderConfig(
        arch="bert", vocab_size=1000, hidden=256, layers=2, heads=4, ffn=512, max_pos=130, type_vocab=1, pad_id=0, ln_eps=1e-5)
    for mt in ("xlm-roberta", "roberta"):
        cfg = weights._config_from_hf(dict(base, model_type=mt))
        assert cfg.arch == "xlmr" and type(cfg) is EncoderConfig


@pytest.mark.parametrize("change", [dict(attention_bias=True),
                                    dict(rope_parameters={"rope_theta": 1e6, "rope_type": "yarn", "factor": 4.0}),
                                    dict(rope_scaling={"type": "linear", "factor": 2.0}),
                                    dict(use_sliding_window=True),
                                    dict(layer_types=["sliding_attention", "full_attention"]),
                                    dict(hidden_act="gelu")], ids=lambda c: next(iter(c)))
def test_qwen3_variants_the_kernels_do_not_compute_are_refused(change):
    from tensor_truth_amd import weights

    with pytest.raises(NotImplementedError, match=next(iter(change)).replace("rope_parameters", "rope_type")
                       .replace("rope_scaling", "rope_type")):
        weights._config_from_hf(dict(_config(FIXTURES[0]), **change))


def test_qwen3_head_dim_default_is_qwen3configs():
    from tensor_truth_amd import weights

    d = {k: v for k, v in _config(FIXTURES[0]).items() if k != "head_dim"}
    assert weights._config_from_hf(d).head_dim == 128     # transformers' Qwen3Config default, not hidden // heads (= 64 here)


def test_qwen3_checkpoint_with_extra_tensors_is_refused():
    """q/k/v biases (attention_bias checkpoints) or any other tensor the forward would not read: refused, not ignored."""
    import torch

    from tensor_truth_amd import weights
    from tensor_truth_amd.decoder import DecoderWeights

    cfg = weights._config_from_hf(_config(FIXTURES[0]))
    sd = weights.load_state(os.path.join(GOLDEN, FIXTURES[0]))
    sd["layers.0.self_attn.q_proj.bias"] = torch.zeros(cfg.heads * cfg.head_dim)
    with pytest.raises(NotImplementedError, match="q_proj.bias"):
        DecoderWeights(cfg, sd, torch.device("cuda", 0))


def test_decoder_pooling_default_is_last_token():
    from tensor_truth_amd import weights

    assert weights.pooling_mode(None, "last") == "last"
    assert weights.pooling_mode(os.path.join(GOLDEN, "nonexistent"), "last") == "last"
    assert weights.pooling_mode(None) == "cls"          # encoders keep theirs


@pytest.mark.parametrize("name", FIXTURES)
def test_qwen3_state_dict_names(name):
    """Every tensor the decoder weights are built from is in the (sharded) checkpoint, under the Qwen3Model names, with the
    shapes the kernels expect; nothing else is there."""
    from tensor_truth_amd import weights
    from tensor_truth_amd.decoder import state_names
    from tensor_truth_amd.encoder import _strip_prefix

    cfg = weights._config_from_hf(_config(name))
    sd = _strip_prefix(weights.load_state(os.path.join(GOLDEN, name)))
    assert set(sd) == set(state_names(cfg))
    D, H = cfg.head_dim, cfg.hidden
    for i in range(cfg.layers):
        p = f"layers.{i}."
        assert tuple(sd[p + "self_attn.q_proj.weight"].shape) == (cfg.heads * D, H)
        assert tuple(sd[p + "self_attn.k_proj.weight"].shape) == (cfg.kv_heads * D, H)
        assert tuple(sd[p + "self_attn.q_norm.weight"].shape) == (D,)
        assert tuple(sd[p + "mlp.down_proj.weight"].shape) == (H, cfg.ffn)
    # a *ForCausalLM export carries the same tensors under "model."
    assert set(_strip_prefix({"model." + k: v for k, v in sd.items()})) == set(sd)


@pytest.mark.default_precision
def test_decoder_reference_precision_is_refused_not_substituted():
    import torch

    from tensor_truth_amd import precision, weights

    cfg = weights._config_from_hf(_config(FIXTURES[0]))
    for mk in (None, {}, {"torch_dtype": "float32"}):
        with pytest.raises(NotImplementedError) as ei:
            precision.build_encoder(cfg, {}, torch.device("cuda", 0), mk, "embedder test")
        assert "bfloat16" in str(ei.value) and "float16" in str(ei.value)


def test_decoder_struct_layouts(tmp_path):
    from tensor_truth_amd.decoder import _DecLayerW, _DecW

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler")
    header = open(os.path.join(INCLUDE, "tt_hip.h")).read()
    mirrors = {"tt_decoder_weights": _DecW, "tt_decoder_layer_weights": _DecLayerW}
    assert dict(_DecW._fields_)["layer"]._type_ is _DecLayerW
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
        assert size == __import__("ctypes").sizeof(S), s
        assert [f for f, _, _ in flds] == [n for n, _ in S._fields_], s
        for f, off, sz in flds:
            assert getattr(S, f).offset == off and getattr(S, f).size == sz, (s, f)


def test_decoder_bad_shapes_refused_without_a_device(built_lib):
    """head_dim outside {64, 128}, heads not a multiple of kv_heads, hidden > 1024: refused by the argument checks -- with a NULL
    workspace and NULL token arrays, so nothing can have been launched -- and sized as 0 bytes."""
    import ctypes

    from tensor_truth_amd import _lib
    from tensor_truth_amd.decoder import _DecLayerW, _DecW

    lib = _lib.load_library()
    layers = (_DecLayerW * 1)()
    for sfx in ("", "_f16"):
        for kw, code, text in ((dict(head_dim=96), -2, "head_dim"), (dict(heads=6, kv_heads=4), -1, "kv_heads"),
                               (dict(hidden=2048), -2, "hidden")):
            a = dict(hidden=1024, layers=1, heads=16, kv_heads=8, head_dim=128, ffn=3072, vocab=1000, rms_eps=1e-6,
                     rope_theta=1e6, embed=1, final_norm=1)
            a.update(kw)
            w = _DecW(layer=ctypes.cast(layers, ctypes.POINTER(_DecLayerW)), **a)
            assert getattr(lib, "tt_decoder_workspace_bytes" + sfx)(ctypes.byref(w), 256) == 0
            rc = getattr(lib, "tt_decoder_forward" + sfx)(ctypes.byref(w), None, None, None, None, None, 1, 256, 16, None, None, 0, None)
            assert rc == code, (kw, rc)
            assert text in lib.tt_last_error().decode()
