"""EmbeddingGemma embedders (``Gemma3TextModel`` with ``use_bidirectional_attention``: google/embeddinggemma-300m) on the HIP path:
weights in the layout of ``tt_gemma_weights`` (include/tt_hip.h), driven by the one host-side ``encoder.Encoder`` through the
``GEMMA_BF16_PATH`` record.

The reference embeds with whatever Hugging Face name its config holds (``app_utils/config_schema.py:96-104``,
``services/model_manager.py:214-260``).  Every size comes from ``config.json`` (``weights._config_from_hf``): the per-layer
attention type (``layer_types``), the two RoPE bases, the window.  Positions are 0-based within each sequence (RoPE; no position
table).  The sentence-transformers modules behind the transformer -- ``Pooling`` (mean), two bias-free ``Dense`` modules with the
identity activation, ``Normalize`` -- are read from the checkpoint directory (``dense_modules``) and run in fp32
(``tt_gemma_pool_dense``).  Precision: bf16 only.  The model card rules float16 out (the activations overflow), and the
reference-precision default of the XLM-R / BERT family has no implementation here (``precision.build_encoder``).
"""
from __future__ import annotations

import ctypes
import json
import os
from ctypes import POINTER, Structure, c_float, c_int32, c_void_p
from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch

from .encoder import GEMMA_BF16_PATH, EncoderConfig, _FamilyWeights, _strip_prefix

LAYER_KINDS = ("full_attention", "sliding_attention")


@dataclass(frozen=True)
class GemmaConfig(EncoderConfig):
    """The ``EncoderConfig`` fields (``ln_eps`` = ``rms_norm_eps``; ``pad_id`` = the filler ``pack_tokens`` writes into rows of no
    sequence) plus grouped-query attention -- ``kv_heads`` KV heads of ``head_dim`` each -- and what the attention reads per layer:
    ``layer_types[i]`` is "full_attention" or "sliding_attention"; a sliding layer keeps key k for query q iff
    ``|q - k| <= window`` and rotates with ``local_rope_theta``.  ``window`` is ``sliding_window // 2`` of the value config.json
    holds: transformers rewrites a bidirectional config's S to ``S // 2 + 1`` when it loads it and masks with ``|q - k| <`` that."""

    arch: str = "gemma3_text"
    kv_heads: int = 0
    head_dim: int = 0
    layer_types: Tuple[str, ...] = ()
    global_rope_theta: float = 1e6
    local_rope_theta: float = 1e4
    window: int = 0


class _GemmaLayerW(Structure):
    """tt_gemma_layer_weights."""
    _fields_ = [(n, c_void_p) for n in ("qkv_w", "q_norm", "k_norm", "o_w", "input_norm", "post_attn_norm", "pre_ffn_norm",
                                        "post_ffn_norm", "gate_up_w", "down_w")] + [("sliding", c_int32)]


class _GemmaW(Structure):
    """tt_gemma_weights."""
    _fields_ = ([(n, c_int32) for n in ("hidden", "layers", "heads", "kv_heads", "head_dim", "ffn", "vocab", "window")]
                + [(n, c_float) for n in ("rms_eps", "global_rope_theta", "local_rope_theta", "embed_scale")]
                + [("embed", c_void_p), ("layer", POINTER(_GemmaLayerW)), ("final_norm", c_void_p)]
                + [("dense1_out", c_int32), ("dense2_out", c_int32), ("dense1_wt", c_void_p), ("dense2_wt", c_void_p)])


_LAYER_NORMS = ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm")
# the sentence-transformers Dense pair travels in the state dict under these names (``dense_modules`` reads them from 2_Dense/ and
# 3_Dense/; ``synthetic_state`` draws them)
DENSE_NAMES = ("dense.0.weight", "dense.1.weight")


def state_names(cfg: GemmaConfig) -> List[str]:
    """The checkpoint tensors a ``Gemma3TextModel`` of ``cfg`` carries (after the ``model.`` prefix of ``*ForCausalLM`` exports is
    stripped), in the order the weights are built from them."""
    names = ["embed_tokens.weight"]
    for i in range(cfg.layers):
        p = f"layers.{i}."
        names += [p + f"self_attn.{n}_proj.weight" for n in ("q", "k", "v", "o")]
        names += [p + "self_attn.q_norm.weight", p + "self_attn.k_norm.weight"] + [p + n + ".weight" for n in _LAYER_NORMS]
        names += [p + f"mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
    return names + ["norm.weight"]


def check_config(cfg: GemmaConfig) -> None:
    """The shapes the EmbeddingGemma kernels take (tt_gemma_forward refuses the others before a launch; say so here first)."""
    D, nq, nkv, H = cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.hidden
    if D != 256:
        raise NotImplementedError(f"gemma3_text: head_dim={D} (supported: 256)")
    if nkv <= 0 or nq % nkv:
        raise ValueError(f"gemma3_text: num_attention_heads={nq} is not a multiple of num_key_value_heads={nkv}")
    if H % 128 or H > 1024:
        raise NotImplementedError(f"gemma3_text: hidden_size={H} (a multiple of 128 up to 1024, the scan's limit)")
    if ((nq + 2 * nkv) * D) % 128 or (nq * D) % 64 or cfg.ffn <= 0 or cfg.ffn % 64:
        raise NotImplementedError(f"gemma3_text: heads={nq} kv_heads={nkv} head_dim={D} intermediate_size={cfg.ffn} do not fit the "
                                  "GEMM tiles")
    if len(cfg.layer_types) != cfg.layers or set(cfg.layer_types) - set(LAYER_KINDS):
        raise NotImplementedError(f"gemma3_text: layer_types={cfg.layer_types!r} does not name full_attention / sliding_attention "
                                  f"for each of the {cfg.layers} layers")
    if cfg.window < 0 or cfg.global_rope_theta <= 0 or cfg.local_rope_theta <= 0:
        raise ValueError(f"gemma3_text: window={cfg.window} rope bases {cfg.global_rope_theta} / {cfg.local_rope_theta}")


def check_state(cfg: GemmaConfig, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``state`` without its ``model.`` prefix, after checking that it holds every tensor of ``state_names(cfg)`` plus the Dense pair
    and nothing the forward would not read: projection biases, a vision tower ... mean another variant of the architecture and are
    refused, not ignored.  A ``*ForCausalLM`` export's ``lm_head`` plays no part."""
    sd = _strip_prefix(state)
    names = state_names(cfg) + list(DENSE_NAMES)
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"checkpoint is not an EmbeddingGemma of {cfg}: missing {missing[:4]}")
    extra = sorted(set(sd) - set(names) - {"lm_head.weight"})
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the EmbeddingGemma path does not compute: {extra[:4]}")
    return sd


def dense_modules(model_dir: str) -> Dict[str, torch.Tensor]:
    """The sentence-transformers tail a checkpoint directory declares (``modules.json``), which must be Transformer -> Pooling
    (mean) -> Dense -> Dense -> Normalize: -> the two ``linear.weight`` matrices under ``DENSE_NAMES``.  Anything else -- another
    pooling, a Dense module with a bias or an activation other than the identity, a missing Normalize, ``truncate_dim`` (Matryoshka
    output sizes) -- is refused by name: no kernel here computes it."""
    from safetensors.torch import load_file

    mj = os.path.join(model_dir, "modules.json")
    if not os.path.exists(mj):
        raise NotImplementedError(f"{model_dir}: no modules.json: an EmbeddingGemma checkpoint names Pooling, two Dense modules and "
                                  "Normalize there")
    with open(mj) as f:
        mods = sorted(json.load(f), key=lambda m: m.get("idx", 0))
    kinds = [str(m.get("type", "")).rsplit(".", 1)[-1] for m in mods]
    if kinds != ["Transformer", "Pooling", "Dense", "Dense", "Normalize"]:
        raise NotImplementedError(f"{model_dir}: modules.json names {kinds}; supported: Transformer, Pooling, Dense, Dense, Normalize")
    with open(os.path.join(model_dir, mods[1]["path"], "config.json")) as f:
        pc = json.load(f)
    on = sorted(k for k, v in pc.items() if k.startswith("pooling_mode_") and v is True)
    if on != ["pooling_mode_mean_tokens"]:
        raise NotImplementedError(f"{model_dir}: pooling {on} (supported: pooling_mode_mean_tokens)")
    st = os.path.join(model_dir, "config_sentence_transformers.json")
    if os.path.exists(st):
        with open(st) as f:
            if json.load(f).get("truncate_dim") is not None:
                raise NotImplementedError(f"{model_dir}: truncate_dim is set: Matryoshka output sizes are not supported")
    out = {}
    for name, m in zip(DENSE_NAMES, mods[2:4]):
        d = os.path.join(model_dir, m["path"])
        with open(os.path.join(d, "config.json")) as f:
            dc = json.load(f)
        act = str(dc.get("activation_function", "torch.nn.modules.linear.Identity")).rsplit(".", 1)[-1]
        if dc.get("bias", True):
            raise NotImplementedError(f"{d}: bias=true: the Dense modules of the EmbeddingGemma tail carry no bias")
        if act != "Identity":
            raise NotImplementedError(f"{d}: activation_function={dc.get('activation_function')!r} (supported: Identity)")
        sd = load_file(os.path.join(d, "model.safetensors"))
        if sorted(sd) != ["linear.weight"]:
            raise NotImplementedError(f"{d}: tensors {sorted(sd)} (expected linear.weight alone)")
        w = sd["linear.weight"]
        if tuple(w.shape) != (dc.get("out_features", w.shape[0]), dc.get("in_features", w.shape[1])):
            raise ValueError(f"{d}: linear.weight {tuple(w.shape)} does not match its config.json")
        out[name] = w
    return out


def embed_scale(hidden: int) -> float:
    """sqrt(hidden) rounded to bf16, as ``Gemma3TextScaledWordEmbedding`` rounds it to the weights' type (768: 27.75)."""
    return float(torch.tensor(float(hidden) ** 0.5).to(torch.bfloat16))


class GemmaWeights(_FamilyWeights):
    """Device-resident EmbeddingGemma weights for ``tt_gemma_forward``: the projections and the embedding table in bf16 -- q/k/v
    rows concatenated into one matrix, gate/up into another -- the norm weights in fp32 as stored (the kernels add the 1), and the
    Dense pair in fp32, transposed to [in][out] (the tail kernel's threads read them row by row)."""

    _paths, _path_name = (GEMMA_BF16_PATH,), "the EmbeddingGemma path"

    def __init__(self, cfg: GemmaConfig, state: Dict[str, torch.Tensor], device: torch.device,
                 dtype: torch.dtype = torch.bfloat16):
        self._begin(cfg, device, dtype, dtypes=(torch.bfloat16,))
        check_config(cfg)
        if cfg.num_labels:
            raise NotImplementedError("gemma3_text: no classification head is supported")
        sd = check_state(cfg, state)
        mat, vec = self._loaders(sd)
        H, D, nq, nkv, F = cfg.hidden, cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.ffn
        emb = mat(["embed_tokens.weight"], (cfg.vocab_size, H))
        self._layers = (_GemmaLayerW * max(cfg.layers, 1))()
        for i in range(cfg.layers):
            p, L = f"layers.{i}.", self._layers[i]
            L.qkv_w = mat([p + f"self_attn.{n}_proj.weight" for n in ("q", "k", "v")], ((nq + 2 * nkv) * D, H))
            L.o_w = mat([p + "self_attn.o_proj.weight"], (H, nq * D))
            L.gate_up_w = mat([p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"], (2 * F, H))
            L.down_w = mat([p + "mlp.down_proj.weight"], (H, F))
            L.q_norm, L.k_norm = vec([p + "self_attn.q_norm.weight"], D), vec([p + "self_attn.k_norm.weight"], D)
            for field, name in zip(("input_norm", "post_attn_norm", "pre_ffn_norm", "post_ffn_norm"), _LAYER_NORMS):
                setattr(L, field, vec([p + name + ".weight"], H))
            L.sliding = 1 if cfg.layer_types[i] == "sliding_attention" else 0
        d1, d2 = sd[DENSE_NAMES[0]], sd[DENSE_NAMES[1]]
        if d1.dim() != 2 or d2.dim() != 2 or d1.shape[1] != H or d2.shape[1] != d1.shape[0]:
            raise ValueError(f"Dense modules {tuple(d1.shape)} -> {tuple(d2.shape)} do not chain from hidden_size={H}")
        n1, n2 = int(d1.shape[0]), int(d2.shape[0])
        if n1 % 64 or n1 > 3072 or n2 % 64 or n2 > 1024:
            raise NotImplementedError(f"gemma3_text: Dense outputs {n1} and {n2} (multiples of 64, up to 3072 and 1024, the scan's limit)")
        self.out_dim = n2
        f32 = dict(device=device, dtype=torch.float32)
        self.struct = _GemmaW(hidden=H, layers=cfg.layers, heads=nq, kv_heads=nkv, head_dim=D, ffn=F, vocab=cfg.vocab_size,
                              window=cfg.window, rms_eps=cfg.ln_eps, global_rope_theta=cfg.global_rope_theta,
                              local_rope_theta=cfg.local_rope_theta, embed_scale=embed_scale(H), embed=emb,
                              layer=ctypes.cast(self._layers, POINTER(_GemmaLayerW)), final_norm=vec(["norm.weight"], H),
                              dense1_out=n1, dense2_out=n2, dense1_wt=self._kept(d1.to(**f32).t().contiguous()).data_ptr(),
                              dense2_wt=self._kept(d2.to(**f32).t().contiguous()).data_ptr())


def synthetic_state(cfg: GemmaConfig, seed: int = 0, dense: Tuple[int, int] = (0, 0)) -> Dict[str, torch.Tensor]:
    """Seeded random EmbeddingGemma weights of ``cfg`` (fp32, CPU) with trained-model-like scales: N(0, 0.02) projections and
    embeddings, norm weights around 0 (the norms multiply by 1 + w), a Dense pair H -> ``dense[0]`` -> ``dense[1]`` (default:
    H -> 4H -> H, the 300m's shape)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std=0.02):
        return torch.randn(*shape, generator=g) * std

    H, D, nq, nkv, F = cfg.hidden, cfg.head_dim, cfg.heads, cfg.kv_heads, cfg.ffn
    n1, n2 = dense[0] or 4 * H, dense[1] or H
    sd = {"embed_tokens.weight": rnd(cfg.vocab_size, H), "norm.weight": rnd(H, std=0.1)}
    for i in range(cfg.layers):
        p = f"layers.{i}."
        sd[p + "self_attn.q_proj.weight"] = rnd(nq * D, H)
        sd[p + "self_attn.k_proj.weight"] = rnd(nkv * D, H)
        sd[p + "self_attn.v_proj.weight"] = rnd(nkv * D, H)
        sd[p + "self_attn.o_proj.weight"] = rnd(H, nq * D)
        sd[p + "self_attn.q_norm.weight"] = rnd(D, std=0.1)
        sd[p + "self_attn.k_norm.weight"] = rnd(D, std=0.1)
        for n in _LAYER_NORMS:
            sd[p + n + ".weight"] = rnd(H, std=0.1)
        sd[p + "mlp.gate_proj.weight"] = rnd(F, H)
        sd[p + "mlp.up_proj.weight"] = rnd(F, H)
        sd[p + "mlp.down_proj.weight"] = rnd(H, F)
    sd[DENSE_NAMES[0]] = rnd(n1, H)
    sd[DENSE_NAMES[1]] = rnd(n2, n1)
    return sd


def default_layer_types(layers: int, pattern: int = 6) -> Tuple[str, ...]:
    """What transformers derives when config.json names no ``layer_types``: every ``pattern``-th layer is full attention."""
    return tuple("sliding_attention" if (i + 1) % pattern else "full_attention" for i in range(layers))


# google/embeddinggemma-300m's geometry (its config.json: sliding_window 512, i.e. +-256): what the 300m-shaped tests and
# measurements build with seeded weights
EMBEDDINGGEMMA_300M = GemmaConfig(vocab_size=262144, hidden=768, layers=24, heads=3, ffn=1152, max_pos=2048, type_vocab=1, pad_id=0,
                                  ln_eps=1e-6, kv_heads=1, head_dim=256, layer_types=default_layer_types(24), global_rope_theta=1e6,
                                  local_rope_theta=1e4, window=256)
