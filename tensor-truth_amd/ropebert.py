"""Post-LN BERT encoders with rotary positions on the HIP path: ``NomicBertModel`` (nomic-ai/nomic-embed-text-v1 / -v1.5,
``model_type: "nomic_bert"``) and ``JinaEmbeddingsV3Model`` (jina-embeddings-v3 in its transformers format, ``model_type:
"jina_embeddings_v3"``), weights in the layout of ``tt_ropebert_weights`` (include/tt_hip.h), driven by the one host-side
``encoder.Encoder`` through the ``ROPEBERT_*_PATH`` records.

The reference hands whatever Hugging Face name its config holds to ``HuggingFaceEmbedding`` (``services/model_manager.py:188-272``).
transformers implements both families with one layer class: no position table, rotate-half RoPE on q and k with one base
(``rope_parameters.rope_theta``: 1000 for NomicBERT, 20000 for Jina), bidirectional attention, post-LN residuals.  They differ in
the biases (NomicBERT has none on q / k / v / o and the MLP, Jina has all) and the MLP (SwiGLU against GELU).  Positions are 0-based
within each sequence (``position_ids = arange(seq_length)`` in both modelling files); every token of an embedder call is of type 0,
whose ``token_type_embeddings`` row is still added.  Precision: bf16 or fp16; the reference-precision default of the XLM-R / BERT
family has no implementation here (``precision.build_encoder``).

Checkpoints in the original remote-code tensor layout (``encoder.layers.N.attn.Wqkv``, ``fc11`` / ``fc12`` / ``fc2``, ``norm1`` /
``norm2``, ``emb_ln``; Jina: ``mixer.Wqkv``, ``mixer.out_proj``) are renamed by exactly the rules ``transformers/conversion_mapping.py``
lists for the two types (``to_transformers_names``); their ``config.json`` must still be in the transformers format.
"""
from __future__ import annotations

import ctypes
import re
from ctypes import POINTER, Structure, c_float, c_int32, c_void_p
from dataclasses import dataclass
from typing import Dict, List

import torch

from .encoder import ROPEBERT_BF16_PATH, ROPEBERT_FP16_PATH, EncoderConfig, _FamilyWeights

MODEL_TYPES = ("nomic_bert", "jina_embeddings_v3")
# what the installed NomicBertConfig / JinaEmbeddingsV3Config default to
DEFAULTS = {
    "nomic_bert": dict(vocab_size=30528, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                       hidden_act="silu", max_position_embeddings=2048, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0,
                       rope_theta=1000.0),
    "jina_embeddings_v3": dict(vocab_size=250002, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16,
                               intermediate_size=4096, hidden_act="gelu", max_position_embeddings=8194, type_vocab_size=1,
                               layer_norm_eps=1e-5, pad_token_id=1, rope_theta=20000.0),
}
# keys of the original remote-code configs (nomic's NomicBertConfig is a GPT2Config, Jina's an XLMRobertaFlashConfig); none of
# them is read: a config.json that carries them WITHOUT the transformers keys is refused
REMOTE_CODE_KEYS = ("n_embd", "n_layer", "n_head", "n_inner", "n_positions", "rotary_emb_base", "rotary_emb_fraction",
                    "activation_function", "lora_adaptations", "lora_main_params_trainable")


@dataclass(frozen=True)
class RopeBertConfig(EncoderConfig):
    """The ``EncoderConfig`` fields (``arch`` = the checkpoint's ``model_type``; ``pad_id`` = the filler ``pack_tokens`` writes into
    rows of no sequence) plus the RoPE base, the MLP (``"swiglu"``: NomicBERT, no biases anywhere; ``"gelu"``: Jina, biases
    everywhere)."""

    arch: str = "nomic_bert"
    rope_theta: float = 1000.0
    mlp: str = "swiglu"

    @property
    def biases(self) -> bool:
        return self.mlp == "gelu"


def config_from_hf(d: dict) -> RopeBertConfig:
    """``config.json`` of ``model_type`` "nomic_bert" / "jina_embeddings_v3" in the transformers format -> ``RopeBertConfig``;
    defaults are the installed config classes'.  Variants the kernels do not compute are refused by field name."""
    mt = d.get("model_type")
    if mt not in MODEL_TYPES:
        raise ValueError(f"model_type={mt!r} is not one of {MODEL_TYPES}")
    dflt = DEFAULTS[mt]
    if "hidden_size" not in d and any(k in d for k in REMOTE_CODE_KEYS):
        found = [k for k in REMOTE_CODE_KEYS if k in d]
        raise ValueError(f"{mt}: config.json carries the original remote-code keys {found} and no hidden_size: a transformers-format "
                         "config.json (hidden_size, num_hidden_layers, num_attention_heads, intermediate_size, rope_parameters) is "
                         "needed; convert the checkpoint with transformers first")

    def get(key):
        v = d.get(key)
        return dflt[key] if v is None else v

    hidden, heads = int(get("hidden_size")), int(get("num_attention_heads"))
    rp = d.get("rope_parameters") or {}
    rope_type = str(rp.get("rope_type", rp.get("type", "default")))
    if d.get("rope_scaling"):
        rope_type = str(d["rope_scaling"].get("rope_type", d["rope_scaling"].get("type", rope_type)))
    head_dim = d.get("head_dim") or (hidden // heads if heads > 0 else 0)
    act = str(get("hidden_act"))
    want_act = dflt["hidden_act"]
    bad = [f"{n}={v!r}" for n, v, ok in (("rope_type", rope_type, rope_type == "default"),
                                         ("head_dim", head_dim, head_dim == 64 and hidden == 64 * heads),
                                         ("hidden_act", act, act == want_act),
                                         ("hidden_size", hidden, hidden <= 1024 and hidden % 128 == 0)) if not ok]
    if bad:
        raise NotImplementedError(f"{mt} checkpoint with {', '.join(bad)}: the path computes default RoPE (no dynamic-NTK or other "
                                  f"scaling), head_dim 64, hidden_act {want_act!r} and hidden_size a multiple of 128 up to 1024 only")
    archs = " ".join(d.get("architectures") or [])
    if "ForSequenceClassification" in archs or "ForTokenClassification" in archs or "ForQuestionAnswering" in archs:
        raise ValueError(f"{mt}: architectures={d.get('architectures')!r}: only the embedder (the base model) is supported; a "
                         "*ForSequenceClassification head of this type is not -- no such cross-encoder is published")
    vocab = int(get("vocab_size"))
    pad = d.get("pad_token_id", dflt["pad_token_id"])
    theta = rp.get("rope_theta") or d.get("rope_theta") or dflt["rope_theta"]
    return RopeBertConfig(arch=mt, vocab_size=vocab, hidden=hidden, layers=int(get("num_hidden_layers")), heads=heads,
                          ffn=int(get("intermediate_size")), max_pos=int(get("max_position_embeddings")),
                          type_vocab=int(get("type_vocab_size")), pad_id=int(pad) if pad is not None and 0 <= int(pad) < vocab else 0,
                          ln_eps=float(get("layer_norm_eps")), num_labels=0, rope_theta=float(theta),
                          mlp="swiglu" if mt == "nomic_bert" else "gelu")


class _RbLayerW(Structure):
    """tt_ropebert_layer_weights."""
    _fields_ = [(n, c_void_p) for n in ("qkv_w", "qkv_b", "o_w", "o_b", "ln1_g", "ln1_b", "up_w", "up_b", "down_w", "down_b",
                                        "ln2_g", "ln2_b")]


class _RbW(Structure):
    """tt_ropebert_weights."""
    _fields_ = ([(n, c_int32) for n in ("hidden", "layers", "heads", "ffn", "vocab", "type_vocab", "mlp_kind")]
                + [(n, c_float) for n in ("ln_eps", "rope_theta")]
                + [(n, c_void_p) for n in ("word_emb", "type_emb", "emb_ln_g", "emb_ln_b")] + [("layer", POINTER(_RbLayerW))])


# ---- names -----------------------------------------------------------------------------------------------------------------------
# transformers/conversion_mapping.py, entries "nomic_bert" and "jina_embeddings_v3": plain substring renamings, then Wqkv chunked
# along dim 0 into q_proj, k_proj, v_proj
_RENAMES = {
    "nomic_bert": (("encoder.layers", "layers"), ("emb_ln", "embeddings.LayerNorm"), ("attn.out_proj", "self_attn.o_proj"),
                   ("fc11", "up_proj"), ("fc12", "gate_proj"), ("fc2", "down_proj"), ("norm1", "post_attention_layernorm"),
                   ("norm2", "post_mlp_layernorm")),
    "jina_embeddings_v3": (("emb_ln", "embeddings.LayerNorm"), ("encoder.layers", "layers"), ("mixer.out_proj", "self_attn.o_proj"),
                           ("norm1", "post_attention_layernorm"), ("norm2", "post_mlp_layernorm")),
}
_WQKV = {"nomic_bert": "attn.Wqkv", "jina_embeddings_v3": "mixer.Wqkv"}
_PREFIXES = ("0.auto_model.", "nomic_bert.", "jina_embeddings_v3.", "bert.", "roberta.")
# tensors that play no part: masked-LM heads (cls.* / lm_head.*), the pooler (sentence-transformers never reads it), RoPE buffers
_IGNORED = re.compile(r"^(cls\.|lm_head\.|pooler\.)|inv_freq$|^embeddings\.position_ids$|^embeddings\.token_type_ids$")


def to_transformers_names(arch: str, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``state`` under the transformers names: an optional prefix stripped, the original layout's names rewritten by the rules
    above, a fused ``Wqkv`` split into q, k, v (three equal chunks along dim 0).  A state already under those names is unchanged."""
    out: Dict[str, torch.Tensor] = {}
    for k, v in state.items():
        for pre in _PREFIXES:
            if k.startswith(pre):
                k = k[len(pre):]
                break
        for old, new in _RENAMES[arch]:
            # (a transformers name never holds an original pattern except "fc2" of Jina's own mlp.fc2, which its rules leave alone)
            k = k.replace(old, new)
        w = _WQKV[arch]
        if k.endswith((w + ".weight", w + ".bias")):
            if v.shape[0] % 3:
                raise ValueError(f"{k} {tuple(v.shape)}: a fused Wqkv holds three equal blocks of rows")
            for n, part in zip("qkv", v.chunk(3, dim=0)):
                out[k.replace(w, f"self_attn.{n}_proj")] = part
            continue
        out[k] = v
    return out


def _layer_modules(cfg: RopeBertConfig) -> List[str]:
    mlp = ["mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"] if cfg.mlp == "swiglu" else ["mlp.fc1", "mlp.fc2"]
    return [f"self_attn.{n}_proj" for n in "qkvo"] + mlp


def state_names(cfg: RopeBertConfig) -> List[str]:
    """The checkpoint tensors a model of ``cfg`` carries, under the transformers names."""
    names = ["embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight",
             "embeddings.LayerNorm.bias"]
    for i in range(cfg.layers):
        p = f"layers.{i}."
        for m in _layer_modules(cfg):
            names += [p + m + ".weight"] + ([p + m + ".bias"] if cfg.biases else [])
        for m in ("post_attention_layernorm", "post_mlp_layernorm"):
            names += [p + m + ".weight", p + m + ".bias"]
    return names


def check_config(cfg: RopeBertConfig) -> None:
    """The shapes the kernels take (tt_ropebert_forward refuses the others before a launch; say so here first)."""
    H, nh = cfg.hidden, cfg.heads
    if cfg.arch not in MODEL_TYPES:
        raise ValueError(f"ropebert: arch={cfg.arch!r} is not one of {MODEL_TYPES}")
    if H % 128 or H > 1024:
        raise NotImplementedError(f"{cfg.arch}: hidden_size={H} (a multiple of 128 up to 1024, the scan's limit)")
    if nh <= 0 or H != 64 * nh:
        raise NotImplementedError(f"{cfg.arch}: hidden_size={H} with num_attention_heads={nh}: head_dim must be 64")
    fmul = 64 if cfg.mlp == "swiglu" else 128
    if cfg.ffn <= 0 or cfg.ffn % fmul:
        raise NotImplementedError(f"{cfg.arch}: intermediate_size={cfg.ffn} (a multiple of {fmul})")
    if cfg.mlp not in ("swiglu", "gelu"):
        raise NotImplementedError(f"{cfg.arch}: mlp={cfg.mlp!r} (supported: 'swiglu', 'gelu')")
    if cfg.num_labels:
        raise NotImplementedError(f"{cfg.arch}: classification heads are not supported (embedders only)")
    if cfg.rope_theta <= 0 or cfg.type_vocab < 1:
        raise ValueError(f"{cfg.arch}: rope_theta={cfg.rope_theta} type_vocab_size={cfg.type_vocab}")


def check_state(cfg: RopeBertConfig, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``state`` under the transformers names, after checking that it holds every tensor of ``state_names(cfg)`` and nothing the
    forward would not read: the LoRA tensors of an unmerged Jina checkpoint, biases under a NomicBERT config ... are refused by
    name, not ignored.  Masked-LM heads, the pooler and RoPE buffers play no part."""
    sd = to_transformers_names(cfg.arch, state)
    names = state_names(cfg)
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"checkpoint is not a {cfg.arch} of {cfg}: missing {missing[:4]}")
    extra = sorted(k for k in set(sd) - set(names) if not _IGNORED.search(k))
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the {cfg.arch} path does not compute: {extra[:4]}")
    return sd


class RopeBertWeights(_FamilyWeights):
    """Device-resident weights for ``tt_ropebert_forward`` (bf16) or ``tt_ropebert_forward_f16`` (fp16): the projections (q, k, v
    rows concatenated to [3H][H]; SwiGLU: gate rows then up rows, [2F][H], the order ``gated_act_kernel`` reads) and the embedding
    tables in the element type; biases and LayerNorm parameters in fp32."""

    _paths, _path_name = (ROPEBERT_BF16_PATH, ROPEBERT_FP16_PATH), "the path"

    def __init__(self, cfg: RopeBertConfig, state: Dict[str, torch.Tensor], device: torch.device, dtype: torch.dtype = torch.bfloat16):
        self._begin(cfg, device, dtype)
        check_config(cfg)
        sd = check_state(cfg, state)
        mat, vec = self._loaders(sd)
        H, F = cfg.hidden, cfg.ffn

        def bias(names, n):
            return vec(names, n) if cfg.biases else None

        self._layers = (_RbLayerW * max(cfg.layers, 1))()
        for i in range(cfg.layers):
            p, L = f"layers.{i}.", self._layers[i]
            qkv = [p + f"self_attn.{n}_proj." for n in "qkv"]
            L.qkv_w, L.qkv_b = mat([m + "weight" for m in qkv], (3 * H, H)), bias([m + "bias" for m in qkv], 3 * H)
            L.o_w, L.o_b = mat([p + "self_attn.o_proj.weight"], (H, H)), bias([p + "self_attn.o_proj.bias"], H)
            L.ln1_g, L.ln1_b = vec([p + "post_attention_layernorm.weight"], H), vec([p + "post_attention_layernorm.bias"], H)
            if cfg.mlp == "swiglu":
                L.up_w, L.up_b = mat([p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight"], (2 * F, H)), None
                L.down_w, L.down_b = mat([p + "mlp.down_proj.weight"], (H, F)), None
            else:
                L.up_w, L.up_b = mat([p + "mlp.fc1.weight"], (F, H)), bias([p + "mlp.fc1.bias"], F)
                L.down_w, L.down_b = mat([p + "mlp.fc2.weight"], (H, F)), bias([p + "mlp.fc2.bias"], H)
            L.ln2_g, L.ln2_b = vec([p + "post_mlp_layernorm.weight"], H), vec([p + "post_mlp_layernorm.bias"], H)
        self.struct = _RbW(hidden=H, layers=cfg.layers, heads=cfg.heads, ffn=F, vocab=cfg.vocab_size, type_vocab=cfg.type_vocab,
                           mlp_kind=1 if cfg.mlp == "swiglu" else 0, ln_eps=cfg.ln_eps, rope_theta=cfg.rope_theta,
                           word_emb=mat(["embeddings.word_embeddings.weight"], (cfg.vocab_size, H)),
                           type_emb=mat(["embeddings.token_type_embeddings.weight"], (cfg.type_vocab, H)),
                           emb_ln_g=vec(["embeddings.LayerNorm.weight"], H), emb_ln_b=vec(["embeddings.LayerNorm.bias"], H),
                           layer=ctypes.cast(self._layers, POINTER(_RbLayerW)))


def synthetic_state(cfg: RopeBertConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random weights of ``cfg`` (fp32, CPU) under the transformers names, with trained-model-like scales: N(0, 0.02)
    projections and embeddings, LayerNorm weights around 1 (benchmarks and tests)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std=0.02):
        return torch.randn(*shape, generator=g) * std

    H, F = cfg.hidden, cfg.ffn
    sd = {"embeddings.word_embeddings.weight": rnd(cfg.vocab_size, H), "embeddings.token_type_embeddings.weight": rnd(cfg.type_vocab, H),
          "embeddings.LayerNorm.weight": 1 + rnd(H, std=0.1), "embeddings.LayerNorm.bias": rnd(H, std=0.05)}
    shapes = {"self_attn.q_proj": (H, H), "self_attn.k_proj": (H, H), "self_attn.v_proj": (H, H), "self_attn.o_proj": (H, H),
              "mlp.gate_proj": (F, H), "mlp.up_proj": (F, H), "mlp.down_proj": (H, F), "mlp.fc1": (F, H), "mlp.fc2": (H, F)}
    for i in range(cfg.layers):
        p = f"layers.{i}."
        for m in _layer_modules(cfg):
            sd[p + m + ".weight"] = rnd(*shapes[m])
            if cfg.biases:
                sd[p + m + ".bias"] = rnd(shapes[m][0])
        for m in ("post_attention_layernorm", "post_mlp_layernorm"):
            sd[p + m + ".weight"], sd[p + m + ".bias"] = 1 + rnd(H, std=0.1), rnd(H, std=0.05)
    return sd


# the published geometries (the installed config classes' defaults, which are those of nomic-embed-text-v1.5 and jina-embeddings-v3)
NOMIC_BASE = RopeBertConfig(arch="nomic_bert", vocab_size=30528, hidden=768, layers=12, heads=12, ffn=3072, max_pos=2048, type_vocab=2,
                            pad_id=0, ln_eps=1e-12, rope_theta=1000.0, mlp="swiglu")
JINA_V3 = RopeBertConfig(arch="jina_embeddings_v3", vocab_size=250002, hidden=1024, layers=24, heads=16, ffn=4096, max_pos=8194,
                         type_vocab=1, pad_id=1, ln_eps=1e-5, rope_theta=20000.0, mlp="gelu")
