"""Locating model weights for the HIP encoders.

Order of resolution (first hit wins):
  1. ``model_kwargs["state_dict"]``      -- tensors handed over directly (tests);
  2. a local model directory             -- ``model_kwargs["model_dir"]``, ``$TT_AMD_MODEL_DIR/<org>/<name>``
                                            or the HF hub cache, holding ``model.safetensors`` (or ``pytorch_model.bin``)
                                            (HF checkpoint names) + ``config.json``;
  3. ``model_kwargs["synthetic_seed"]``  -- seeded random init of the known architecture
                                            (benchmarks / parity tests; no network here).
Anything else raises, like the reference does when a model cannot be loaded
(``model_manager.py:265-272``: the caller wraps it in ``RuntimeError("Failed to load ...")``).
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Tuple

import torch

from .encoder import KNOWN_CONFIGS, EncoderConfig, synthetic_state, synthetic_state_device


WEIGHT_FILES = ("model.safetensors", "model.safetensors.index.json", "pytorch_model.bin")


def _decoder_config_from_hf(d: dict) -> EncoderConfig:
    """``model_type == "qwen3"`` (Qwen3-Embedding; a ``Qwen3ForSequenceClassification`` reranker): every size from config.json,
    nothing assumed.  A head exists iff ``architectures`` names a ``*ForSequenceClassification`` (what the reference's loader,
    ``AutoModelForSequenceClassification``, instantiates with trained weights); ``pad_token_id`` decides which token it reads."""
    from .decoder import DecoderConfig

    # variants the decoder kernels do not compute are refused, never run as plain Qwen3 (no silent wrong vectors)
    rope = d.get("rope_scaling") or d.get("rope_parameters") or {}     # transformers 4.x / 5.x spelling
    rope_type = rope.get("rope_type", rope.get("type", "default"))
    layer_types = sorted(set(d.get("layer_types") or ["full_attention"]))
    bad = [f"{n}={v!r}" for n, v, ok in (
        ("attention_bias", d.get("attention_bias", False), not d.get("attention_bias", False)),
        ("rope_type", rope_type, rope_type == "default"),
        ("use_sliding_window", d.get("use_sliding_window", False), not d.get("use_sliding_window", False)),
        ("layer_types", layer_types, layer_types == ["full_attention"]),
        ("hidden_act", d.get("hidden_act", "silu"), d.get("hidden_act", "silu") == "silu")) if not ok]
    if bad:
        raise NotImplementedError(f"qwen3 checkpoint with {', '.join(bad)}: the decoder embedder computes bias-free full causal "
                                  "attention with default RoPE and SiLU only")
    heads = d["num_attention_heads"]
    num_labels = 0
    if "ForSequenceClassification" in " ".join(d.get("architectures") or []):
        n = d.get("num_labels") or (len(d["id2label"]) if d.get("id2label") else 1)
        if n != 1:
            raise ValueError(f"qwen3 classification checkpoint with {n} labels: only single-label (sigmoid) cross-encoder heads "
                             "are supported")
        num_labels = 1
    pad = d.get("pad_token_id")
    return DecoderConfig(
        arch="qwen3", vocab_size=d["vocab_size"], hidden=d["hidden_size"], layers=d["num_hidden_layers"], heads=heads,
        ffn=d["intermediate_size"], max_pos=d["max_position_embeddings"], type_vocab=1, pad_id=0,
        ln_eps=d.get("rms_norm_eps", 1e-6), num_labels=num_labels, pad_token_id=None if pad is None else int(pad), kv_heads=d.get("num_key_value_heads") or heads,
        head_dim=d.get("head_dim") or 128,   # Qwen3Config's default (not hidden // heads)
        rope_theta=float(d.get("rope_theta") or (d.get("rope_parameters") or {}).get("rope_theta") or 10000.0))


def _modernbert_config_from_hf(d: dict) -> EncoderConfig:
    """``model_type == "modernbert"`` (gte-modernbert, nomic modernbert-embed, gte-reranker-modernbert, the answerdotai/ModernBERT
    fine-tunes): every size from config.json.  ``layer_types`` is read; derived from ``global_attn_every_n_layers`` only where an
    older export does not carry it, like the two RoPE bases (``rope_parameters``, else ``global_rope_theta`` /
    ``local_rope_theta``).  A head exists iff ``architectures`` names a ``*ForSequenceClassification``."""
    from .modernbert import ModernBertConfig, default_layer_types

    layers = d["num_hidden_layers"]
    layer_types = d.get("layer_types")
    if not layer_types:
        layer_types = default_layer_types(layers, int(d.get("global_attn_every_n_layers", 3)))
    rp = d.get("rope_parameters") or {}
    g, loc = rp.get("full_attention") or {}, rp.get("sliding_attention") or {}
    rope_types = sorted({str(x.get("rope_type", x.get("type", "default"))) for x in (g, loc, d.get("rope_scaling") or {})})
    glu = d.get("hidden_activation", "gelu")
    cact = d.get("classifier_activation", "gelu")
    # variants the ModernBERT kernels do not compute are refused by field name, never run as the plain model
    bad = [f"{n}={v!r}" for n, v, ok in (
        ("attention_bias", d.get("attention_bias", False), not d.get("attention_bias", False)),
        ("mlp_bias", d.get("mlp_bias", False), not d.get("mlp_bias", False)),
        ("norm_bias", d.get("norm_bias", False), not d.get("norm_bias", False)),
        ("classifier_bias", d.get("classifier_bias", False), not d.get("classifier_bias", False)),
        ("rope_type", rope_types, rope_types == ["default"]),
        ("hidden_activation", glu, glu == "gelu"),
        ("classifier_activation", cact, cact == "gelu")) if not ok]
    if bad:
        raise NotImplementedError(f"modernbert checkpoint with {', '.join(bad)}: the ModernBERT path computes bias-free layers "
                                  "with default RoPE and exact-erf GELU only")
    num_labels = 0
    if "ForSequenceClassification" in " ".join(d.get("architectures") or []):
        n = d.get("num_labels") or (len(d["id2label"]) if d.get("id2label") else 1)
        if n != 1:
            raise NotImplementedError(f"modernbert classification checkpoint with num_labels={n}: only single-label (sigmoid) "
                                      "cross-encoder heads are supported")
        num_labels = 1
    pad = d.get("pad_token_id")
    vocab = d["vocab_size"]
    return ModernBertConfig(
        arch="modernbert", vocab_size=vocab, hidden=d["hidden_size"], layers=layers, heads=d["num_attention_heads"],
        ffn=d["intermediate_size"], max_pos=d["max_position_embeddings"], type_vocab=1,
        pad_id=int(pad) if pad is not None and 0 <= int(pad) < vocab else 0, ln_eps=d.get("norm_eps", 1e-5), num_labels=num_labels,
        layer_types=tuple(layer_types),
        global_rope_theta=float(g.get("rope_theta") or d.get("global_rope_theta") or 160000.0),
        local_rope_theta=float(loc.get("rope_theta") or d.get("local_rope_theta") or d.get("global_rope_theta") or 10000.0),
        local_attention=int(d.get("local_attention", 128)), classifier_pooling=str(d.get("classifier_pooling", "cls")))


def _gemma_config_from_hf(d: dict) -> EncoderConfig:
    """``model_type == "gemma3_text"`` with ``use_bidirectional_attention`` (google/embeddinggemma-300m): every size from
    config.json.  ``layer_types`` is read; derived from ``sliding_window_pattern`` only where an older export does not carry it,
    like the two RoPE bases (``rope_parameters``, else ``rope_theta`` / ``rope_local_base_freq``).  The window the kernels compare
    with is ``sliding_window // 2``: transformers rewrites a bidirectional config's S to ``S // 2 + 1`` on load and masks with
    ``|q - k| <`` that value."""
    from .gemma import LAYER_KINDS, GemmaConfig, default_layer_types

    layers = d["num_hidden_layers"]
    layer_types = d.get("layer_types") or default_layer_types(layers, int(d.get("sliding_window_pattern", 6)))
    rp = d.get("rope_parameters") or {}
    g, loc = rp.get("full_attention") or {}, rp.get("sliding_attention") or {}
    rope_types = sorted({str(x.get("rope_type", x.get("type", "default"))) for x in (g, loc, d.get("rope_scaling") or {})})
    head_dim = d.get("head_dim") or 256     # Gemma3TextConfig's default (not hidden // heads)
    act = d.get("hidden_activation", "gelu_pytorch_tanh")
    qpas = d.get("query_pre_attn_scalar", 256)
    kinds = sorted(set(layer_types))
    # variants the EmbeddingGemma kernels do not compute are refused by field name, never run as the plain model
    bad = [f"{n}={v!r}" for n, v, ok in (
        ("use_bidirectional_attention", d.get("use_bidirectional_attention"), d.get("use_bidirectional_attention") is True),
        ("attn_logit_softcapping", d.get("attn_logit_softcapping"), d.get("attn_logit_softcapping") is None),
        ("attention_bias", d.get("attention_bias", False), not d.get("attention_bias", False)),
        ("hidden_activation", act, act == "gelu_pytorch_tanh"),
        ("rope_type", rope_types, rope_types == ["default"]),
        ("query_pre_attn_scalar", qpas, qpas == head_dim),
        ("layer_types", kinds, not set(kinds) - set(LAYER_KINDS))) if not ok]
    if bad:
        raise NotImplementedError(f"gemma3_text checkpoint with {', '.join(bad)}: the EmbeddingGemma path computes the bias-free "
                                  "bidirectional text encoder with default RoPE, GELU_tanh and a 1 / sqrt(head_dim) score scale "
                                  "only (use_bidirectional_attention false or absent is a causal language model)")
    if "ForSequenceClassification" in " ".join(d.get("architectures") or []):
        raise NotImplementedError("gemma3_text classification checkpoints are not supported (architectures names a "
                                  "*ForSequenceClassification)")
    heads = d["num_attention_heads"]
    pad = d.get("pad_token_id")
    vocab = d["vocab_size"]
    return GemmaConfig(
        arch="gemma3_text", vocab_size=vocab, hidden=d["hidden_size"], layers=layers, heads=heads, ffn=d["intermediate_size"],
        max_pos=d["max_position_embeddings"], type_vocab=1, pad_id=int(pad) if pad is not None and 0 <= int(pad) < vocab else 0,
        ln_eps=d.get("rms_norm_eps", 1e-6), num_labels=0, kv_heads=d.get("num_key_value_heads") or heads, head_dim=head_dim,
        layer_types=tuple(layer_types),
        global_rope_theta=float(g.get("rope_theta") or d.get("rope_theta") or 1e6),
        local_rope_theta=float(loc.get("rope_theta") or d.get("rope_local_base_freq") or 1e4),
        window=int(d.get("sliding_window", 4096)) // 2)


def _mpnet_config_from_hf(d: dict) -> EncoderConfig:
    """``model_type == "mpnet"`` (sentence-transformers/all-mpnet-base-v2, multi-qa-mpnet-base-*): every size from config.json.
    The bucket function's 32 buckets and max_distance 128 are hard-coded in transformers; ``relative_attention_num_buckets`` only
    sizes the table, and any other size is refused by name.  Embedders only: a ``*ForSequenceClassification`` is refused."""
    from .mpnet import NUM_BUCKETS

    nb = d.get("relative_attention_num_buckets", NUM_BUCKETS)
    act = d.get("hidden_act", "gelu")
    bad = [f"{n}={v!r}" for n, v, ok in (("relative_attention_num_buckets", nb, nb == NUM_BUCKETS),
                                         ("hidden_act", act, act == "gelu")) if not ok]
    if bad:
        raise NotImplementedError(f"mpnet checkpoint with {', '.join(bad)}: the MPNet path computes the {NUM_BUCKETS}-bucket "
                                  "relative-position bias and exact-erf GELU only")
    archs = " ".join(d.get("architectures") or [])
    if "ForSequenceClassification" in archs:
        raise NotImplementedError(f"mpnet classification checkpoints are not supported (architectures={d.get('architectures')!r} "
                                  "names a *ForSequenceClassification): MPNet cross-encoders are out of scope")
    pad = d.get("pad_token_id", 1)
    return EncoderConfig(
        arch="mpnet", vocab_size=d["vocab_size"], hidden=d["hidden_size"], layers=d["num_hidden_layers"],
        heads=d["num_attention_heads"], ffn=d["intermediate_size"], max_pos=d["max_position_embeddings"], type_vocab=1,
        pad_id=1 if pad is None else int(pad), ln_eps=d.get("layer_norm_eps", 1e-12), num_labels=0)


def _deberta_config_from_hf(d: dict) -> EncoderConfig:
    """``model_type == "deberta-v2"`` (DebertaV2ForSequenceClassification: mixedbread-ai/mxbai-rerank-*-v1, the deberta-v3 checkpoints
    under cross-encoder/, fine-tunes of microsoft/deberta-v3-*): every size from config.json.  The kernels compute the v3 form of the
    disentangled attention -- c2p + p2c with shared projections, log buckets, normalised relative embeddings, no absolute positions,
    no token types, no convolution; every other variant of the architecture is refused by field name, never run as that form."""
    from .deberta import DebertaConfig

    pat = d.get("pos_att_type")
    if isinstance(pat, str):
        pat = [x.strip() for x in pat.lower().split("|") if x.strip()]
    pat = sorted(str(x).lower() for x in (pat or []))
    hidden, heads = d["hidden_size"], d["num_attention_heads"]
    max_pos = d["max_position_embeddings"]
    mrp = d.get("max_relative_positions", -1)
    mrp = max_pos if mrp is None or mrp < 1 else int(mrp)
    buckets = d.get("position_buckets", -1)
    norm = str(d.get("norm_rel_ebd", "none")).lower()
    emb = d.get("embedding_size") or hidden
    pool = d.get("pooler_hidden_size") or hidden
    act, pact = d.get("hidden_act", "gelu"), d.get("pooler_hidden_act", "gelu")
    bad = [f"{n}={v!r}" for n, v, ok in (
        ("relative_attention", d.get("relative_attention", False), d.get("relative_attention", False) is True),
        ("pos_att_type", d.get("pos_att_type"), pat == ["c2p", "p2c"]),
        ("share_att_key", d.get("share_att_key", False), d.get("share_att_key", False) is True),
        ("norm_rel_ebd", d.get("norm_rel_ebd", "none"), norm == "layer_norm"),
        ("position_biased_input", d.get("position_biased_input", True), d.get("position_biased_input", True) is False),
        ("type_vocab_size", d.get("type_vocab_size", 0), not d.get("type_vocab_size", 0)),
        ("conv_kernel_size", d.get("conv_kernel_size", 0), not (d.get("conv_kernel_size") or 0) > 0),
        ("embedding_size", emb, emb == hidden),
        ("pooler_hidden_size", pool, pool == hidden),
        ("pooler_hidden_act", pact, pact == "gelu"),
        ("hidden_act", act, act == "gelu"),
        ("position_buckets", buckets, isinstance(buckets, int) and buckets > 0),
        ("max_relative_positions", d.get("max_relative_positions", -1), mrp <= max_pos)) if not ok]
    if bad:
        raise NotImplementedError(f"deberta-v2 checkpoint with {', '.join(bad)}: the DeBERTa path computes the v3 disentangled "
                                  "attention only (relative_attention with pos_att_type c2p|p2c, share_att_key, norm_rel_ebd "
                                  "layer_norm, position_buckets > 0, no position_biased_input, no token types, no convolution, "
                                  "exact-erf GELU)")
    if heads <= 0 or hidden != 64 * heads or hidden % 128 or hidden > 1024:
        raise NotImplementedError(f"deberta-v2 checkpoint with hidden_size={hidden}, num_attention_heads={heads}: head_dim must be 64 "
                                  "and hidden_size a multiple of 128 up to 1024")
    num_labels = 0
    if "ForSequenceClassification" in " ".join(d.get("architectures") or []):
        n = d.get("num_labels") or (len(d["id2label"]) if d.get("id2label") else 1)
        if n != 1:
            raise NotImplementedError(f"deberta-v2 classification checkpoint with num_labels={n}: only single-label (sigmoid) "
                                      "cross-encoder heads are supported")
        num_labels = 1
    pad = d.get("pad_token_id", 0)
    vocab = d["vocab_size"]
    return DebertaConfig(
        arch="deberta-v2", vocab_size=vocab, hidden=hidden, layers=d["num_hidden_layers"], heads=heads, ffn=d["intermediate_size"],
        max_pos=max_pos, type_vocab=1, pad_id=int(pad) if pad is not None and 0 <= int(pad) < vocab else 0,
        ln_eps=d.get("layer_norm_eps", 1e-7), num_labels=num_labels, position_buckets=int(buckets), max_relative_positions=mrp)


def _config_from_hf(d: dict, num_labels_default: int = 0) -> EncoderConfig:
    mt = d.get("model_type", "xlm-roberta")
    if mt == "mpnet":
        return _mpnet_config_from_hf(d)
    if mt == "deberta-v2":
        return _deberta_config_from_hf(d)
    if mt == "gemma3_text":
        return _gemma_config_from_hf(d)
    if mt == "qwen3":
        return _decoder_config_from_hf(d)
    if mt == "modernbert":
        return _modernbert_config_from_hf(d)
    if mt in ("nomic_bert", "jina_embeddings_v3"):
        from .ropebert import config_from_hf as ropebert_config_from_hf

        return ropebert_config_from_hf(d)
    if mt == "t5":
        from .t5 import config_from_hf as t5_config_from_hf

        return t5_config_from_hf(d)
    if mt == "umt5":
        raise NotImplementedError("umt5 checkpoints carry a relative-position bias table in every block (the T5 path adds block "
                                  "0's table in every block): not supported")
    if mt == "bert" and d.get("position_embedding_type") == "alibi":
        # JinaBERT (jina-embeddings-v2): a remote-code architecture whose config.json says "bert"
        from .jinabert import config_from_hf as jinabert_config_from_hf

        return jinabert_config_from_hf(d)
    arch = "bert" if mt == "bert" else "xlmr"
    archs = " ".join(d.get("architectures", []))
    num_labels = 1 if "SequenceClassification" in archs else num_labels_default
    return EncoderConfig(
        arch=arch, vocab_size=d["vocab_size"], hidden=d["hidden_size"], layers=d["num_hidden_layers"],
        heads=d["num_attention_heads"], ffn=d["intermediate_size"], max_pos=d["max_position_embeddings"],
        type_vocab=d.get("type_vocab_size", 1), pad_id=d.get("pad_token_id", 1 if arch == "xlmr" else 0),
        ln_eps=d.get("layer_norm_eps", 1e-5), num_labels=num_labels)


def head_activation(model_name: str, model_dir: Optional[str], model_kwargs: Optional[dict]) -> str:
    """What ``CrossEncoder.predict`` applies to a single-label head's logit ([UPSTREAM-K], sentence-transformers): the
    activation named in the checkpoint's config.json (``sbert_ce_default_activation_function``, or
    ``sentence_transformers.activation_fn`` in newer exports), else Sigmoid.  The BGE rerankers carry none (sigmoid
    scores in (0, 1)); the ``cross-encoder/ms-marco-*`` checkpoints name ``torch.nn.modules.linear.Identity`` and are
    scored by their raw logits.  ``model_kwargs["activation"]`` ("sigmoid" / "identity") overrides."""
    mk = model_kwargs or {}
    if mk.get("activation"):
        act = str(mk["activation"]).lower()
        if act not in ("sigmoid", "identity"):
            raise ValueError("model_kwargs['activation'] must be 'sigmoid' or 'identity'")
        return act
    name = None
    if model_dir and os.path.exists(os.path.join(model_dir, "config.json")):
        with open(os.path.join(model_dir, "config.json")) as f:
            d = json.load(f)
        name = d.get("sbert_ce_default_activation_function") or (d.get("sentence_transformers") or {}).get("activation_fn")
    elif model_name.startswith("cross-encoder/ms-marco-"):
        name = "torch.nn.modules.linear.Identity"      # synthetic weights under the real name: the real checkpoint's setting
    if name is None:
        return "sigmoid"
    tail = str(name).rsplit(".", 1)[-1].lower()
    if tail == "identity":
        return "identity"
    if tail == "sigmoid":
        return "sigmoid"
    raise ValueError(f"cross-encoder activation '{name}' is not supported (Sigmoid or Identity)")


def pooling_mode(model_dir: Optional[str], default: str = "cls") -> str:
    """The sentence-transformers pooling a checkpoint directory declares (``1_Pooling/config.json``): "cls", "mean", "last"
    (``pooling_mode_lasttoken``: the decoder embedders), ... ;
    ``default`` when the directory declares nothing: "cls" for encoders (the BGE models the reference defaults to are CLS +
    Normalize), "last" for decoder embedders (their first token has seen only itself)."""
    if not model_dir:
        return default
    pc = os.path.join(model_dir, "1_Pooling", "config.json")
    if not os.path.exists(pc):
        return default
    with open(pc) as f:
        d = json.load(f)
    on = [k[len("pooling_mode_"):] for k, v in d.items() if k.startswith("pooling_mode_") and v is True]
    if on == ["cls_token"]:
        return "cls"
    if on == ["lasttoken"]:
        return "last"
    return "+".join(sorted(on)) or "none"


def find_model_dir(model_name: str, model_kwargs: Optional[dict]) -> Optional[str]:
    mk = model_kwargs or {}
    cands = []
    if mk.get("model_dir"):
        cands.append(mk["model_dir"])
    if os.path.isdir(model_name):
        cands.append(model_name)
    root = os.environ.get("TT_AMD_MODEL_DIR")
    if root:
        cands += [os.path.join(root, model_name), os.path.join(root, model_name.split("/")[-1])]
    for c in cands:
        if any(os.path.exists(os.path.join(c, f)) for f in WEIGHT_FILES):
            return c
    try:  # HF hub cache, offline
        from huggingface_hub import try_to_load_from_cache

        for f in WEIGHT_FILES:
            p = try_to_load_from_cache(model_name, f)
            if isinstance(p, str) and os.path.exists(p):
                return os.path.dirname(p)
    except Exception:  # noqa: BLE001
        pass
    return None


def load_state(model_dir: str) -> Dict[str, torch.Tensor]:
    """``model.safetensors`` if present, else the shards ``model.safetensors.index.json`` names, else the older
    ``pytorch_model.bin`` (tensors only, ``weights_only=True``)."""
    st = os.path.join(model_dir, "model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file

        return load_file(st)
    idx = os.path.join(model_dir, "model.safetensors.index.json")
    if os.path.exists(idx):
        from safetensors.torch import load_file

        with open(idx) as f:
            shards = sorted(set(json.load(f)["weight_map"].values()))
        out: Dict[str, torch.Tensor] = {}
        for sh in shards:
            out.update(load_file(os.path.join(model_dir, sh)))
        return out
    return torch.load(os.path.join(model_dir, "pytorch_model.bin"), map_location="cpu", weights_only=True)


def resolve(model_name: str, model_kwargs: Optional[dict], device: torch.device,
            want_head: bool) -> Tuple[EncoderConfig, Dict[str, torch.Tensor], Optional[str]]:
    """-> (config, state dict, model_dir or None)."""
    mk = model_kwargs or {}
    cfg = mk.get("encoder_config") or KNOWN_CONFIGS.get(model_name)
    if cfg is None:
        from .mpnet import KNOWN_CONFIGS as mpnet_configs

        cfg = mpnet_configs.get(model_name)
    if cfg is None:
        from .deberta import KNOWN_CONFIGS as deberta_configs

        cfg = deberta_configs.get(model_name)
    if cfg is None:
        from .t5 import KNOWN_CONFIGS as t5_configs

        cfg = t5_configs.get(model_name)
    if "state_dict" in mk:
        if cfg is None:
            raise ValueError(f"no architecture known for '{model_name}': pass model_kwargs['encoder_config']")
        return cfg, mk["state_dict"], None
    mdir = find_model_dir(model_name, mk)
    if mdir is not None:
        with open(os.path.join(mdir, "config.json")) as f:
            cfg = _config_from_hf(json.load(f), 1 if want_head else 0)
        if want_head and cfg.arch in ("nomic_bert", "jina_embeddings_v3"):
            # (HipSentenceTransformerRerank's loader: refused before the weights are read)
            raise ValueError(f"'{model_name}': {cfg.arch} checkpoints are served as embedders only (HipHuggingFaceEmbedding); "
                             "a *ForSequenceClassification head of this type is not supported -- no such cross-encoder is published")
        if want_head and cfg.arch == "jina_bert":
            raise ValueError(f"'{model_name}': jina_bert checkpoints are served as embedders only (HipHuggingFaceEmbedding); "
                             "a *ForSequenceClassification head of this type is not supported (jina-reranker-v1 has 32-wide heads)")
        if want_head and cfg.arch == "t5":
            raise ValueError(f"'{model_name}': t5 checkpoints are served as embedders only (HipHuggingFaceEmbedding); a T5 "
                             "cross-encoder is not supported")
        state = load_state(mdir)
        if cfg.arch == "t5":
            from .t5 import dense_module

            state.update(dense_module(mdir))       # the sentence-transformers Dense module, where the directory has one
        if cfg.arch == "gemma3_text" and not want_head:
            from .gemma import dense_modules

            state.update(dense_modules(mdir))      # the sentence-transformers Dense pair lives beside the transformer's tensors
        return cfg, state, mdir
    if "synthetic_seed" in mk:
        if cfg is None:
            raise ValueError(f"no architecture known for '{model_name}': pass model_kwargs['encoder_config']")
        seed = int(mk["synthetic_seed"])
        if cfg.arch == "qwen3":
            from .decoder import synthetic_state as decoder_state

            return cfg, decoder_state(cfg, seed), None
        if cfg.arch == "modernbert":
            from .modernbert import synthetic_state as modernbert_state

            return cfg, modernbert_state(cfg, seed), None
        if cfg.arch == "gemma3_text":
            from .gemma import synthetic_state as gemma_state

            return cfg, gemma_state(cfg, seed), None
        if cfg.arch == "mpnet":
            from .mpnet import synthetic_state as mpnet_state

            return cfg, mpnet_state(cfg, seed), None
        if cfg.arch == "deberta-v2":
            from .deberta import synthetic_state as deberta_state

            return cfg, deberta_state(cfg, seed), None
        if cfg.arch in ("nomic_bert", "jina_embeddings_v3"):
            from .ropebert import synthetic_state as ropebert_state

            return cfg, ropebert_state(cfg, seed), None
        if cfg.arch == "jina_bert":
            from .jinabert import synthetic_state as jinabert_state

            return cfg, jinabert_state(cfg, seed), None
        if cfg.arch == "t5":
            from .t5 import synthetic_state as t5_state

            return cfg, t5_state(cfg, seed), None
        if mk.get("synthetic_on_device", cfg.layers * cfg.hidden >= 12 * 768):
            return cfg, synthetic_state_device(cfg, device, seed), None
        return cfg, synthetic_state(cfg, seed), None
    raise FileNotFoundError(
        f"weights for '{model_name}' not found: no model.safetensors under model_kwargs['model_dir'], "
        f"$TT_AMD_MODEL_DIR or the HF cache, and this environment has no network. "
        f"(Benchmarks/tests: pass model_kwargs={{'synthetic_seed': N}}.)")


def prompts(model_dir: Optional[str]) -> Dict[str, str]:
    """The sentence-transformers ``prompts`` a checkpoint directory declares (``config_sentence_transformers.json``), e.g. the
    Qwen3-Embedding instruction under "query" and "" under "document"; {} when it declares none."""
    if not model_dir:
        return {}
    pc = os.path.join(model_dir, "config_sentence_transformers.json")
    if not os.path.exists(pc):
        return {}
    with open(pc) as f:
        d = json.load(f)
    return {str(k): str(v) for k, v in (d.get("prompts") or {}).items()}
