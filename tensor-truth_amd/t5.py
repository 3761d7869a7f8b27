"""T5 encoders on the HIP path: embedders (``T5EncoderModel``: sentence-transformers/sentence-t5-base / -large, gtr-t5-base /
-large, hkunlp/instructor-base / -large), weights in the layout of ``tt_t5_weights`` (include/tt_hip.h), driven by the one host-side
``encoder.Encoder`` through the ``T5_BF16_PATH`` record.

The reference hands whatever Hugging Face name its config holds to ``HuggingFaceEmbedding`` (``services/model_manager.py:188-272``).
The arithmetic is ``transformers/models/t5/modeling_t5.py``'s, restated in include/tt_hip.h: pre-norm blocks without biases, a
``T5LayerNorm`` (no mean subtraction, fp32 statistics, rounded to the element type before the weight multiplies), attention scores
that are NOT divided by sqrt(d_kv), and a learned relative-position bias ``[32 buckets][heads]`` that lives in block 0 and is added
in every block.  ``T5Attention._relative_position_bucket`` (32 buckets, max_distance 128, bidirectional, key - query) is the
function MPNet copied: the per-head table over the clamped distance is ``mpnet.distance_table`` of block 0's tensor, and the
attention kernel is MPNet's, unchanged -- it computes q . k / 8 + table, so the q rows of the fused projection are stored times 8
here (an exponent shift: exact in bf16).  There are no positions and no token types; the tokenizer ends a sequence with ``</s>``
and pads with id 0.  The sentence-transformers modules behind the transformer -- ``Pooling`` (mean), an optional bias-free
``Dense`` with the identity activation, ``Normalize`` -- are read from the checkpoint directory (``dense_module``) and run in fp32
(``tt_t5_pool_dense``).  Precision: bf16 only.  T5's FFN activations leave fp16's range (transformers' own fp16 run clamps them,
which is another model), and the reference-precision default of the XLM-R / BERT family has no implementation here
(``precision.build_encoder``).
"""
from __future__ import annotations

import ctypes
import json
import os
from ctypes import POINTER, Structure, c_float, c_int32, c_void_p
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .encoder import T5_BF16_PATH, EncoderConfig, _FamilyWeights
from .mpnet import MAX_DISTANCE, NUM_BUCKETS, distance_table

MLP_KINDS = {"relu": 0, "gated-gelu": 1}     # feed_forward_proj -> tt_t5_weights.mlp_kind
MAX_TOKENS = 512                             # sequences stay within the relative-bias attention's range, as for MPNet
DENSE_NAME = "dense.weight"                  # the sentence-transformers Dense module travels in the state dict under this name


@dataclass(frozen=True)
class T5Config(EncoderConfig):
    """The ``EncoderConfig`` fields (``hidden`` = ``d_model``, ``ffn`` = ``d_ff``, ``ln_eps`` = ``layer_norm_epsilon``, ``max_pos`` =
    the longest sequence; ``pad_id`` = the filler ``pack_tokens`` writes into rows of no sequence) plus what only T5 names."""

    arch: str = "t5"
    d_kv: int = 64
    mlp_kind: int = 0            # 0: relu; 1: gated-gelu (gelu_new)
    num_buckets: int = NUM_BUCKETS
    max_distance: int = MAX_DISTANCE


class _T5LayerW(Structure):
    """tt_t5_layer_weights."""
    _fields_ = [(n, c_void_p) for n in ("ln_attn", "qkv_w", "o_w", "ln_ffn", "wi", "wo")]


class _T5W(Structure):
    """tt_t5_weights."""
    _fields_ = ([(n, c_int32) for n in ("d_model", "layers", "heads", "d_kv", "d_ff", "vocab", "mlp_kind", "num_buckets",
                                        "max_distance")]
                + [("eps", c_float), ("embed", c_void_p), ("layer", POINTER(_T5LayerW)), ("final_norm", c_void_p),
                   ("rel_bias", c_void_p), ("bias_table", c_void_p), ("dense_out", c_int32), ("dense_wt", c_void_p)])


def config_from_hf(d: dict) -> T5Config:
    """``model_type == "t5"`` with a ``T5EncoderModel``: every size from config.json.  Variants the T5 kernels do not compute are
    refused by field name, never run as the plain encoder."""
    ffp = d.get("feed_forward_proj", "relu")
    nb = d.get("relative_attention_num_buckets", NUM_BUCKETS)
    md = d.get("relative_attention_max_distance", MAX_DISTANCE)
    bad = [f"{n}={v!r}" for n, v, ok in (
        ("feed_forward_proj", ffp, ffp in MLP_KINDS),
        ("is_decoder", d.get("is_decoder", False), not d.get("is_decoder", False)),
        ("relative_attention_num_buckets", nb, nb == NUM_BUCKETS),
        ("relative_attention_max_distance", md, md == MAX_DISTANCE)) if not ok]
    if bad:
        raise NotImplementedError(f"t5 checkpoint with {', '.join(bad)}: the T5 path computes the encoder stack with the "
                                  f"{NUM_BUCKETS}-bucket, max-distance-{MAX_DISTANCE} relative-position bias and a relu or "
                                  "gated-gelu MLP only")
    archs = " ".join(d.get("architectures") or [])
    if "ForSequenceClassification" in archs or "ForTokenClassification" in archs or "ForQuestionAnswering" in archs:
        raise NotImplementedError(f"t5 classification checkpoints are not supported (architectures={d.get('architectures')!r}): "
                                  "T5 encoders are served as embedders only")
    pad = d.get("pad_token_id", 0)
    vocab = d["vocab_size"]
    return T5Config(arch="t5", vocab_size=vocab, hidden=d["d_model"], layers=d["num_layers"], heads=d["num_heads"], ffn=d["d_ff"],
                    max_pos=MAX_TOKENS, type_vocab=1, pad_id=int(pad) if pad is not None and 0 <= int(pad) < vocab else 0,
                    ln_eps=d.get("layer_norm_epsilon", 1e-6), num_labels=0, d_kv=d.get("d_kv", 64), mlp_kind=MLP_KINDS[ffp],
                    num_buckets=nb, max_distance=md)


def check_config(cfg: T5Config) -> None:
    """The shapes the T5 kernels take (tt_t5_forward refuses the others before a launch; say so here first)."""
    H, nh = cfg.hidden, cfg.heads
    if H <= 0 or H % 128 or H > 1024:
        raise NotImplementedError(f"t5: d_model={H} (a multiple of 128 up to 1024, the scan's limit)")
    if cfg.d_kv != 64 or nh <= 0 or nh * 64 != H:
        raise NotImplementedError(f"t5: d_kv={cfg.d_kv} with num_heads={nh} and d_model={H}: d_kv must be 64 and num_heads * 64 = "
                                  "d_model")
    if cfg.ffn <= 0 or cfg.ffn % 128:
        raise NotImplementedError(f"t5: d_ff={cfg.ffn} (a multiple of 128)")
    if cfg.num_buckets != NUM_BUCKETS:
        raise NotImplementedError(f"t5: relative_attention_num_buckets={cfg.num_buckets} (supported: {NUM_BUCKETS})")
    if cfg.max_distance != MAX_DISTANCE:
        raise NotImplementedError(f"t5: relative_attention_max_distance={cfg.max_distance} (supported: {MAX_DISTANCE})")
    if cfg.mlp_kind not in (0, 1):
        raise NotImplementedError(f"t5: mlp_kind={cfg.mlp_kind} (0: relu, 1: gated-gelu)")
    if cfg.num_labels:
        raise NotImplementedError("t5: classification heads are not supported (embedders only)")


_REL_BIAS = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
_EMBED = "shared.weight"
# tied copies of the embedding table, as a T5EncoderModel (or a checkpoint cut out of the full model) may store them
_EMBED_ALIASES = ("encoder.embed_tokens.weight",)


def state_names(cfg: T5Config) -> List[str]:
    """The checkpoint tensors a ``T5EncoderModel`` of ``cfg`` carries, under their canonical names (``check_state``)."""
    names = [_EMBED, _REL_BIAS]
    wi = ("wi_0", "wi_1") if cfg.mlp_kind == 1 else ("wi",)
    for i in range(cfg.layers):
        p = f"encoder.block.{i}."
        names += [p + f"layer.0.SelfAttention.{n}.weight" for n in "qkvo"] + [p + "layer.0.layer_norm.weight"]
        names += [p + f"layer.1.DenseReluDense.{n}.weight" for n in wi + ("wo",)] + [p + "layer.1.layer_norm.weight"]
    return names + ["encoder.final_layer_norm.weight"]


def _canonical(state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Names without the sentence-transformers ``0.auto_model.`` prefix; a bare encoder stack (``block.0...``, ``embed_tokens``,
    ``final_layer_norm``: a saved ``T5Stack``) gets its ``encoder.`` back."""
    out = {}
    for k, v in state.items():
        if k.startswith("0.auto_model."):
            k = k[len("0.auto_model."):]
        if k.startswith(("block.", "final_layer_norm.", "embed_tokens.")):
            k = "encoder." + k
        out[k] = v
    return out


def check_state(cfg: T5Config, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """``state`` under canonical names, after checking that it holds every tensor of ``state_names(cfg)`` and nothing the forward
    would not read.  A decoder stack, an ``lm_head``, a classifier or a bias table in a block other than 0 (umt5) mean another
    model and are refused by name, not ignored.  ``encoder.embed_tokens.weight`` is the tied copy of ``shared.weight`` (either may
    be the one that is stored); the Dense module (``DENSE_NAME``) is optional."""
    sd = _canonical(state)
    if _EMBED not in sd:
        for alias in _EMBED_ALIASES:
            if alias in sd:
                sd[_EMBED] = sd[alias]
                break
    for what, hit in (("a decoder stack", lambda k: k.startswith("decoder.")), ("a language-model head", lambda k: k.startswith("lm_head")),
                      ("a classifier", lambda k: k.startswith(("classifier", "classification_head", "qa_outputs"))),
                      ("a relative-position bias table in a block other than 0 (umt5's per-layer tables)",
                       lambda k: k.endswith("relative_attention_bias.weight") and k != _REL_BIAS)):
        found = sorted(k for k in sd if hit(k))
        if found:
            raise NotImplementedError(f"checkpoint carries {what}: {found[:4]}; the T5 path computes the encoder stack of a "
                                      "T5EncoderModel only")
    names = state_names(cfg)
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"checkpoint is not a T5 encoder of {cfg}: missing {missing[:4]}")
    extra = sorted(set(sd) - set(names) - set(_EMBED_ALIASES) - {DENSE_NAME})
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the T5 path does not compute: {extra[:4]}")
    return sd


def _pooling_config(model_dir: str, mods: List[dict]) -> dict:
    with open(os.path.join(model_dir, mods[1]["path"], "config.json")) as f:
        return json.load(f)


def dense_module(model_dir: str) -> Dict[str, torch.Tensor]:
    """The sentence-transformers tail a checkpoint directory declares (``modules.json``), which must be Transformer -> Pooling
    (mean) [-> Dense] -> Normalize: -> {``DENSE_NAME``: the Dense module's ``linear.weight``}, or {} when there is none.  Anything
    else -- another pooling, a Dense module with a bias or an activation other than the identity, a missing Normalize -- is
    refused by name: no kernel here computes it.  A directory without modules.json is the bare transformer: {}."""
    from safetensors.torch import load_file

    mj = os.path.join(model_dir, "modules.json")
    if not os.path.exists(mj):
        return {}
    with open(mj) as f:
        mods = sorted(json.load(f), key=lambda m: m.get("idx", 0))
    kinds = [str(m.get("type", "")).rsplit(".", 1)[-1] for m in mods]
    if kinds not in (["Transformer", "Pooling", "Normalize"], ["Transformer", "Pooling", "Dense", "Normalize"]):
        raise NotImplementedError(f"{model_dir}: modules.json names {kinds}; supported: Transformer, Pooling, [Dense,] Normalize")
    on = sorted(k for k, v in _pooling_config(model_dir, mods).items() if k.startswith("pooling_mode_") and v is True)
    if on != ["pooling_mode_mean_tokens"]:
        raise NotImplementedError(f"{model_dir}: pooling {on} (supported: pooling_mode_mean_tokens)")
    if len(mods) == 3:
        return {}
    d = os.path.join(model_dir, mods[2]["path"])
    with open(os.path.join(d, "config.json")) as f:
        dc = json.load(f)
    act = str(dc.get("activation_function", "torch.nn.modules.linear.Identity")).rsplit(".", 1)[-1]
    if dc.get("bias", True):
        raise NotImplementedError(f"{d}: bias=true: the Dense module of the T5 tail carries no bias")
    if act != "Identity":
        raise NotImplementedError(f"{d}: activation_function={dc.get('activation_function')!r} (supported: Identity)")
    if os.path.exists(os.path.join(d, "model.safetensors")):
        sd = load_file(os.path.join(d, "model.safetensors"))
    else:
        sd = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu", weights_only=True)
    if sorted(sd) != ["linear.weight"]:
        raise NotImplementedError(f"{d}: tensors {sorted(sd)} (expected linear.weight alone)")
    w = sd["linear.weight"]
    if tuple(w.shape) != (dc.get("out_features", w.shape[0]), dc.get("in_features", w.shape[1])):
        raise ValueError(f"{d}: linear.weight {tuple(w.shape)} does not match its config.json")
    return {DENSE_NAME: w}


def include_prompt(model_dir: Optional[str]) -> bool:
    """``1_Pooling/config.json``'s ``include_prompt`` (sentence-transformers ``Pooling``; INSTRUCTOR sets it false): whether the
    tokens of the instruction take part in the mean.  Absent: true."""
    if not model_dir:
        return True
    pc = os.path.join(model_dir, "1_Pooling", "config.json")
    if not os.path.exists(pc):
        return True
    with open(pc) as f:
        return json.load(f).get("include_prompt", True) is not False


def max_seq_length(model_dir: Optional[str]) -> int:
    """``sentence_bert_config.json``'s ``max_seq_length`` (256 for sentence-t5, 512 for gtr-t5 and INSTRUCTOR), capped at
    ``MAX_TOKENS``; ``MAX_TOKENS`` when the directory names none."""
    if model_dir:
        sb = os.path.join(model_dir, "sentence_bert_config.json")
        if os.path.exists(sb):
            with open(sb) as f:
                n = json.load(f).get("max_seq_length")
            if n:
                return max(1, min(int(n), MAX_TOKENS))
    return MAX_TOKENS


def prompt_tokens(tokenizer, prompt: str) -> int:
    """How many leading tokens of ``prompt + text`` belong to the instruction, as sentence-transformers counts them: the tokens
    ``prompt`` alone gives, without the ``</s>`` that closes it."""
    return max(0, len(tokenizer.encode(prompt, None)) - 1) if prompt else 0


def pooled_ranges(seq_start: np.ndarray, seq_len: np.ndarray, skip: int) -> Tuple[np.ndarray, np.ndarray]:
    """The row range each sequence's mean is taken over when the first ``skip`` tokens (the instruction) stay out of it:
    ``(seq_start + skip, seq_len - skip)``, what ``tt_t5_pool_dense`` is handed.  A text with nothing left behind its prompt
    (empty, or cut away by the length limit) has no mean: ValueError."""
    if skip < 0:
        raise ValueError(f"prompt length {skip}")
    starts, lens = np.asarray(seq_start, dtype=np.int64) + skip, np.asarray(seq_len, dtype=np.int64) - skip
    if (lens <= 0).any():
        b = int(np.argmax(lens <= 0))
        raise ValueError(f"include_prompt is false and text {b} has no token left behind its {skip}-token prompt "
                         f"({int(seq_len[b])} tokens in all)")
    return starts.astype(np.int32), lens.astype(np.int32)


class T5Weights(_FamilyWeights):
    """Device-resident T5 encoder weights for ``tt_t5_forward``: the projections and the embedding table in bf16 -- q (times 8), k
    and v rows concatenated into one matrix, wi_0 / wi_1 of the gated form into another -- the norm weights in fp32 holding the
    values their bf16 rounding has (transformers multiplies by the bf16 weight), block 0's bias table and the per-head distance
    table built from it in fp32, and the Dense module in fp32, transposed to [in][out] (the tail kernel's threads read it row by
    row)."""

    _paths, _path_name = (T5_BF16_PATH,), "the T5 path"

    def __init__(self, cfg: T5Config, state: Dict[str, torch.Tensor], device: torch.device, dtype: torch.dtype = torch.bfloat16):
        self._begin(cfg, device, dtype, dtypes=(torch.bfloat16,))
        check_config(cfg)
        sd = check_state(cfg, state)
        H, F = cfg.hidden, cfg.ffn
        class Rounded:
            """What the loaders read: every tensor rounded to bf16 first -- the norm weights then hold their bf16 values in fp32 --
            and the q rows times 8 (a power of two: exact)."""
            def __getitem__(self, name):
                t = sd[name].to(dtype)
                return t * 8.0 if name.endswith("SelfAttention.q.weight") else t

        mat, vec = self._loaders(Rounded())
        emb = mat([_EMBED], (cfg.vocab_size, H))
        self._layers = (_T5LayerW * max(cfg.layers, 1))()
        for i in range(cfg.layers):
            p, L = f"encoder.block.{i}.", self._layers[i]
            a, m = p + "layer.0.SelfAttention.", p + "layer.1.DenseReluDense."
            L.ln_attn = vec([p + "layer.0.layer_norm.weight"], H)
            L.qkv_w = mat([a + "q.weight", a + "k.weight", a + "v.weight"], (3 * H, H))
            L.o_w = mat([a + "o.weight"], (H, H))
            L.ln_ffn = vec([p + "layer.1.layer_norm.weight"], H)
            if cfg.mlp_kind == 1:
                L.wi = mat([m + "wi_0.weight", m + "wi_1.weight"], (2 * F, H))
            else:
                L.wi = mat([m + "wi.weight"], (F, H))
            L.wo = mat([m + "wo.weight"], (H, F))
        rel = sd[_REL_BIAS]
        if tuple(rel.shape) != (NUM_BUCKETS, cfg.heads):
            raise ValueError(f"{_REL_BIAS} {tuple(rel.shape)} does not match {cfg} (expected {(NUM_BUCKETS, cfg.heads)})")
        rel = self._kept(rel.to(dtype).to(device=device, dtype=torch.float32).contiguous())
        self.bias_table = self._kept(distance_table(rel))
        dense_out, dense_wt = 0, None
        if DENSE_NAME in sd:
            dw = sd[DENSE_NAME]
            if dw.dim() != 2 or dw.shape[1] != H:
                raise ValueError(f"Dense module {tuple(dw.shape)} does not read d_model={H}")
            dense_out = int(dw.shape[0])
            if dense_out % 128 or dense_out > 1024:
                raise NotImplementedError(f"t5: Dense out_features={dense_out} (a multiple of 128 up to 1024, the scan's limit)")
            dense_wt = self._kept(dw.to(device=device, dtype=torch.float32).t().contiguous()).data_ptr()
        self.out_dim = dense_out or H
        self.struct = _T5W(d_model=H, layers=cfg.layers, heads=cfg.heads, d_kv=cfg.d_kv, d_ff=F, vocab=cfg.vocab_size,
                           mlp_kind=cfg.mlp_kind, num_buckets=cfg.num_buckets, max_distance=cfg.max_distance, eps=cfg.ln_eps,
                           embed=emb, layer=ctypes.cast(self._layers, POINTER(_T5LayerW)),
                           final_norm=vec(["encoder.final_layer_norm.weight"], H), rel_bias=rel.data_ptr(),
                           bias_table=self.bias_table.data_ptr(), dense_out=dense_out, dense_wt=dense_wt)


def synthetic_state(cfg: T5Config, seed: int = 0, dense: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Seeded random T5 encoder weights of ``cfg`` (fp32, CPU) with trained-model-like scales: unit-scale embeddings (T5 does not
    normalise them), projections whose outputs stay of order one, norm weights around 1, a bias table several units wide, and a
    Dense module d_model -> ``dense`` (default 768, the published checkpoints' width; 0: none)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, std):
        return torch.randn(*shape, generator=g) * std

    H, F = cfg.hidden, cfg.ffn
    sd = {_EMBED: rnd(cfg.vocab_size, H, std=1.0), _REL_BIAS: rnd(NUM_BUCKETS, cfg.heads, std=2.0),
          "encoder.final_layer_norm.weight": 1 + rnd(H, std=0.1)}
    for i in range(cfg.layers):
        p = f"encoder.block.{i}."
        a, m = p + "layer.0.SelfAttention.", p + "layer.1.DenseReluDense."
        sd[a + "q.weight"], sd[a + "k.weight"] = rnd(H, H, std=(H * 8.0) ** -0.5), rnd(H, H, std=H ** -0.5)
        sd[a + "v.weight"], sd[a + "o.weight"] = rnd(H, H, std=H ** -0.5), rnd(H, H, std=H ** -0.5)
        sd[p + "layer.0.layer_norm.weight"], sd[p + "layer.1.layer_norm.weight"] = 1 + rnd(H, std=0.1), 1 + rnd(H, std=0.1)
        for n in (("wi_0", "wi_1") if cfg.mlp_kind == 1 else ("wi",)):
            sd[m + n + ".weight"] = rnd(F, H, std=H ** -0.5)
        sd[m + "wo.weight"] = rnd(H, F, std=F ** -0.5)
    n_out = 768 if dense is None else dense
    if n_out:
        sd[DENSE_NAME] = rnd(n_out, H, std=H ** -0.5)
    return sd


# the published geometries (config.json of the six checkpoints: relu, vocab 32128, d_kv 64; a Dense module to 768)
T5_BASE = T5Config(vocab_size=32128, hidden=768, layers=12, heads=12, ffn=3072, max_pos=MAX_TOKENS, type_vocab=1, pad_id=0,
                   ln_eps=1e-6)
T5_LARGE = T5Config(vocab_size=32128, hidden=1024, layers=24, heads=16, ffn=4096, max_pos=MAX_TOKENS, type_vocab=1, pad_id=0,
                    ln_eps=1e-6)
KNOWN_CONFIGS = {"sentence-transformers/sentence-t5-base": T5_BASE, "sentence-transformers/sentence-t5-large": T5_LARGE,
                 "sentence-transformers/gtr-t5-base": T5_BASE, "sentence-transformers/gtr-t5-large": T5_LARGE,
                 "hkunlp/instructor-base": T5_BASE, "hkunlp/instructor-large": T5_LARGE}
