"""Encoder (bi-encoder / cross-encoder) host side: weight packing, varlen token packing and
the ctypes calls into libtt_hip.so's ``tt_encoder_forward`` / ``tt_embed_pool`` /
``tt_rerank_head``.

Mirrors what the reference obtains from ``HuggingFaceEmbedding`` (built at
``src/tensortruth/services/model_manager.py:254-260``) and ``SentenceTransformerRerank``
(``model_manager.py:333-337``): XLM-R / BERT encoder forward -> CLS pooling + L2
normalisation (embeddings), or -> classification head + sigmoid (rerank scores).
There is no CPU path.

``Encoder`` drives every precision: the weights object it is given names its path through the library as an
``EncoderPath`` record.  The 16-bit path is here (``EncoderWeights``: bf16 with fp32 accumulation, the reference's
``torch_dtype: bfloat16`` option, ``model_manager.py:218-229``; or fp16); the reference-precision paths keep their weight
classes in ``encoder_x3`` (split planes), ``encoder_f16c`` and ``encoder_f32``, all built by the one checkpoint walk of
``_CheckpointWeights``.
"""
from __future__ import annotations

import ctypes
import dataclasses
import itertools
import os
import threading
from ctypes import POINTER, Structure, c_float, c_int32, c_void_p
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


@dataclass(frozen=True)
class EncoderConfig:
    """The HF config fields the hot path reads."""

    # "xlmr" | "bert" | "qwen3" (decoder embedder: decoder.DecoderConfig) | "modernbert" (modernbert.ModernBertConfig) |
    # "gemma3_text" (EmbeddingGemma: gemma.GemmaConfig) | "mpnet" (MPNet embedders: mpnet.MpnetWeights; positions as "xlmr") |
    # "deberta-v2" (DeBERTa-v2 / v3 cross-encoders: deberta.DebertaConfig)
    # "nomic_bert" | "jina_embeddings_v3" (post-LN encoders with RoPE: ropebert.RopeBertConfig; positions 0-based)
    # "t5" (T5 encoders: t5.T5Config; no positions)
    # "jina_bert" (JinaBERT, jina-embeddings-v2: jinabert.JinaBertConfig; ALiBi attention, no position table)
    arch: str = "xlmr"
    vocab_size: int = 250002
    hidden: int = 1024
    layers: int = 24
    heads: int = 16
    ffn: int = 4096
    max_pos: int = 8194
    type_vocab: int = 1
    pad_id: int = 1
    ln_eps: float = 1e-5     # the RMSNorm epsilon for "qwen3"
    num_labels: int = 0

    @property
    def max_seq_len(self) -> int:
        # XLM-R (and MPNet) reserves positions 0..pad_id for padding
        return self.max_pos - (self.pad_id + 1) if self.arch in ("xlmr", "mpnet") else self.max_pos


BGE_M3 = EncoderConfig()
BGE_RERANKER_V2_M3 = EncoderConfig(num_labels=1)
BGE_SMALL_EN_V15 = EncoderConfig(arch="bert", vocab_size=30522, hidden=384, layers=12, heads=12, ffn=1536,
                                 max_pos=512, type_vocab=2, pad_id=0, ln_eps=1e-12)

# the other two rerankers the reference offers out of the box (app_utils/config_schema.py:83-87): XLM-R base with the same
# head as v2-m3, and a 6-layer BERT (MiniLM) whose head is BertForSequenceClassification's pooler + classifier
BGE_RERANKER_BASE = EncoderConfig(vocab_size=250002, hidden=768, layers=12, heads=12, ffn=3072, max_pos=514, num_labels=1)
MS_MARCO_MINILM_L6_V2 = EncoderConfig(arch="bert", vocab_size=30522, hidden=384, layers=6, heads=12, ffn=1536, max_pos=512,
                                      type_vocab=2, pad_id=0, ln_eps=1e-12, num_labels=1)

KNOWN_CONFIGS = {
    "BAAI/bge-m3": BGE_M3,
    "BAAI/bge-reranker-v2-m3": BGE_RERANKER_V2_M3,
    "BAAI/bge-small-en-v1.5": BGE_SMALL_EN_V15,
    "BAAI/bge-reranker-base": BGE_RERANKER_BASE,
    "cross-encoder/ms-marco-MiniLM-L-6-v2": MS_MARCO_MINILM_L6_V2,
}


# the twelve tensors of a layer, in the order tt_layer_weights, tt_layer_weights_f32 and tt_layer_weights_x3 of
# include/tt_hip.h start with them (tt_layer_weights_f16c interleaves block-scale pointers: encoder_f16c._LayerWC)
_LAYER_FIELDS = ("qkv_w", "qkv_b", "o_w", "o_b", "ln1_g", "ln1_b", "ffn1_w", "ffn1_b", "ffn2_w", "ffn2_b", "ln2_g", "ln2_b")


class _LayerW(Structure):
    """tt_layer_weights: the layer's tensors, then the fp8 operands of its projections (``set_gemm_dtype("fp8")``)."""
    _fields_ = [(n, c_void_p) for n in _LAYER_FIELDS + ("qkv_w8", "qkv_wscale", "ffn1_w8", "ffn1_wscale",
                                                         "o_w8", "o_wscale", "ffn2_w8", "ffn2_wscale")] + [("ffn_act_scale", c_float)]


class _PlainLayerW(Structure):
    """tt_layer_weights_f32 and tt_layer_weights_x3: the layer's tensors and nothing else."""
    _fields_ = [(n, c_void_p) for n in _LAYER_FIELDS]


def _weights_struct(name: str, layer: type, *extra) -> type:
    """ctypes mirror of one of the tt_encoder_weights* structs: the header they share, with a ``layer`` array of ``layer``
    structs, then ``extra`` fields.  The struct type's ``layer_type`` is ``layer``."""
    fields = ([(n, c_int32) for n in ("hidden", "layers", "heads", "ffn", "vocab", "max_pos", "type_vocab")] + [("ln_eps", c_float)]
              + [(n, c_void_p) for n in ("word_emb", "pos_emb", "type_emb", "emb_ln_g", "emb_ln_b")] + [("layer", POINTER(layer))]
              + [(n, c_void_p) for n in ("cls_dense_w", "cls_dense_b", "cls_out_w", "cls_out_b")] + list(extra))
    return type(name, (Structure,), {"_fields_": fields, "layer_type": layer})


_EncW = _weights_struct("_EncW", _LayerW, ("ffn_absmax_out", c_void_p))


@dataclass(frozen=True, kw_only=True)
class EncoderPath:
    """What a weights class tells ``Encoder`` about its path through libtt_hip.so: the entry points, the ``_scratch`` keys of
    their workspaces, the element type of the hidden states and how a batch's rows are padded.

    ``row_tile``: the path's GEMMs run whole tiles of this many rows, so a batch's rows are rounded up to a multiple of it (0:
    the rows as packed).  ``skinny``: up to 256 rows in multiples of 64 are kept (weight-streaming skinny GEMMs), and the
    CLS-only output is padded to 64 rows up to 256 sequences; otherwise that output is padded to 256 rows."""

    forward: str                 # the whole forward, and its workspace size
    workspace: str
    cls_forward: Optional[str]   # the last layer for the CLS rows only, and its workspace size; None: pooling and the head
    cls_workspace: Optional[str]  # read the full forward's hidden states at the sequence starts
    pool: str                    # CLS and mean pooling
    pool_mean: str
    head: Optional[str]          # classification head; its workspace holds two padded [B, H] tiles of hidden-state elements
    scratch: str                 # _scratch keys of the forward's and the head's workspaces
    head_scratch: str
    hidden: torch.dtype          # element type of the hidden states
    row_tile: int = 0
    skinny: bool = False
    pool_writes_bf16: bool = True  # the pooling kernel writes the bf16 copy of an embedding (else it is rounded from fp32 here)
    no_fp8: Optional[str] = None   # why ``calibrate_fp8`` does not apply; None: it does
    pool_last: Optional[str] = None  # last-token pooling (decoder embedders); None: the path has none
    rows_forward: Optional[str] = None    # decoder paths: the forward whose last layer runs for ONE row per sequence only
    rows_workspace: Optional[str] = None  # (``pooled_rows``), and its workspace size
    score: Optional[str] = None      # decoder paths: the *ForSequenceClassification score head over those rows
    pooled_head: Optional[str] = None  # ModernBERT / DeBERTa paths: pooling ("cls" / "mean") + classification head over the full forward
    pool_dense: Optional[str] = None   # EmbeddingGemma / T5 paths: mean pooling + the Dense module(s) + L2 norm over the full forward


BF16_PATH = EncoderPath(forward="tt_encoder_forward", workspace="tt_encoder_workspace_bytes",
                        cls_forward="tt_encoder_forward_cls", cls_workspace="tt_encoder_cls_workspace_bytes",
                        pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head="tt_rerank_head",
                        scratch="enc", head_scratch="head", hidden=torch.bfloat16)
FP16_PATH = EncoderPath(forward="tt_encoder_forward_f16", workspace="tt_encoder_workspace_bytes_f16",
                        cls_forward="tt_encoder_forward_cls_f16", cls_workspace="tt_encoder_cls_workspace_bytes_f16",
                        pool="tt_embed_pool_f16", pool_mean="tt_embed_pool_mean_f16", head="tt_rerank_head_f16",
                        scratch="enc", head_scratch="head", hidden=torch.float16, pool_writes_bf16=False)
# the decoder embedder (Qwen3Model architecture, decoder.DecoderWeights): full forward, then last-token pooling; its hidden states
# have the encoder's layout, so first-token and mean pooling read them with the encoder's kernels.  Its one-row-per-sequence tail
# (``rows_forward``: last-token pooling, and the classification checkpoints' score head) keeps whichever row ``pooled_rows`` names.
DECODER_BF16_PATH = EncoderPath(forward="tt_decoder_forward", workspace="tt_decoder_workspace_bytes", cls_forward=None,
                                cls_workspace=None, pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head=None,
                                scratch="enc", head_scratch="head", hidden=torch.bfloat16, pool_last="tt_embed_pool_last",
                                rows_forward="tt_decoder_forward_rows", rows_workspace="tt_decoder_rows_workspace_bytes",
                                score="tt_decoder_score", no_fp8="the decoder embedder has no fp8 projections")
DECODER_FP16_PATH = EncoderPath(forward="tt_decoder_forward_f16", workspace="tt_decoder_workspace_bytes_f16", cls_forward=None,
                                cls_workspace=None, pool="tt_embed_pool_f16", pool_mean="tt_embed_pool_mean_f16", head=None,
                                scratch="enc", head_scratch="head", hidden=torch.float16, pool_writes_bf16=False,
                                pool_last="tt_embed_pool_last_f16", rows_forward="tt_decoder_forward_rows_f16",
                                rows_workspace="tt_decoder_rows_workspace_bytes_f16", score="tt_decoder_score_f16",
                                no_fp8="the decoder embedder has no fp8 projections")
# ModernBERT encoders (modernbert.ModernBertWeights): full forward; first-token and mean pooling with the encoder's kernels; the
# classification head pools ("cls" / "mean", the checkpoint's ``classifier_pooling``) the full forward's rows itself.
MODERNBERT_BF16_PATH = EncoderPath(forward="tt_modernbert_forward", workspace="tt_modernbert_workspace_bytes", cls_forward=None,
                                   cls_workspace=None, pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head=None,
                                   scratch="enc", head_scratch="head", hidden=torch.bfloat16, pooled_head="tt_modernbert_head",
                                   no_fp8="the ModernBERT path has no fp8 projections")
MODERNBERT_FP16_PATH = EncoderPath(forward="tt_modernbert_forward_f16", workspace="tt_modernbert_workspace_bytes_f16",
                                   cls_forward=None, cls_workspace=None, pool="tt_embed_pool_f16",
                                   pool_mean="tt_embed_pool_mean_f16", head=None, scratch="enc", head_scratch="head",
                                   hidden=torch.float16, pool_writes_bf16=False, pooled_head="tt_modernbert_head_f16",
                                   no_fp8="the ModernBERT path has no fp8 projections")
# EmbeddingGemma embedders (gemma.GemmaWeights): full forward, then the sentence-transformers tail in one entry point (mean pooling,
# Dense, Dense, Normalize); bf16 only, no other pooling, no head.
GEMMA_BF16_PATH = EncoderPath(forward="tt_gemma_forward", workspace="tt_gemma_workspace_bytes", cls_forward=None, cls_workspace=None,
                              pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head=None, scratch="enc", head_scratch="head",
                              hidden=torch.bfloat16, pool_dense="tt_gemma_pool_dense",
                              no_fp8="the EmbeddingGemma path has no fp8 projections")
# MPNet embedders (mpnet.MpnetWeights): full forward with the relative-position bias in the attention; first-token and mean pooling
# with the encoder's kernels; no CLS-only forward, no head, no fp8.
MPNET_BF16_PATH = EncoderPath(forward="tt_mpnet_forward", workspace="tt_mpnet_workspace_bytes", cls_forward=None, cls_workspace=None,
                              pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head=None, scratch="enc", head_scratch="head",
                              hidden=torch.bfloat16, no_fp8="the MPNet path has no fp8 projections")
MPNET_FP16_PATH = EncoderPath(forward="tt_mpnet_forward_f16", workspace="tt_mpnet_workspace_bytes_f16", cls_forward=None,
                              cls_workspace=None, pool="tt_embed_pool_f16", pool_mean="tt_embed_pool_mean_f16", head=None,
                              scratch="enc", head_scratch="head", hidden=torch.float16, pool_writes_bf16=False,
                              no_fp8="the MPNet path has no fp8 projections")

# DeBERTa-v2 / v3 cross-encoders (deberta.DebertaWeights): full forward with disentangled attention; the classification head
# (ContextPooler + classifier) reads the full forward's first rows; no CLS-only forward, no fp8.
DEBERTA_BF16_PATH = EncoderPath(forward="tt_deberta_forward", workspace="tt_deberta_workspace_bytes", cls_forward=None,
                                cls_workspace=None, pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head=None, scratch="enc",
                                head_scratch="head", hidden=torch.bfloat16, pooled_head="tt_deberta_head",
                                no_fp8="the DeBERTa path has no fp8 projections")
DEBERTA_FP16_PATH = EncoderPath(forward="tt_deberta_forward_f16", workspace="tt_deberta_workspace_bytes_f16", cls_forward=None,
                                cls_workspace=None, pool="tt_embed_pool_f16", pool_mean="tt_embed_pool_mean_f16", head=None,
                                scratch="enc", head_scratch="head", hidden=torch.float16, pool_writes_bf16=False,
                                pooled_head="tt_deberta_head_f16", no_fp8="the DeBERTa path has no fp8 projections")

# NomicBERT / Jina-v3 embedders (ropebert.RopeBertWeights): post-LN layers with RoPE; first-token and mean pooling with the
# encoder's kernels; no CLS-only forward, no head, no fp8.
ROPEBERT_BF16_PATH = EncoderPath(forward="tt_ropebert_forward", workspace="tt_ropebert_workspace_bytes", cls_forward=None,
                                 cls_workspace=None, pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head=None, scratch="enc",
                                 head_scratch="head", hidden=torch.bfloat16, no_fp8="the NomicBERT / Jina-v3 path has no fp8 projections")
ROPEBERT_FP16_PATH = EncoderPath(forward="tt_ropebert_forward_f16", workspace="tt_ropebert_workspace_bytes_f16", cls_forward=None,
                                 cls_workspace=None, pool="tt_embed_pool_f16", pool_mean="tt_embed_pool_mean_f16", head=None,
                                 scratch="enc", head_scratch="head", hidden=torch.float16, pool_writes_bf16=False,
                                 no_fp8="the NomicBERT / Jina-v3 path has no fp8 projections")

# JinaBERT embedders (jinabert.JinaBertWeights): post-LN layers with ALiBi attention and GEGLU; first-token and mean pooling with
# the encoder's kernels; no CLS-only forward, no head, no fp8.
JINABERT_BF16_PATH = EncoderPath(forward="tt_jinabert_forward", workspace="tt_jinabert_workspace_bytes", cls_forward=None,
                                 cls_workspace=None, pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head=None, scratch="enc",
                                 head_scratch="head", hidden=torch.bfloat16, no_fp8="the JinaBERT path has no fp8 projections")
JINABERT_FP16_PATH = EncoderPath(forward="tt_jinabert_forward_f16", workspace="tt_jinabert_workspace_bytes_f16", cls_forward=None,
                                 cls_workspace=None, pool="tt_embed_pool_f16", pool_mean="tt_embed_pool_mean_f16", head=None,
                                 scratch="enc", head_scratch="head", hidden=torch.float16, pool_writes_bf16=False,
                                 no_fp8="the JinaBERT path has no fp8 projections")

# T5 encoders (t5.T5Weights): full forward with MPNet's biased attention kernel; the sentence-transformers tail in one entry point
# (mean pooling over a row range, the optional Dense, Normalize); bf16 only, no other pooling, no head.
T5_BF16_PATH = EncoderPath(forward="tt_t5_forward", workspace="tt_t5_workspace_bytes", cls_forward=None, cls_workspace=None,
                           pool="tt_embed_pool", pool_mean="tt_embed_pool_mean", head=None, scratch="enc", head_scratch="head",
                           hidden=torch.bfloat16, pool_dense="tt_t5_pool_dense", no_fp8="the T5 path has no fp8 projections")


def _strip_prefix(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for k, v in sd.items():
        for pre in ("roberta.", "bert.", "model.", "0.auto_model."):
            if k.startswith(pre):
                k = k[len(pre):]
                break
        out[k] = v
    # BertForSequenceClassification (cross-encoder/ms-marco-MiniLM-L-6-v2, the third of the reference's out-of-the-box
    # rerankers, config_schema.py:83-87): logits = classifier(tanh(pooler.dense(h[CLS]))) -- the same dense -> tanh -> projection
    # as RobertaClassificationHead's classifier.dense / classifier.out_proj, under other names
    if "classifier.dense.weight" not in out and "pooler.dense.weight" in out and "classifier.weight" in out:
        out["classifier.dense.weight"], out["classifier.dense.bias"] = out["pooler.dense.weight"], out["pooler.dense.bias"]
        out["classifier.out_proj.weight"], out["classifier.out_proj.bias"] = out["classifier.weight"], out["classifier.bias"]
    return out


class _CheckpointWeights:
    """Device-resident weights built from an HF state dict (``embeddings.word_embeddings.weight``,
    ``encoder.layer.{i}.attention.self.query.weight`` ... optional ``roberta.``/``bert.`` prefix, ``classifier.dense`` /
    ``classifier.out_proj`` for the reranker), in the struct layout of one path of libtt_hip.so.

    ``_load`` walks the checkpoint for every weight class; biases and LayerNorm parameters are fp32 on every path.  A
    subclass says how it stores the projections (``_matrix``) and the embedding tables and classifier matrices
    (``_table``; fp32 here), and carries its ``path`` and ctypes ``_Struct``."""

    path: EncoderPath
    _Struct: type

    def _load(self, cfg: EncoderConfig, state: Dict[str, torch.Tensor], device: torch.device) -> None:
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} need a HIP device; tensor_truth_amd has no CPU path")
        self.cfg, self.device = cfg, device
        self._keep: List[torch.Tensor] = []
        sd = _strip_prefix(state)

        def take(*names):
            return sd[names[0]] if len(names) == 1 else torch.cat([sd[n] for n in names], 0)

        def vec(*names):
            return self._kept(names, take(*names).to(device=device, dtype=torch.float32).contiguous()).data_ptr()

        def table(name):
            return self._table([name], sd[name])

        H = cfg.hidden
        word, pos, typ = (table(f"embeddings.{n}_embeddings.weight") for n in ("word", "position", "token_type"))
        if word.shape != (cfg.vocab_size, H) or pos.shape != (cfg.max_pos, H):
            raise ValueError(f"embedding tables {tuple(word.shape)} / {tuple(pos.shape)} do not match {cfg}")
        w = self._Struct(hidden=H, layers=cfg.layers, heads=cfg.heads, ffn=cfg.ffn, vocab=cfg.vocab_size, max_pos=cfg.max_pos,
                         type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps, word_emb=word.data_ptr(), pos_emb=pos.data_ptr(),
                         type_emb=typ.data_ptr(), emb_ln_g=vec("embeddings.LayerNorm.weight"),
                         emb_ln_b=vec("embeddings.LayerNorm.bias"))
        self._layers = (self._Struct.layer_type * max(cfg.layers, 1))()
        for i in range(cfg.layers):
            p = f"encoder.layer.{i}."
            L = self._layers[i]
            for field, mods in (("qkv", [f"attention.self.{n}." for n in ("query", "key", "value")]),   # one [3H][H] matrix
                                ("o", ["attention.output.dense."]), ("ffn1", ["intermediate.dense."]), ("ffn2", ["output.dense."])):
                names = [p + m + "weight" for m in mods]
                self._matrix(L, field + "_w", names, take(*names))
                setattr(L, field + "_b", vec(*(p + m + "bias" for m in mods)))
            L.ln1_g, L.ln1_b = vec(p + "attention.output.LayerNorm.weight"), vec(p + "attention.output.LayerNorm.bias")
            L.ln2_g, L.ln2_b = vec(p + "output.LayerNorm.weight"), vec(p + "output.LayerNorm.bias")
        w.layer = ctypes.cast(self._layers, POINTER(self._Struct.layer_type))
        if cfg.num_labels:
            if cfg.num_labels != 1:
                raise ValueError("only single-label (sigmoid) cross-encoder heads are supported")
            w.cls_dense_w, w.cls_dense_b = table("classifier.dense.weight").data_ptr(), vec("classifier.dense.bias")
            w.cls_out_w, w.cls_out_b = table("classifier.out_proj.weight").data_ptr(), vec("classifier.out_proj.bias")
        self.struct = w

    def _kept(self, names: Sequence[str], t: torch.Tensor) -> torch.Tensor:
        """Keep ``t`` (the tensor of the checkpoint entries ``names``, concatenated) resident."""
        self._keep.append(t)
        return t

    def _table(self, names: Sequence[str], x: torch.Tensor) -> torch.Tensor:
        return self._kept(names, x.to(device=self.device, dtype=torch.float32).contiguous())

    def _matrix(self, L: Structure, field: str, names: Sequence[str], x: torch.Tensor) -> None:
        """Store one projection ``x`` [out][in] (checkpoint entries ``names``) and point ``L.<field>`` at it."""
        setattr(L, field, self._table(names, x).data_ptr())

    def parameters(self) -> Iterable[torch.Tensor]:
        """For ModelManager-style memory accounting (reference model_manager.py:477-507)."""
        return iter(self._keep)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._keep)


class _FamilyWeights:
    """What the weight holders of the packed-varlen families share -- post-LN (mpnet.py, deberta.py, jinabert.py, ropebert.py) and
    pre-norm (decoder.py, modernbert.py, t5.py, gemma.py): the dtype / device checks, the resident tensors and the two loaders of
    checkpoint entries.  A subclass names its paths (``_paths``: bf16, then fp16 where the family has one) and what the dtype error
    calls them (``_path_name``), and builds its own ctypes struct."""

    _paths: Tuple[EncoderPath, ...]
    _path_name: str

    def _begin(self, cfg: EncoderConfig, device: torch.device, dtype: torch.dtype,
               dtypes: Tuple[torch.dtype, ...] = (torch.bfloat16, torch.float16)) -> None:
        """``dtypes``: what the family computes in, in the order of ``_paths`` (T5 and EmbeddingGemma: bfloat16 alone)."""
        name = type(self).__name__
        if dtype not in dtypes:
            if len(dtypes) == 1:
                raise NotImplementedError(f"{name}: {self._path_name} computes in bfloat16 only")
            raise ValueError(f"{name}: {self._path_name} computes in bfloat16 or float16")
        if device.type != "cuda":
            raise RuntimeError(f"{name} need a HIP device; tensor_truth_amd has no CPU path")
        self.cfg, self.device, self.dtype = cfg, device, dtype
        self.path = self._paths[dtypes.index(dtype)]
        self.gemm_dtype = dtype
        self._keep: List[torch.Tensor] = []

    def _loaders(self, sd: Dict[str, torch.Tensor], flatten: bool = False):
        """``(mat, vec)``: ``mat(names, shape)`` keeps the checkpoint entries ``names`` of ``sd``, concatenated along dim 0, in the
        element type and ``vec(names, n)`` in fp32; both return the device address and refuse a shape other than the one given.
        ``flatten``: ``vec`` takes entries of any shape (a [1][H] classifier row) and reads them as vectors."""
        def mat(names, shape):
            t = torch.cat([sd[n] for n in names], 0)
            if tuple(t.shape) != shape:
                raise ValueError(f"{names[0]} ... {tuple(t.shape)} does not match {self.cfg} (expected {shape})")
            return self._kept(t.to(device=self.device, dtype=self.dtype).contiguous()).data_ptr()

        def vec(names, n):
            t = torch.cat([sd[x].reshape(-1) if flatten else sd[x] for x in names], 0)
            if tuple(t.shape) != (n,):
                raise ValueError(f"{names[0]} ... {tuple(t.shape)} does not match {self.cfg}")
            return self._kept(t.to(device=self.device, dtype=torch.float32).contiguous()).data_ptr()

        return mat, vec

    def _kept(self, t: torch.Tensor) -> torch.Tensor:
        self._keep.append(t)
        return t

    def parameters(self) -> Iterable[torch.Tensor]:
        """For ModelManager-style memory accounting (reference model_manager.py:477-507)."""
        return iter(self._keep)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._keep)


class EncoderWeights(_CheckpointWeights):
    """The 16-bit path (``tt_encoder_forward``): matrices and embedding tables in bf16, or fp16 (the library's ``*_f16``
    entry points); biases and LayerNorm parameters fp32."""

    _Struct = _EncW

    def __init__(self, cfg: EncoderConfig, state: Dict[str, torch.Tensor], device: torch.device,
                 dtype: torch.dtype = torch.bfloat16):
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("EncoderWeights: the 16-bit path computes in bfloat16 or float16")
        self.dtype = dtype           # element type of matrices and activations: bf16, or fp16 (libtt_hip's *_f16 entry points)
        self.path = FP16_PATH if dtype == torch.float16 else BF16_PATH
        self._named: Dict[str, torch.Tensor] = {}     # HF name -> the resident tensor (state_dict())
        self._qkv_w: List[torch.Tensor] = []
        self._ffn1_w: List[torch.Tensor] = []
        self._o_w: List[torch.Tensor] = []
        self._ffn2_w: List[torch.Tensor] = []
        self._fp8: List[torch.Tensor] = []
        self.ffn_act_scales: Optional[List[float]] = None   # per layer, from calibrate_fp8()
        self.gemm_dtype = "bf16"
        self._load(cfg, state, device)

    def _kept(self, names, t):
        self._named.update(zip(names, t.chunk(len(names)) if len(names) > 1 else [t]))    # Q / K / V: row slices
        return super()._kept(names, t)

    def _table(self, names, x):
        return self._kept(names, x.to(device=self.device, dtype=self.dtype).contiguous())

    def _matrix(self, L, field, names, x):
        t = self._table(names, x)
        getattr(self, "_" + field).append(t)
        setattr(L, field, t.data_ptr())

    @staticmethod
    def _quantize_rows(w: torch.Tensor):
        """bf16 [out][in] -> (e4m3 bytes [out][in], fp32 scale [out]) with w ~= w8 * scale[out]."""
        wf = w.to(torch.float32)
        amax = wf.abs().amax(dim=1, keepdim=True)
        inv = torch.where(amax > 0, 448.0 / amax, torch.zeros_like(amax))
        w8 = (wf * inv).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
        scale = torch.where(amax > 0, amax * (1.0 / 448.0), torch.ones_like(amax)).reshape(-1).contiguous()
        return w8, scale

    def set_gemm_dtype(self, dtype: str) -> None:
        """"bf16" (default) or "fp8": the encoder layers' projections run on OCP e4m3 operands with fp32 accumulation
        (BASELINE.json config 5, "fp8 MFMA reranker").  Weights are quantised here per output channel; activations
        per token inside the LayerNorm kernels (Q/K/V, FFN-up inputs) or by a row pass (attention context); the FFN
        intermediate is written as e4m3 by the FFN-up epilogue with one static scale per layer, which needs
        ``calibrate_fp8`` first -- without it the FFN output projection stays bf16.  Needs hidden and ffn to be
        multiples of 256; the bf16 weights stay resident (CLS tail, small batches)."""
        if dtype not in ("bf16", "fp8"):
            raise ValueError(f"gemm dtype {dtype!r} not in ('bf16', 'fp8')")
        if dtype == "fp8" and self.dtype != torch.bfloat16:
            raise ValueError("fp8 projections exist for bf16 encoders only")
        n = self.cfg.layers
        if dtype == "fp8":
            if self.cfg.hidden % 256 or self.cfg.ffn % 256:
                raise ValueError("fp8 GEMMs need hidden and ffn to be multiples of 256")
            if not self._fp8:
                for i in range(n):
                    for w in (self._qkv_w[i], self._ffn1_w[i], self._o_w[i], self._ffn2_w[i]):
                        self._fp8 += list(self._quantize_rows(w))
                self._keep += self._fp8
            for i in range(n):
                L = self._layers[i]
                q8, qs, f8, fs, o8, os_, d8, ds = self._fp8[8 * i: 8 * i + 8]
                L.qkv_w8, L.qkv_wscale, L.ffn1_w8, L.ffn1_wscale = q8.data_ptr(), qs.data_ptr(), f8.data_ptr(), fs.data_ptr()
                L.o_w8, L.o_wscale, L.ffn2_w8, L.ffn2_wscale = o8.data_ptr(), os_.data_ptr(), d8.data_ptr(), ds.data_ptr()
                L.ffn_act_scale = float(self.ffn_act_scales[i]) if self.ffn_act_scales else 0.0
        else:
            for i in range(n):
                L = self._layers[i]
                L.qkv_w8 = L.qkv_wscale = L.ffn1_w8 = L.ffn1_wscale = None
                L.o_w8 = L.o_wscale = L.ffn2_w8 = L.ffn2_wscale = None
                L.ffn_act_scale = 0.0
        self.gemm_dtype = dtype

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """HF checkpoint name -> the resident (bf16 / fp32) tensor: what these weights ARE after rounding to bf16,
        e.g. to run the same model through the fp32 path (``encoder_f32.EncoderWeightsF32(cfg, w.state_dict(), dev)``)."""
        return dict(self._named)


def synthetic_state(cfg: EncoderConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random-init weights of the given architecture (HF init: normal(0, 0.02);
    LayerNorm gamma/beta perturbed).  Same generator sequence as the test oracle's
    ``synth_weights`` so parity tests can rebuild identical weights from a seed."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, std=0.02: (torch.randn(*s, generator=g) * std)  # noqa: E731
    H, F = cfg.hidden, cfg.ffn
    W = {
        "embeddings.word_embeddings.weight": n(cfg.vocab_size, H),
        "embeddings.position_embeddings.weight": n(cfg.max_pos, H),
        "embeddings.token_type_embeddings.weight": n(cfg.type_vocab, H),
        "embeddings.LayerNorm.weight": 1.0 + n(H, std=0.1),
        "embeddings.LayerNorm.bias": n(H, std=0.05),
    }
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        for nm in ("query", "key", "value"):
            W[p + f"attention.self.{nm}.weight"] = n(H, H)
            W[p + f"attention.self.{nm}.bias"] = n(H)
        W[p + "attention.output.dense.weight"] = n(H, H)
        W[p + "attention.output.dense.bias"] = n(H)
        W[p + "attention.output.LayerNorm.weight"] = 1.0 + n(H, std=0.1)
        W[p + "attention.output.LayerNorm.bias"] = n(H, std=0.05)
        W[p + "intermediate.dense.weight"] = n(F, H)
        W[p + "intermediate.dense.bias"] = n(F)
        W[p + "output.dense.weight"] = n(H, F)
        W[p + "output.dense.bias"] = n(H)
        W[p + "output.LayerNorm.weight"] = 1.0 + n(H, std=0.1)
        W[p + "output.LayerNorm.bias"] = n(H, std=0.05)
    if cfg.num_labels:
        W["classifier.dense.weight"] = n(H, H)
        W["classifier.dense.bias"] = n(H)
        W["classifier.out_proj.weight"] = n(cfg.num_labels, H, std=0.2)
        W["classifier.out_proj.bias"] = n(cfg.num_labels)
    return W


def synthetic_state_device(cfg: EncoderConfig, device: torch.device, seed: int = 0,
                           dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """Random-init weights generated directly on the device (benchmarks: avoids building a
    2.3 GB fp32 model on the host).  Not reproducible against the CPU oracle.  ``dtype=torch.float32`` keeps the
    matrices unrounded (the reference-precision legs: their lo planes must not be all zero)."""
    g = torch.Generator(device=device).manual_seed(seed)
    n = lambda *s, std=0.02: (torch.randn(*s, generator=g, device=device) * std).to(dtype)  # noqa: E731
    H, F = cfg.hidden, cfg.ffn
    W = {
        "embeddings.word_embeddings.weight": n(cfg.vocab_size, H),
        "embeddings.position_embeddings.weight": n(cfg.max_pos, H),
        "embeddings.token_type_embeddings.weight": n(cfg.type_vocab, H),
        "embeddings.LayerNorm.weight": 1.0 + n(H, std=0.1).float(),
        "embeddings.LayerNorm.bias": n(H, std=0.05).float(),
    }
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        for nm in ("query", "key", "value"):
            W[p + f"attention.self.{nm}.weight"] = n(H, H)
            W[p + f"attention.self.{nm}.bias"] = n(H).float()
        W[p + "attention.output.dense.weight"] = n(H, H)
        W[p + "attention.output.dense.bias"] = n(H).float()
        W[p + "attention.output.LayerNorm.weight"] = 1.0 + n(H, std=0.1).float()
        W[p + "attention.output.LayerNorm.bias"] = n(H, std=0.05).float()
        W[p + "intermediate.dense.weight"] = n(F, H)
        W[p + "intermediate.dense.bias"] = n(F).float()
        W[p + "output.dense.weight"] = n(H, F)
        W[p + "output.dense.bias"] = n(H).float()
        W[p + "output.LayerNorm.weight"] = 1.0 + n(H, std=0.1).float()
        W[p + "output.LayerNorm.bias"] = n(H, std=0.05).float()
    if cfg.num_labels:
        W["classifier.dense.weight"] = n(H, H)
        W["classifier.dense.bias"] = n(H).float()
        W["classifier.out_proj.weight"] = n(cfg.num_labels, H, std=0.2)
        W["classifier.out_proj.bias"] = n(cfg.num_labels).float()
    return W


# Rows between sequence starts are rounded up to this.  8 (default): every sequence owns its V8 token groups, so its
# attention tiles -- and therefore its bits -- do not depend on where it sits in the batch (scores are invariant under
# permuting / splitting a batch: tests/test_configs_gpu.py).  1: back to back, no padding rows at all (the attention
# kernels mask the token group two sequences share): -0.8 % step time on 292-token pairs, more on short texts, at the
# price of one-bf16-ulp differences between placements (a different tiling of the same keys).
_PACK_ALIGN = max(1, int(os.environ.get("TT_PACK_ALIGN", "8")))


@dataclass
class PackedBatch:
    """Varlen packed token batch (host arrays): see include/tt_hip.h 'Token layout'."""

    ids: np.ndarray        # [n_rows] int32
    pos: np.ndarray        # [n_rows] int32
    types: Optional[np.ndarray]
    seq_start: np.ndarray  # [B] int32 (any row is legal for the kernels; multiples of _PACK_ALIGN here)
    seq_len: np.ndarray    # [B] int32
    n_rows: int            # multiple of 128
    max_len: int
    n_tokens: int          # real tokens (sum of seq_len)


def _round_rows(used: int) -> int:
    """Token rows of a batch: a multiple of the 256-row GEMM tile; up to 256 rows (one query, a few short texts) a
    multiple of 64 -- the projections then run as weight-streaming skinny GEMMs (csrc/gemm.hip)."""
    # (TT_GEMM_SKINNY=0: the A/B switch of tools/gpu_skinny.sh -- honoured with the diagnostic library only, like the kernels' own read)
    if used <= 256 and not (_lib.is_diag() and os.environ.get("TT_GEMM_SKINNY", "1") == "0"):
        return max(64, (used + 63) // 64 * 64)
    return (used + 255) // 256 * 256


def pack_tokens(seqs: Sequence[Sequence[int]], cfg: EncoderConfig,
                type_ids: Optional[Sequence[Sequence[int]]] = None, max_len: Optional[int] = None) -> PackedBatch:
    """Pack token-id sequences (already carrying their special tokens) without padding tokens: sequence
    starts are aligned to ``_PACK_ALIGN`` rows (8 by default, see above), the total to the 256-row GEMM tile.  Sequences longer
    than ``max_len`` (default: the model's limit) are truncated on the right, as the
    reference's tokenizer call does (``truncation=True``)."""
    limit = cfg.max_seq_len if max_len is None else min(max_len, cfg.max_seq_len)
    n_seq = len(seqs)
    lens = np.fromiter((min(len(s), limit) for s in seqs), dtype=np.int64, count=n_seq)
    if n_seq == 0 or (lens <= 0).any():
        raise ValueError("empty token sequence")
    # no per-sequence Python work below: one flat copy of all tokens and one scatter (a 100k-document ingest packs ~10^7
    # sequences; the per-sequence slice / arange loop was a third of the host time of an ingest batch)
    aligned = (lens + _PACK_ALIGN - 1) // _PACK_ALIGN * _PACK_ALIGN
    starts = np.zeros(n_seq, dtype=np.int64)
    np.cumsum(aligned[:-1], out=starts[1:])
    n_rows = _round_rows(int(aligned.sum()))
    total = int(lens.sum())

    def flat_of(rows) -> np.ndarray:
        if all(isinstance(r, np.ndarray) for r in rows):
            return np.concatenate([np.asarray(r[:n], dtype=np.int32) for r, n in zip(rows, lens)]) if n_seq > 1 else \
                np.asarray(rows[0][: lens[0]], dtype=np.int32)
        return np.fromiter(itertools.chain.from_iterable(r if len(r) == n else r[:n] for r, n in zip(rows, lens)),
                           dtype=np.int32, count=total)

    first = np.zeros(n_seq, dtype=np.int64)
    np.cumsum(lens[:-1], out=first[1:])
    within = np.arange(total, dtype=np.int64) - np.repeat(first, lens)
    dest = np.repeat(starts, lens) + within
    flat = flat_of(seqs)
    if flat.min() < 0 or flat.max() >= cfg.vocab_size:
        raise ValueError("token id outside the vocabulary")
    ids = np.full(n_rows, cfg.pad_id, dtype=np.int32)
    pos = np.zeros(n_rows, dtype=np.int32)
    pos_off = cfg.pad_id + 1 if cfg.arch in ("xlmr", "mpnet") else 0
    ids[dest] = flat
    pos[dest] = within + pos_off
    types = None
    if type_ids is not None:
        types = np.zeros(n_rows, dtype=np.int32)
        types[dest] = flat_of(type_ids)
    return PackedBatch(ids, pos, types, starts.astype(np.int32), lens.astype(np.int32), int(n_rows),
                       int(lens.max()), total)


def pack_flat(flat: np.ndarray, first: np.ndarray, lens: np.ndarray, sel: np.ndarray, cfg: EncoderConfig,
              max_len: Optional[int] = None) -> PackedBatch:
    """``pack_tokens([sequence i for i in sel])`` for sequences given as ONE flat int32 array (sequence i = ``flat[first[i] : first[i] +
    lens[i]]``): no per-sequence Python at all -- the ingest feeder packs ~10^7 sequences per 100 000 documents, and the list of
    per-sequence arrays ``pack_tokens`` takes cost it 40 us per sequence (a quarter of a 100 000-document build, round 5)."""
    limit = cfg.max_seq_len if max_len is None else min(max_len, cfg.max_seq_len)
    sel = np.asarray(sel, dtype=np.int64)
    n_seq = len(sel)
    ln = np.minimum(lens[sel].astype(np.int64), limit)
    if n_seq == 0 or (ln <= 0).any():
        raise ValueError("empty token sequence")
    aligned = (ln + _PACK_ALIGN - 1) // _PACK_ALIGN * _PACK_ALIGN
    starts = np.zeros(n_seq, dtype=np.int64)
    np.cumsum(aligned[:-1], out=starts[1:])
    n_rows = _round_rows(int(aligned.sum()))
    total = int(ln.sum())
    local_first = np.zeros(n_seq, dtype=np.int64)
    np.cumsum(ln[:-1], out=local_first[1:])
    within = np.arange(total, dtype=np.int64) - np.repeat(local_first, ln)
    src = np.repeat(first[sel].astype(np.int64), ln) + within
    dest = np.repeat(starts, ln) + within
    vals = flat[src]
    if vals.min() < 0 or vals.max() >= cfg.vocab_size:
        raise ValueError("token id outside the vocabulary")
    ids = np.full(n_rows, cfg.pad_id, dtype=np.int32)
    pos = np.zeros(n_rows, dtype=np.int32)
    pos_off = cfg.pad_id + 1 if cfg.arch in ("xlmr", "mpnet") else 0
    ids[dest] = vals
    pos[dest] = within + pos_off
    return PackedBatch(ids, pos, None, starts.astype(np.int32), ln.astype(np.int32), int(n_rows), int(ln.max()), total)


def pack_token_matrix(ids2d: np.ndarray, cfg: EncoderConfig, type_ids2d: Optional[np.ndarray] = None) -> PackedBatch:
    """Vectorised ``pack_tokens`` for sequences of one common length (rows of ``ids2d``): no Python
    loop, so host packing of a few thousand rerank pairs stays in the 100-microsecond range."""
    ids2d = np.ascontiguousarray(ids2d, dtype=np.int32)
    n, length = ids2d.shape
    if n == 0 or length == 0:
        raise ValueError("empty token matrix")
    if length > cfg.max_seq_len:
        ids2d = ids2d[:, : cfg.max_seq_len]
        length = cfg.max_seq_len
    stride = (length + _PACK_ALIGN - 1) // _PACK_ALIGN * _PACK_ALIGN
    n_rows = _round_rows(n * stride)
    ids = np.full(n_rows, cfg.pad_id, dtype=np.int32)
    pos = np.zeros(n_rows, dtype=np.int32)
    pos_off = cfg.pad_id + 1 if cfg.arch in ("xlmr", "mpnet") else 0
    view = ids[: n * stride].reshape(n, stride)
    view[:, :length] = ids2d
    pos[: n * stride].reshape(n, stride)[:, :length] = np.arange(length, dtype=np.int32) + pos_off
    types = None
    if type_ids2d is not None:
        types = np.zeros(n_rows, dtype=np.int32)
        types[: n * stride].reshape(n, stride)[:, :length] = np.asarray(type_ids2d, dtype=np.int32)[:, :length]
    if ids2d.min() < 0 or ids2d.max() >= cfg.vocab_size:
        raise ValueError("token id outside the vocabulary")
    starts = (np.arange(n, dtype=np.int64) * stride).astype(np.int32)
    lens = np.full(n, length, dtype=np.int32)
    return PackedBatch(ids, pos, types, starts, lens, int(n_rows), int(length), int(n * length))


def pooled_rows(batch: PackedBatch, pad_token_id: Optional[int] = None) -> np.ndarray:
    """-> int32 [B]: the absolute row of the token a decoder's one-row-per-sequence tail keeps for each sequence of ``batch``.
    transformers' rule for ``*ForSequenceClassification`` decoders, restated: with ``pad_token_id`` set, the RIGHTMOST token whose
    id differs from it -- position 0 if the sequence holds nothing else -- and with ``pad_token_id`` None the last token (what
    last-token pooling reads too).  Causal attention makes the tokens behind the pooled one irrelevant to it.  One vectorised
    pass over the ids of the batch as packed (i.e. after truncation)."""
    starts, lens = batch.seq_start.astype(np.int64), batch.seq_len.astype(np.int64)
    if pad_token_id is None:
        return (starts + lens - 1).astype(np.int32)
    first = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(lens[:-1], out=first[1:])
    within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(first, lens)
    keep = batch.ids[np.repeat(starts, lens) + within] != pad_token_id
    return (starts + np.maximum.reduceat(np.where(keep, within, 0), first)).astype(np.int32)


class _Scratch:
    """Workspace buffers keyed by (kind, device, HIP stream): launches on one stream execute in order, so every
    forward enqueued on that stream can reuse ONE buffer -- whichever host thread enqueues it -- as long as a whole
    forward is enqueued atomically (``Encoder._enqueue_lock``; two threads interleaving their launches over one
    workspace would corrupt both).  Bounded by the largest batch per stream, not by the number of request threads
    (per-thread buffers of 5-20 GB each would not fit 32 executor threads).  Growing frees the old buffer through
    torch's stream-ordered caching allocator, which is safe for work already enqueued on the same stream."""

    def __init__(self):
        self.bufs = {}
        self.lock = threading.Lock()

    def get(self, key, device, nbytes):
        stream = torch.cuda.current_stream(device).cuda_stream
        k = (key, device.type, device.index, stream)
        with self.lock:
            buf = self.bufs.get(k)
            if buf is None or buf.numel() < nbytes + 256:
                buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
                self.bufs[k] = buf
        base = (buf.data_ptr() + 255) // 256 * 256
        return buf, base


_scratch = _Scratch()
_ENQUEUE_LOCKS: Dict[Tuple[str, Optional[int]], threading.Lock] = {}


class _Stager:
    """Ring of pinned host buffers for the token arrays of a batch, shared by all threads of the process.  One buffer
    holds every array of one batch, goes to the device in ONE asynchronous copy on the compute stream, and is reused
    once the event recorded behind that copy has fired -- so the host can pack and enqueue batch i+1 (and tokenize
    batch i+2) while the GPU is still computing batch i.  Process-wide rather than per
    thread: pinning memory costs milliseconds per allocation, and under the coalescing front every request thread
    leads a batch now and then (32 executor threads x their own rings = 128 pinned allocations on the hot path)."""

    SLOTS = 8

    def __init__(self):
        self.slots = []
        self.cursor = 0
        self.lock = threading.Lock()

    def acquire(self, nbytes: int):
        """-> a slot whose ``lock`` is HELD: the caller fills ``buf``, issues the copy, records ``ev`` and releases it."""
        with self.lock:
            if len(self.slots) < self.SLOTS:
                self.slots.append({"buf": None, "ev": None, "lock": threading.Lock()})
                slot = self.slots[-1]
            else:
                slot = self.slots[self.cursor % self.SLOTS]
            self.cursor += 1
        slot["lock"].acquire()
        if slot["ev"] is not None:
            slot["ev"].synchronize()  # eight batches later: long fired
            slot["ev"] = None
        if slot["buf"] is None or slot["buf"].numel() < nbytes:
            slot["buf"] = torch.empty(max(nbytes, 4 << 20), dtype=torch.uint8, pin_memory=True)
        return slot


_stager = _Stager()


def _pad_rows(batch: PackedBatch, multiple: int, skinny: bool) -> PackedBatch:
    """``batch`` with its rows rounded up to a multiple of ``multiple`` (the tiled GEMMs of a path run whole tiles), padding
    with the last token id and position 0.  ``skinny``: up to 256 rows in multiples of 64 stay as they are -- the projections
    then run as weight-streaming skinny GEMMs (``_round_rows`` packs exactly that)."""
    if skinny and batch.n_rows <= 256 and batch.n_rows % 64 == 0:
        return batch
    n = (batch.n_rows + multiple - 1) // multiple * multiple
    if n == batch.n_rows:
        return batch

    def pad(a, fill):
        if a is None:
            return None
        out = np.full(n, fill, dtype=a.dtype)
        out[: a.size] = a
        return out

    return dataclasses.replace(batch, ids=pad(batch.ids, batch.ids[-1] if batch.ids.size else 0), pos=pad(batch.pos, 0),
                               types=pad(batch.types, 0), n_rows=n)


class Encoder:
    """Runs the HIP encoder for one set of weights, on the path they carry (``weights.path``)."""

    def __init__(self, weights: _CheckpointWeights):
        self.w = weights
        self.cfg = weights.cfg
        self.device = weights.device
        self.path = weights.path
        self.lib = _lib.load_library()
        # one forward (scratch lookup + every launch of it) is enqueued atomically: the workspace is shared per stream
        self._enqueue_lock = _ENQUEUE_LOCKS.setdefault((self.device.type, self.device.index), threading.Lock())

    def _upload(self, batch: PackedBatch, *more: np.ndarray):
        """Token arrays of a batch -> device int32 views (ids, pos, types | None, seq_start, seq_len, and one per int32 array of
        ``more``: the pooled rows of a decoder's tail): one pinned staging buffer, one asynchronous host-to-device copy on the
        current stream."""
        parts = [batch.ids, batch.pos, batch.types, batch.seq_start, batch.seq_len, *more]
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            if a is not None:
                total += (a.size + 63) // 64 * 64          # 256-byte aligned sub-arrays
        slot = _stager.acquire(total * 4)
        try:
            host = slot["buf"][: total * 4].view(torch.int32)
            hn = host.numpy()
            for a, o in zip(parts, offs):
                if a is not None:
                    hn[o:o + a.size] = a
            with torch.cuda.device(self.device):
                devbuf = torch.empty(total, dtype=torch.int32, device=self.device)
                devbuf.copy_(host, non_blocking=True)
                slot["ev"] = torch.cuda.Event()
                slot["ev"].record(torch.cuda.current_stream(self.device))
        finally:
            slot["lock"].release()
        return tuple(devbuf[o:o + a.size] if a is not None else None for a, o in zip(parts, offs))

    def _padded(self, batch: PackedBatch) -> PackedBatch:
        return _pad_rows(batch, self.path.row_tile, self.path.skinny) if self.path.row_tile else batch

    def _run(self, name: str, workspace: str, batch: PackedBatch, out_rows: int, *ws_args):
        """Upload ``batch`` and enqueue the forward entry point ``name`` (sized by ``workspace(struct, n_rows, *ws_args)``)
        -> (its output [out_rows, H] in the path's hidden dtype, seq_start, seq_len device tensors)."""
        dev, w = self.device, ctypes.byref(self.w.struct)
        ids, pos, types, starts, lens = self._upload(batch)
        out = torch.empty((out_rows, self.cfg.hidden), dtype=self.path.hidden, device=dev)
        need = getattr(self.lib, workspace)(w, batch.n_rows, *ws_args)
        with self._enqueue_lock, torch.cuda.device(dev):
            ws, base = _scratch.get(self.path.scratch, dev, need)
            rc = getattr(self.lib, name)(w, ids.data_ptr(), pos.data_ptr(), types.data_ptr() if types is not None else None,
                                         starts.data_ptr(), lens.data_ptr(), len(batch.seq_len), batch.n_rows, batch.max_len,
                                         out.data_ptr(), base, need, torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, name)
        return out, starts, lens

    def forward_packed(self, batch: PackedBatch, want_lens: bool = False):
        """-> (hidden [n_rows, H] (the weights' dtype on the 16-bit path, fp32 elsewhere), seq_start [B] int32 device
        tensor[, seq_len [B] int32 device tensor]); ``n_rows`` after the path's padding."""
        batch = self._padded(batch)
        hidden, starts, lens = self._run(self.path.forward, self.path.workspace, batch, batch.n_rows)
        return (hidden, starts, lens) if want_lens else (hidden, starts)

    def calibrate_fp8(self, batch: PackedBatch, margin: float = 2.0) -> List[float]:
        """One bf16 forward over ``batch`` that records max |GELU output| per layer (``ffn_absmax_out`` hook) and sets
        the static e4m3 scales of the FFN intermediate, ``margin * max / 448`` (values beyond saturate).  Call before
        ``weights.set_gemm_dtype("fp8")`` to move the FFN output projection to fp8 as well."""
        if self.path.no_fp8:
            raise RuntimeError(self.path.no_fp8)
        w = self.w
        prev = w.gemm_dtype
        w.set_gemm_dtype("bf16")
        absmax = torch.zeros(max(self.cfg.layers, 1), dtype=torch.float32, device=self.device)
        w.struct.ffn_absmax_out = absmax.data_ptr()
        try:
            self.forward_packed(batch)
            vals = absmax.cpu().tolist()
        finally:
            w.struct.ffn_absmax_out = None
        w.ffn_act_scales = [max(v, 1e-6) * margin / 448.0 for v in vals[: self.cfg.layers]]
        w.set_gemm_dtype(prev)
        return w.ffn_act_scales

    def cls_hidden_packed(self, batch: PackedBatch) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (final hidden state of every sequence's CLS token, row ids [B] int32).  Where the path has a CLS-only forward,
        the last layer is evaluated for the CLS rows only, into [pad(B), H] with rows 0..B-1; otherwise (and for a model
        without layers) this is the full forward and its sequence starts."""
        p = self.path
        if p.cls_forward is None or self.cfg.layers == 0:
            return self.forward_packed(batch)
        B = len(batch.seq_len)
        b_pad = (B + 63) // 64 * 64 if p.skinny and B <= 256 else (B + 255) // 256 * 256
        cls, _, _ = self._run(p.cls_forward, p.cls_workspace, self._padded(batch), b_pad, B)
        return cls, torch.arange(B, dtype=torch.int32, device=self.device)

    def rows_hidden_packed(self, batch: PackedBatch, rows: np.ndarray) -> torch.Tensor:
        """Decoder paths: -> [pad(B), H], row b = the final hidden state of row ``rows[b]`` of ``batch`` (``pooled_rows``), the
        bits the full forward gives that row.  The last layer's attention, output projection and MLP run for those rows only
        (``tt_decoder_forward_rows``); pad(B) as ``cls_hidden_packed`` pads, rows B.. zero."""
        p, dev, w = self.path, self.device, ctypes.byref(self.w.struct)
        if p.rows_forward is None:
            raise RuntimeError("this path has no one-row-per-sequence forward")
        B = len(batch.seq_len)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.shape != (B,) or (rows < batch.seq_start).any() or (rows >= batch.seq_start + batch.seq_len).any():
            raise ValueError("pooled rows: one row inside each sequence is needed")
        batch = self._padded(batch)
        ids, pos, types, starts, lens, pool = self._upload(batch, rows)
        if types is not None:
            raise ValueError("a decoder has no token types")
        out = torch.empty((_round_rows(B), self.cfg.hidden), dtype=p.hidden, device=dev)
        need = getattr(self.lib, p.rows_workspace)(w, batch.n_rows, B)
        with self._enqueue_lock, torch.cuda.device(dev):
            ws, base = _scratch.get(p.scratch, dev, need)
            rc = getattr(self.lib, p.rows_forward)(w, ids.data_ptr(), pos.data_ptr(), None, starts.data_ptr(), lens.data_ptr(), B,
                                                   batch.n_rows, batch.max_len, pool.data_ptr(), out.data_ptr(), base, need,
                                                   torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, p.rows_forward)
        return out

    def _compact_rows(self, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(0 .. n-1, ones) as int32 device tensors: the ``seq_start`` / ``seq_len`` under which the pooling kernels read row b of a
        compact [B, H] buffer for sequence b.  Built once per size class, on the stream that first asks."""
        have = getattr(self, "_compact", None)
        if have is None or have[0].numel() < n:
            cap = max(1024, 1 << (n - 1).bit_length())
            have = (torch.arange(cap, dtype=torch.int32, device=self.device), torch.ones(cap, dtype=torch.int32, device=self.device))
            torch.cuda.current_stream(self.device).synchronize()      # (once per size class: other streams read them later)
            self._compact = have
        return have[0][:n], have[1][:n]

    def embed_packed(self, batch: PackedBatch, pooling: str = "cls", skip: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (embeddings fp32 [B, H] L2-normalised, same rounded to bf16).  ``pooling``: "cls" (the BGE family: the last layer
        runs for the CLS rows only), "mean" (sentence-transformers mean pooling over a sequence's tokens: full last layer) or
        "last" (the last token of every sequence: decoder embedders).  ``skip`` (T5 path: a checkpoint whose Pooling module says
        ``include_prompt: false``): the first ``skip`` tokens of every sequence -- its instruction -- stay out of the mean."""
        p, dev = self.path, self.device
        B, H = len(batch.seq_len), self.cfg.hidden
        if skip and self.cfg.arch != "t5":
            raise ValueError("a prompt is left out of the mean on the T5 path only")
        if p.pool_dense is not None:
            # EmbeddingGemma: the checkpoint's own tail (mean pooling -> Dense -> Dense -> Normalize) behind the full forward; T5:
            # mean pooling -> Dense (where the checkpoint has one) -> Normalize
            if pooling != "mean":
                if self.cfg.arch == "t5":
                    raise ValueError(f"pooling '{pooling}': a T5 encoder checkpoint pools the mean (its Dense module follows it)")
                raise ValueError(f"pooling '{pooling}': an EmbeddingGemma checkpoint pools the mean (its Dense modules follow it)")
            ranges = None
            if skip:
                from .t5 import pooled_ranges

                ranges = pooled_ranges(batch.seq_start, batch.seq_len, skip)     # (raises before anything is enqueued)
            hidden, starts, lens = self.forward_packed(batch, want_lens=True)
            if ranges is not None:
                both = torch.from_numpy(np.concatenate(ranges)).to(dev)
                starts, lens = both[:B], both[B:]
            out = torch.empty((B, self.w.out_dim), dtype=torch.float32, device=dev)
            out16 = torch.empty((B, self.w.out_dim), dtype=torch.bfloat16, device=dev)
            with torch.cuda.device(dev):
                rc = getattr(self.lib, p.pool_dense)(ctypes.byref(self.w.struct), hidden.data_ptr(), H, starts.data_ptr(),
                                                     lens.data_ptr(), B, out.data_ptr(), out16.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(rc, p.pool_dense)
            return out, out16
        out = torch.empty((B, H), dtype=torch.float32, device=dev)
        # the 16-bit copy of an embedding is a SCAN QUERY, i.e. bf16 like the corpus: the pooling kernels write it themselves,
        # except in the fp16 mode, where it is rounded from the fp32 vector here (round to nearest even either way)
        out16 = torch.empty((B, H), dtype=torch.bfloat16, device=dev) if p.pool_writes_bf16 else None
        if pooling == "mean":
            hidden, starts, lens = self.forward_packed(batch, want_lens=True)
            name, rows = p.pool_mean, (starts.data_ptr(), lens.data_ptr())
        elif pooling == "last":
            if p.pool_last is None:
                raise ValueError("last-token pooling needs a decoder path")
            # the last layer for the last tokens only: the same bits as the full forward's rows, pooled from compact row b
            hidden = self.rows_hidden_packed(batch, pooled_rows(batch))
            starts, lens = self._compact_rows(B)
            name, rows = p.pool_last, (starts.data_ptr(), lens.data_ptr())
        elif pooling == "cls":
            hidden, cls_rows = self.cls_hidden_packed(batch)
            name, rows = p.pool, (cls_rows.data_ptr(),)
        else:
            raise ValueError(f"pooling '{pooling}' (supported: 'cls', 'mean', 'last')")
        with torch.cuda.device(dev):
            rc = getattr(self.lib, name)(hidden.data_ptr(), H, *rows, B, H, out.data_ptr(),
                                         out16.data_ptr() if out16 is not None else None, torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, name)
        return out, (out16 if out16 is not None else out.to(torch.bfloat16))

    def rerank_packed(self, batch: PackedBatch, want_logits: bool = False):
        """-> sigmoid scores fp32 [B] (and logits)."""
        if not self.cfg.num_labels:
            raise RuntimeError("these weights carry no classification head")
        p, dev = self.path, self.device
        B, H = len(batch.seq_len), self.cfg.hidden
        scores = torch.empty(B, dtype=torch.float32, device=dev)
        logits = torch.empty(B, dtype=torch.float32, device=dev) if want_logits else None
        if p.score is not None:
            # decoder reranker: the score head reads the pooled token's row of the one-row-per-sequence tail
            hidden = self.rows_hidden_packed(batch, pooled_rows(batch, self.cfg.pad_token_id))
            with torch.cuda.device(dev):
                rc = getattr(self.lib, p.score)(hidden.data_ptr(), H, self.w.score_w.data_ptr(), B, H, scores.data_ptr(),
                                                logits.data_ptr() if want_logits else None, torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(rc, p.score)
            return (scores, logits) if want_logits else scores
        if p.pooled_head is not None:
            # ModernBERT cross-encoder: the head pools the full forward's rows as the checkpoint says and scores them (a DeBERTa
            # cross-encoder's reads the first rows: it has no ``classifier_pooling``)
            hidden, starts, lens = self.forward_packed(batch, want_lens=True)
            with torch.cuda.device(dev):
                rc = getattr(self.lib, p.pooled_head)(ctypes.byref(self.w.struct), hidden.data_ptr(), H, starts.data_ptr(),
                                                      lens.data_ptr(), B, 1 if getattr(self.cfg, "classifier_pooling", "cls") == "mean" else 0,
                                                      scores.data_ptr(), logits.data_ptr() if want_logits else None,
                                                      torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(rc, p.pooled_head)
            return (scores, logits) if want_logits else scores
        hidden, cls_rows = self.cls_hidden_packed(batch)
        n_pad = (B + 127) // 128 * 128
        need = 2 * ((n_pad * H * hidden.element_size() + 255) // 256 * 256)
        with self._enqueue_lock, torch.cuda.device(dev):
            ws, base = _scratch.get(p.head_scratch, dev, need)
            rc = getattr(self.lib, p.head)(ctypes.byref(self.w.struct), hidden.data_ptr(), cls_rows.data_ptr(), B,
                                           scores.data_ptr(), logits.data_ptr() if want_logits else None, base, need,
                                           torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, p.head)
        return (scores, logits) if want_logits else scores

    # -- convenience over python lists -------------------------------------------------------
    def embed(self, seqs, type_ids=None, max_len=None):
        return self.embed_packed(pack_tokens(seqs, self.cfg, type_ids, max_len))

    def rerank(self, seqs, max_len: Optional[int] = 512, want_logits: bool = False):
        return self.rerank_packed(pack_tokens(seqs, self.cfg, None, max_len), want_logits)
