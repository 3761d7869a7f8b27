"""Late-interaction (ColBERT) reranking and exact retrieval on the HIP path: ``colbert-ir/colbertv2.0`` (768 -> 128),
``answerdotai/answerai-colbert-small-v1`` (384, 32-wide heads -> 96) and the same models in PyLate's sentence-transformers layout.

A cross-encoder pushes every (query, passage) pair through the whole encoder at query time.  A late-interaction model encodes a
passage ONCE, when it is indexed, to one L2-normalised vector per kept token (``TokenVectorStore``, in HBM); at query time only the
query runs through the encoder and every candidate is scored by MaxSim, ``sum_i max_j <q_i, d_j>``, over vectors already resident
(``tt_maxsim``) -- or every stored passage is, in one read of the store (``tt_maxsim_scan_topk``, ``HipColbertRetriever``).  The encoder is the BERT forward of the 16-bit path (``tt_encoder_forward[_f16]``); a query is padded with
``[MASK]`` tokens that are encoded and scored but -- unless the checkpoint says otherwise -- never attended to
(``tt_encoder_forward_keylen``); the per-token projection and normalisation is ``tt_colbert_project``.  bf16 (default) or fp16.

Token layout (the contract; restated against installed classes by tests/golden/make_colbert_golden.py):

    query      [CLS] Q body... [SEP] [MASK]... up to ``query_length``; the body is truncated so that the total fits; positions
               0 .. L-1, token types 0; ``key_len`` = the unpadded length (``attend_to_expansion_tokens``: the plain forward);
               all L rows are projected and scored
    document   [CLS] D body... [SEP], truncated to ``document_length``, the plain forward; rows whose token id is in the
               skiplist are not projected ([CLS], the marker and [SEP] are kept)

[UPSTREAM-K] Field and tensor names of both directory layouts are written from knowledge of the upstream projects (stanford
ColBERT's ``artifact.metadata`` and ``bert.* + linear.weight`` state dict; PyLate's ``modules.json`` / ``1_Dense`` /
``config_sentence_transformers.json``), which are not installed here and cannot be checked offline.  The loader is therefore strict:
a tensor or a setting it does not know is refused by name, and a setting it needs is never defaulted silently.
"""
from __future__ import annotations

import ctypes
import functools
import json
import logging
import os
import re
import string
from dataclasses import dataclass, field
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._hostargs import _check_range, _dev_i, _need_device, _stream, _suffix, grown, read_json, resolve_device
from ._hostargs import resolve_dtype as _resolve_dtype
from ._stored import IdTable, _StoredRerank, top_nodes
from .encoder import Encoder, EncoderConfig, EncoderWeights, _scratch, pack_tokens

logger = logging.getLogger(__name__)

MAX_QUERY_LEN, MAX_DOC_LEN, MAX_DIM = 128, 512, 128      # tt_maxsim's limits (include/tt_hip.h)
MAX_SCAN_QUERIES, MAX_SCAN_K = 64, 1024                  # tt_maxsim_scan_topk's (queries per call, k)


# ---- settings ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ColbertConfig:
    """What the two layouts agree on once parsed.  ``layout`` ("stanford" / "pylate") is informational and not compared."""

    query_length: int
    document_length: int
    dim: int
    attend_to_expansion_tokens: bool
    query_marker: int            # token id of Q
    document_marker: int         # token id of D
    cls_id: int
    sep_id: int
    mask_id: int
    skiplist: Tuple[int, ...]    # sorted token ids whose document rows are not projected
    layout: str = field(default="stanford", compare=False)


# stanford ColBERTConfig fields that play no part in serving a checkpoint ([UPSTREAM-K]: colbert/infra/config/settings.py)
_STANFORD_UNUSED = frozenset("""overwrite root experiment index_root name rank nranks amp gpus avoid_fork_if_possible query_token doc_token
checkpoint triples collection queries index_name bsize accumsteps lr maxsteps save_every resume warmup warmup_bert relu nway
use_ib_negatives reranker distillation_alpha ignore_scores model_name index_path index_bsize nbits kmeans_niters pool_factor
clustering_mode protected_tokens ncells centroid_score_threshold ndocs load_index_with_mmap meta""".split())
_STANFORD_READ = frozenset(("query_maxlen", "doc_maxlen", "dim", "mask_punctuation", "attend_to_mask_tokens", "similarity",
                            "interaction", "query_token_id", "doc_token_id"))
# PyLate config_sentence_transformers.json ([UPSTREAM-K]: pylate/models/colbert.py, sentence-transformers' own keys)
_PYLATE_UNUSED = frozenset(("__version__", "prompts", "default_prompt_name", "model_type"))
_PYLATE_READ = frozenset(("query_prefix", "document_prefix", "query_length", "document_length", "attend_to_expansion_tokens",
                          "skiplist_words", "similarity_fn_name", "do_query_expansion"))
# model_kwargs names: the PyLate spelling, and the stanford one as an alias
_ALIASES = {"query_length": "query_maxlen", "document_length": "doc_maxlen", "attend_to_expansion_tokens": "attend_to_mask_tokens"}


def detect_layout(model_dir: Optional[str]) -> Optional[str]:
    """"stanford" for a directory with ``artifact.metadata``, "pylate" for one whose ``modules.json`` names a Dense module and no
    Pooling (a late-interaction model keeps every token), else None -- what ``ModelManager`` dispatches on."""
    if not model_dir or not os.path.isdir(model_dir):
        return None
    if os.path.exists(os.path.join(model_dir, "artifact.metadata")):
        return "stanford"
    mj = os.path.join(model_dir, "modules.json")
    if os.path.exists(mj):
        try:
            with open(mj, encoding="utf-8") as f:
                types = [str(m.get("type", "")) for m in json.load(f)]
        except (OSError, ValueError, AttributeError):
            return None
        if any(t.rsplit(".", 1)[-1] == "Dense" for t in types) and not any(t.rsplit(".", 1)[-1] == "Pooling" for t in types):
            return "pylate"
    return None


class _Vocabulary:
    """What the layout needs from a tokenizer: a text's body ids (no specials) and the id of a token string."""

    def __init__(self, tk):
        self.tk = tk
        hf = getattr(tk, "tk", None)           # tokenization.HFTokenizer wraps a ``tokenizers.Tokenizer``
        self._hf = hf
        if hf is None:                         # the hashing stand-in of synthetic weights: bert-base-uncased's special ids
            sp = tk.sp
            self._fixed = {"[CLS]": sp.bos, "[SEP]": sp.eos, "[MASK]": 103, "[unused0]": 1, "[unused1]": 2}

    def token_id(self, token: str) -> Optional[int]:
        if self._hf is None:
            return self._fixed.get(token)
        return self._hf.token_to_id(token)

    def single_token(self, text: str) -> Optional[int]:
        """The id of ``text`` when it is exactly one token of the vocabulary, else None."""
        tid = self.token_id(text)
        if tid is not None:
            return tid
        if self._hf is None:
            return None
        ids = self._hf.encode(text, add_special_tokens=False).ids
        return ids[0] if len(ids) == 1 else None

    def body(self, text: str) -> List[int]:
        if self._hf is None:
            return self.tk._ids(text)
        return self._hf.encode(text, add_special_tokens=False).ids


def _setting(name: str, mk: dict, files: dict, file_key: str, where: str):
    """``model_kwargs`` wins over the files; a setting neither gives is refused by name."""
    for key in (name, _ALIASES.get(name)):
        if key is not None and mk.get(key) is not None:
            return mk[key]
    if files.get(file_key) is not None:
        return files[file_key]
    raise ValueError(f"ColBERT setting '{name}' is missing: {where} has no '{file_key}' and model_kwargs['{name}'] is not given "
                     "(it is never defaulted)")


def parse_settings(model_dir: Optional[str], vocab: "_Vocabulary", model_kwargs: Optional[dict] = None,
                   dense_out: Optional[int] = None) -> ColbertConfig:
    """The checkpoint directory's settings (either layout; ``model_dir`` None: everything from ``model_kwargs``) ->
    ``ColbertConfig``.  ``dense_out``: rows of the projection matrix, which is what ``dim`` must equal."""
    mk = dict(model_kwargs or {})
    layout = detect_layout(model_dir)
    files: Dict[str, Any] = {}
    if layout == "stanford":
        where = "artifact.metadata"
        files = read_json(os.path.join(model_dir, where))
        unknown = sorted(set(files) - _STANFORD_READ - _STANFORD_UNUSED)
        if unknown:
            raise NotImplementedError(f"artifact.metadata carries fields the ColBERT path does not know: {unknown[:6]}")
        if files.get("interaction", "colbert") != "colbert":
            raise NotImplementedError(f"artifact.metadata interaction={files['interaction']!r}: only 'colbert' (MaxSim) is computed")
    elif layout == "pylate":
        where = "config_sentence_transformers.json"
        p = os.path.join(model_dir, where)
        files = read_json(p) if os.path.exists(p) else {}
        unknown = sorted(set(files) - _PYLATE_READ - _PYLATE_UNUSED)
        if unknown:
            raise NotImplementedError(f"{where} carries fields the ColBERT path does not know: {unknown[:6]}")
        if files.get("do_query_expansion", True) is not True:
            raise NotImplementedError(f"{where} do_query_expansion={files['do_query_expansion']!r}: queries are padded with [MASK] here")
        fn = files.get("similarity_fn_name")
        if fn is not None and str(fn).lower() != "maxsim":
            raise NotImplementedError(f"{where} similarity_fn_name={fn!r}: only MaxSim is computed")
    else:
        where = "model_kwargs"
        layout = str(mk.get("layout", "stanford"))

    stanford = layout == "stanford"
    qlen = int(_setting("query_length", mk, files, "query_maxlen" if stanford else "query_length", where))
    dlen = int(_setting("document_length", mk, files, "doc_maxlen" if stanford else "document_length", where))
    attend = _setting("attend_to_expansion_tokens", mk, files, "attend_to_mask_tokens" if stanford else "attend_to_expansion_tokens",
                      where)
    if not isinstance(attend, bool):
        raise ValueError(f"ColBERT setting 'attend_to_expansion_tokens'={attend!r} must be true or false")
    if stanford:
        sim = _setting("similarity", mk, files, "similarity", where)
        dim = int(_setting("dim", mk, files, "dim", where))
    else:
        sim = mk.get("similarity", "cosine")      # (a PyLate model's vectors are normalised by construction)
        dim = int(mk["dim"]) if mk.get("dim") is not None else dense_out
        if dim is None:
            raise ValueError("ColBERT setting 'dim' is missing: no Dense module and model_kwargs['dim'] is not given")
    if str(sim) != "cosine":
        raise NotImplementedError(f"ColBERT similarity={sim!r}: only 'cosine' (normalised token vectors, MaxSim of dot products) "
                                  "is computed")
    if dense_out is not None and dim != dense_out:
        raise ValueError(f"ColBERT dim={dim} does not match the projection matrix ({dense_out} rows)")
    if dim <= 0 or dim % 32 or dim > MAX_DIM:
        raise NotImplementedError(f"ColBERT dim={dim}: a multiple of 32 up to {MAX_DIM}")
    if not 4 <= qlen <= MAX_QUERY_LEN:
        raise NotImplementedError(f"ColBERT query_length={qlen}: 4 .. {MAX_QUERY_LEN}")
    if not 3 <= dlen <= MAX_DOC_LEN:
        raise NotImplementedError(f"ColBERT document_length={dlen}: 3 .. {MAX_DOC_LEN}")

    def need(token: str) -> int:
        tid = vocab.token_id(token)
        if tid is None:
            raise ValueError(f"the tokenizer has no {token} token")
        return tid

    cls_id, sep_id, mask_id = need("[CLS]"), need("[SEP]"), need("[MASK]")
    if stanford:
        qtok = str(mk.get("query_prefix") or files.get("query_token_id") or "[unused0]")
        dtok = str(mk.get("document_prefix") or files.get("doc_token_id") or "[unused1]")
        punct = _setting("mask_punctuation", mk, files, "mask_punctuation", where)
        if not isinstance(punct, bool):
            raise ValueError(f"ColBERT setting 'mask_punctuation'={punct!r} must be true or false")
        words = list(string.punctuation) if punct else []
    else:
        qtok = str(_setting("query_prefix", mk, files, "query_prefix", where))
        dtok = str(_setting("document_prefix", mk, files, "document_prefix", where))
        words = _setting("skiplist_words", mk, files, "skiplist_words", where)
        if not isinstance(words, (list, tuple)):
            raise ValueError("ColBERT setting 'skiplist_words' must be a list of words")
    markers = []
    for name, tok in (("query_prefix", qtok), ("document_prefix", dtok)):
        tid = vocab.single_token(tok.strip())
        if tid is None:
            raise ValueError(f"ColBERT {name}={tok!r} is not a single token of the tokenizer")
        markers.append(tid)
    skip = sorted({tid for w in words for tid in [vocab.token_id(str(w))] if tid is not None} - {cls_id, sep_id, markers[1]})
    return ColbertConfig(query_length=qlen, document_length=dlen, dim=dim, attend_to_expansion_tokens=attend,
                         query_marker=markers[0], document_marker=markers[1], cls_id=cls_id, sep_id=sep_id, mask_id=mask_id,
                         skiplist=tuple(skip), layout=layout)


# ---- token layout -----------------------------------------------------------------------------------------------------------------
def layout_query(body: Sequence[int], cc: ColbertConfig) -> Tuple[List[int], int]:
    """-> (the ``query_length`` token ids, key_len = the unpadded length)."""
    L = cc.query_length
    ids = [cc.cls_id, cc.query_marker] + [int(t) for t in body[: L - 3]] + [cc.sep_id]
    key_len = len(ids)
    return ids + [cc.mask_id] * (L - key_len), key_len


def layout_document(body: Sequence[int], cc: ColbertConfig) -> Tuple[List[int], List[int]]:
    """-> (token ids, the rows -- positions within the sequence -- that are projected and stored)."""
    ids = [cc.cls_id, cc.document_marker] + [int(t) for t in body[: cc.document_length - 3]] + [cc.sep_id]
    skip = set(cc.skiplist)
    last = len(ids) - 1
    kept = [i for i, t in enumerate(ids) if i < 2 or i == last or t not in skip]
    return ids, kept


# ---- checkpoint --------------------------------------------------------------------------------------------------------------------
def bert_state_names(cfg: EncoderConfig) -> List[str]:
    names = [f"embeddings.{n}" for n in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                                         "LayerNorm.weight", "LayerNorm.bias")]
    for i in range(cfg.layers):
        for m in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                  "attention.output.LayerNorm", "intermediate.dense", "output.dense", "output.LayerNorm"):
            names += [f"encoder.layer.{i}.{m}.weight", f"encoder.layer.{i}.{m}.bias"]
    return names


# tolerated and unused: BertModel's pooler, and the position_ids buffer older transformers wrote into every BERT state dict
_NOT_READ = re.compile(r"^(pooler\.|embeddings\.position_ids$)")


def check_state(cfg: EncoderConfig, state: Dict[str, torch.Tensor], layout: str) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
    """-> (the BERT tensors under BertModel's names, the projection ``linear.weight`` [dim][H]).  stanford: ``bert.*`` plus
    ``linear.weight``; pylate: BertModel's names (optionally under ``bert.``) plus ``linear.weight`` from ``1_Dense``.  Anything
    else is refused by name."""
    if "linear.weight" not in state:
        raise ValueError("checkpoint has no 'linear.weight' (the per-token projection): not a ColBERT checkpoint")
    if "linear.bias" in state:
        raise NotImplementedError("checkpoint carries 'linear.bias': the ColBERT projection has no bias")
    lin = state["linear.weight"]
    sd = {}
    for k, v in state.items():
        if k == "linear.weight":
            continue
        if k.startswith("bert."):
            k = k[len("bert."):]
        elif layout == "stanford":
            raise NotImplementedError(f"checkpoint carries tensors the ColBERT path does not compute: ['{k}']")
        sd[k] = v
    names = bert_state_names(cfg)
    missing = [n for n in names if n not in sd]
    if missing:
        raise ValueError(f"checkpoint is not a BERT of {cfg}: missing {missing[:4]}")
    extra = sorted(k for k in set(sd) - set(names) if not _NOT_READ.search(k))
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the ColBERT path does not compute: {extra[:4]}")
    if lin.dim() != 2 or lin.shape[1] != cfg.hidden:
        raise ValueError(f"linear.weight {tuple(lin.shape)} does not match hidden_size {cfg.hidden}")
    return {n: sd[n] for n in names}, lin


def _dense_module(model_dir: str) -> Tuple[str, dict]:
    """-> (path of the PyLate Dense module, its config.json), after refusing a module list this path does not compute."""
    with open(os.path.join(model_dir, "modules.json"), encoding="utf-8") as f:
        mods = json.load(f)
    kinds = [str(m.get("type", "")).rsplit(".", 1)[-1] for m in mods]
    if kinds != ["Transformer", "Dense"]:
        raise NotImplementedError(f"modules.json names {kinds}: a PyLate ColBERT is a Transformer and one Dense")
    if mods[0].get("path", "") not in ("", "."):
        raise NotImplementedError(f"modules.json: Transformer module at path {mods[0].get('path')!r} (expected the directory itself)")
    dpath = os.path.join(model_dir, str(mods[1].get("path", "1_Dense")))
    dc = read_json(os.path.join(dpath, "config.json"))
    unknown = sorted(set(dc) - {"in_features", "out_features", "bias", "activation_function", "use_residual"})
    if unknown:
        raise NotImplementedError(f"1_Dense/config.json carries fields the ColBERT path does not know: {unknown[:6]}")
    if dc.get("bias", False):
        raise NotImplementedError("1_Dense/config.json bias=true: the ColBERT projection has no bias")
    act = str(dc.get("activation_function", "torch.nn.modules.linear.Identity"))
    if act.rsplit(".", 1)[-1] != "Identity":
        raise NotImplementedError(f"1_Dense/config.json activation_function={act!r}: only Identity is computed")
    if dc.get("use_residual", False):
        raise NotImplementedError("1_Dense/config.json use_residual=true is not computed")
    return dpath, dc


resolve_dtype = functools.partial(_resolve_dtype, family="ColBERT")


def load_checkpoint(model_dir: str, model_kwargs: Optional[dict] = None):
    """A ColBERT directory of either layout -> (EncoderConfig, BERT state dict, linear.weight, ColbertConfig, tokenizer).  Host
    work only."""
    from . import weights as _weights
    from .tokenization import load_tokenizer

    layout = detect_layout(model_dir)
    if layout is None:
        raise ValueError(f"{model_dir} is not a ColBERT directory (no artifact.metadata, no PyLate Dense module)")
    resolve_dtype(model_kwargs)
    hf = read_json(os.path.join(model_dir, "config.json"))
    mt = hf.get("model_type")
    if mt != "bert" or hf.get("position_embedding_type", "absolute") != "absolute":
        raise NotImplementedError(f"config.json model_type={mt!r} position_embedding_type={hf.get('position_embedding_type')!r}: the "
                                  "ColBERT path serves BERT backbones (ModernBERT, XLM-R and Jina ColBERT are not supported)")
    if str(hf.get("hidden_act", "gelu")) != "gelu":
        raise NotImplementedError(f"config.json hidden_act={hf.get('hidden_act')!r}: the encoder computes 'gelu'")
    cfg = _weights._config_from_hf(hf, 0)
    cfg = EncoderConfig(**{**cfg.__dict__, "num_labels": 0})
    state = _weights.load_state(model_dir)
    if layout == "pylate":
        dpath, dc = _dense_module(model_dir)
        from safetensors.torch import load_file

        dense = load_file(os.path.join(dpath, "model.safetensors"))
        extra = sorted(set(dense) - {"linear.weight"})
        if extra:
            raise NotImplementedError(f"1_Dense carries tensors the ColBERT path does not compute: {extra[:4]}")
        if "linear.weight" in state:
            raise NotImplementedError("the Transformer module carries 'linear.weight' beside the Dense module's")
        state = dict(state)
        state.update(dense)
        if "out_features" in dc and int(dc["out_features"]) != dense["linear.weight"].shape[0]:
            raise ValueError(f"1_Dense/config.json out_features={dc['out_features']} does not match linear.weight "
                             f"{tuple(dense['linear.weight'].shape)}")
    bert, lin = check_state(cfg, state, layout)
    tk = (model_kwargs or {}).get("tokenizer") or load_tokenizer(model_dir, "bert", cfg.vocab_size)
    cc = parse_settings(model_dir, _Vocabulary(tk), model_kwargs, dense_out=int(lin.shape[0]))
    if max(cc.query_length, cc.document_length) > cfg.max_pos:
        raise ValueError(f"query_length={cc.query_length} / document_length={cc.document_length} exceed max_position_embeddings="
                         f"{cfg.max_pos}")
    return cfg, bert, lin, cc, tk


# ---- host wrappers of the kernels ------------------------------------------------------------------------------------------------
def maxsim(q_vecs: torch.Tensor, q_start, q_len, d_vecs: torch.Tensor, d_start, d_len, cand=None,
           n_cand: Optional[int] = None) -> torch.Tensor:
    """``tt_maxsim`` -> scores fp32 [n_q][n_cand] (device).  ``q_vecs`` [*, dim], ``d_vecs`` [*, dim]: 16-bit device tensors of
    one type.  ``q_start`` / ``q_len`` (int32), ``d_start`` (int64) / ``d_len`` (int32), ``cand`` ([n_q][n_cand] int32 document
    numbers, < 0 = none; None: documents 0 .. n_cand-1 for every query): host arrays are checked against the kernel's limits
    (q_len 1 .. 128, d_len 0 .. 512, rows inside the buffers) and uploaded; device tensors are taken as they are -- their owner
    (``TokenVectorStore``, ``ColbertEncoder``) checked them when it made them, and the kernel clamps a length into its range."""
    _need_device("maxsim", q_vecs, d_vecs)                # (this wrapper looks at the device first, ``maxsim_wide`` last)
    return _maxsim("maxsim", "tt_maxsim", MAX_QUERY_LEN, MAX_DOC_LEN, None, (), q_vecs, q_start, q_len, d_vecs, d_start, d_len, cand, n_cand)


def _maxsim(name: str, entry: str, max_q: int, max_d: int, check_dim, trailing: tuple, q_vecs: torch.Tensor, q_start, q_len,
            d_vecs: torch.Tensor, d_start, d_len, cand, n_cand: Optional[int]) -> torch.Tensor:
    """The body of ``maxsim`` and ``multivec.maxsim_wide``: library entry ``entry[_f16]`` with the kernel's limits ``max_q`` query
    and ``max_d`` document rows, ``check_dim(name, dim)`` (None: the library's own refusal) and ``trailing``, the entry's integer
    arguments behind ``dim``.  Bad host arguments are refused before the device is looked at."""
    if q_vecs.dtype != d_vecs.dtype or q_vecs.dim() != 2 or d_vecs.dim() != 2 or q_vecs.shape[1] != d_vecs.shape[1]:
        raise ValueError(f"{name}: query and document vectors must be [*, dim] of one 16-bit type")
    entry, dim = entry + _suffix(q_vecs.dtype), int(q_vecs.shape[1])
    if check_dim is not None:
        check_dim(name, dim)
    if not (q_vecs.is_contiguous() and d_vecs.is_contiguous()):
        raise ValueError(f"{name}: row-major vectors with a row stride of dim are needed")
    n_q = len(q_len)
    if not isinstance(q_len, torch.Tensor):
        _check_range("q_len", q_len, 1, max_q)
        _check_range("q_start", q_start, 0, q_vecs.shape[0] - np.asarray(q_len))
    if not isinstance(d_len, torch.Tensor):
        _check_range("d_len", d_len, 0, max_d)
        _check_range("d_start", d_start, 0, d_vecs.shape[0] - np.asarray(d_len))
    n_docs = len(d_len)
    if cand is None:
        n_cand = n_docs if n_cand is None else int(n_cand)
        if not 0 <= n_cand <= n_docs:
            raise ValueError(f"n_cand={n_cand} with {n_docs} documents")
    elif not isinstance(cand, torch.Tensor):
        cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(n_q, -1)
        if cand.size and cand.max() >= n_docs:
            raise ValueError(f"cand holds document number {int(cand.max())} with {n_docs} documents")
    dev = _need_device(name, q_vecs, d_vecs)
    cand_t = None
    if cand is not None:
        cand_t = _dev_i(cand, torch.int32, dev)
        n_cand = int(cand_t.shape[1]) if cand_t.dim() == 2 else int(cand_t.numel() // max(n_q, 1))
    qs, ql = _dev_i(q_start, torch.int32, dev), _dev_i(q_len, torch.int32, dev)
    ds, dl = _dev_i(d_start, torch.int64, dev), _dev_i(d_len, torch.int32, dev)
    scores = torch.empty((n_q, n_cand), dtype=torch.float32, device=dev)
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(q_vecs.data_ptr(), qs.data_ptr(), ql.data_ptr(), n_q, d_vecs.data_ptr(), ds.data_ptr(), dl.data_ptr(),
                                 cand_t.data_ptr() if cand_t is not None else None, n_cand, dim, *trailing, scores.data_ptr(),
                                 _stream(dev))
    _lib.check(rc, entry)
    return scores


def maxsim_scan_topk(q_vecs: torch.Tensor, q_start, q_len, d_vecs: torch.Tensor, d_start, d_len, k: int, alive=None,
                     workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``tt_maxsim_scan_topk`` -> (scores fp32 [n_q][k], document numbers int32 [n_q][k]) on the device: the exact MaxSim top-k over
    every entry of the document arrays in one read of them, ordered by (score descending, document number ascending), padded with
    (-inf, -1).  Every score is ``maxsim``'s for the same pair, bit for bit.  ``alive``: uint8 [n_docs], 0 = a tombstone that is
    never returned (None: every document is live).  1 .. 64 queries, k 1 .. 1024; the arrays are checked as ``maxsim``'s.
    ``workspace``: a caller-owned uint8 device tensor (``tt_maxsim_scan_workspace_bytes``), allocated here when missing or short."""
    name = "maxsim_scan_topk"
    _need_device(name, q_vecs, d_vecs)
    if q_vecs.dtype != d_vecs.dtype or q_vecs.dim() != 2 or d_vecs.dim() != 2 or q_vecs.shape[1] != d_vecs.shape[1]:
        raise ValueError(f"{name}: query and document vectors must be [*, dim] of one 16-bit type")
    entry, dim = "tt_maxsim_scan_topk" + _suffix(q_vecs.dtype), int(q_vecs.shape[1])
    if not (q_vecs.is_contiguous() and d_vecs.is_contiguous()):
        raise ValueError(f"{name}: row-major vectors with a row stride of dim are needed")
    n_q, n_docs = len(q_len), len(d_len)
    if not 1 <= n_q <= MAX_SCAN_QUERIES:
        raise ValueError(f"{name}: {n_q} queries (1 .. {MAX_SCAN_QUERIES})")
    if not 1 <= int(k) <= MAX_SCAN_K:
        raise ValueError(f"{name}: k={k} (1 .. {MAX_SCAN_K})")
    if not isinstance(q_len, torch.Tensor):
        _check_range("q_len", q_len, 1, MAX_QUERY_LEN)
        _check_range("q_start", q_start, 0, q_vecs.shape[0] - np.asarray(q_len))
    if not isinstance(d_len, torch.Tensor):
        _check_range("d_len", d_len, 0, MAX_DOC_LEN)
        _check_range("d_start", d_start, 0, d_vecs.shape[0] - np.asarray(d_len))
    if alive is not None and len(alive) != n_docs:
        raise ValueError(f"{name}: alive holds {len(alive)} entries for {n_docs} documents")
    dev = _need_device(name, q_vecs, d_vecs)
    qs, ql = _dev_i(q_start, torch.int32, dev), _dev_i(q_len, torch.int32, dev)
    ds, dl = _dev_i(d_start, torch.int64, dev), _dev_i(d_len, torch.int32, dev)
    al = None
    if alive is not None:
        al = _dev_i(alive, torch.uint8, dev) if isinstance(alive, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(alive, dtype=np.uint8)).to(dev)
    lib = _lib.load_library()
    need = int(lib.tt_maxsim_scan_workspace_bytes(n_docs, n_q))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    scores = torch.empty((n_q, int(k)), dtype=torch.float32, device=dev)
    idx = torch.empty((n_q, int(k)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(q_vecs.data_ptr(), qs.data_ptr(), ql.data_ptr(), n_q, d_vecs.data_ptr(), ds.data_ptr(), dl.data_ptr(),
                                 al.data_ptr() if al is not None else None, n_docs, dim, int(k), scores.data_ptr(), idx.data_ptr(),
                                 workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream(dev))
    _lib.check(rc, entry)
    return scores, idx


def project(hidden: torch.Tensor, weight: torch.Tensor, rows) -> torch.Tensor:
    """``tt_colbert_project`` -> [n_out][dim] in the operands' type: row n = normalize(weight @ hidden[rows[n]])."""
    dev = hidden.device
    if dev.type != "cuda" or weight.device != dev:
        raise RuntimeError("project: device tensors are needed; tensor_truth_amd has no CPU path")
    if hidden.dtype != weight.dtype or hidden.dim() != 2 or weight.dim() != 2 or hidden.shape[1] != weight.shape[1]:
        raise ValueError("project: hidden [n_rows][H] and weight [dim][H] of one 16-bit type are needed")
    if not (hidden.is_contiguous() and weight.is_contiguous()):
        raise ValueError("project: contiguous operands are needed")
    sfx = _suffix(hidden.dtype)
    rows_t = _dev_i(rows, torch.int32, dev)
    n_out, dim = int(rows_t.numel()), int(weight.shape[0])
    out = torch.empty((n_out, dim), dtype=hidden.dtype, device=dev)
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        rc = getattr(lib, "tt_colbert_project" + sfx)(hidden.data_ptr(), int(hidden.shape[0]), int(hidden.shape[1]), weight.data_ptr(),
                                                      dim, rows_t.data_ptr(), n_out, out.data_ptr(), _stream(dev))
    _lib.check(rc, "tt_colbert_project" + sfx)
    return out


def check_key_len(seq_len, key_len) -> None:
    """1 <= key_len <= seq_len <= 128 for every sequence (what the key-limited kernels are defined for)."""
    seq_len, key_len = np.asarray(seq_len), np.asarray(key_len)
    if seq_len.shape != key_len.shape:
        raise ValueError("key_len: one entry per sequence is needed")
    _check_range("seq_len", seq_len, 1, MAX_QUERY_LEN)
    _check_range("key_len", key_len, 1, seq_len)


def attention_keylimit(qk: torch.Tensor, q_col0: int, k_col0: int, vt: torch.Tensor, out: torch.Tensor, seq_start, seq_len, key_len,
                       heads: int, head_dim: int) -> torch.Tensor:
    """``tt_attention_keylimit`` on ``tt_attention_varlen``'s operands (``vt`` in the V8 layout, [rows / 8][heads * head_dim][8]);
    ``seq_start`` / ``seq_len`` / ``key_len``: host int arrays, checked here and uploaded.  Writes the sequences' rows of ``out``."""
    dev = qk.device
    sfx = _suffix(qk.dtype)
    seq_start, seq_len, key_len = (np.ascontiguousarray(a, dtype=np.int32) for a in (seq_start, seq_len, key_len))
    check_key_len(seq_len, key_len)
    if (seq_start < 0).any() or (seq_start + seq_len > qk.shape[0]).any():
        raise ValueError("seq_start: every sequence must lie inside the rows of qk")
    if vt.numel() < (int((seq_start + seq_len).max()) + 7) // 8 * 8 * heads * head_dim:
        raise ValueError("vt does not hold the 8-row groups of every sequence")
    st, sl, kl = (torch.from_numpy(a).to(dev) for a in (seq_start, seq_len, key_len))
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        rc = getattr(lib, "tt_attention_keylimit" + sfx)(qk.data_ptr(), int(qk.shape[1]), q_col0, k_col0, vt.data_ptr(),
                                                         8 * heads * head_dim, out.data_ptr(), int(out.shape[1]), st.data_ptr(),
                                                         sl.data_ptr(), kl.data_ptr(), len(seq_len), heads, head_dim,
                                                         int(seq_len.max()), _stream(dev))
    _lib.check(rc, "tt_attention_keylimit" + sfx)
    return out


# ---- weights and encoder ----------------------------------------------------------------------------------------------------------
class ColbertWeights:
    """Device-resident weights of a ColBERT checkpoint: the BERT encoder in the layout of ``tt_encoder_weights`` (bf16 or fp16)
    and the projection [dim][H] in the same type."""

    def __init__(self, cfg: EncoderConfig, bert_state: Dict[str, torch.Tensor], linear: torch.Tensor, device: torch.device,
                 dtype: torch.dtype = torch.bfloat16):
        if cfg.arch != "bert" or cfg.num_labels:
            raise ValueError(f"ColbertWeights: a BERT backbone without a classification head is needed, not {cfg}")
        self.encoder = EncoderWeights(cfg, bert_state, device, dtype)
        self.cfg, self.device, self.dtype = cfg, device, dtype
        if linear.dim() != 2 or linear.shape[1] != cfg.hidden:
            raise ValueError(f"linear.weight {tuple(linear.shape)} does not match hidden_size {cfg.hidden}")
        self.linear = linear.to(device=device, dtype=dtype).contiguous()
        self.dim = int(linear.shape[0])

    def parameters(self) -> Iterable[torch.Tensor]:
        """For ModelManager-style memory accounting."""
        yield from self.encoder.parameters()
        yield self.linear

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.parameters())


@dataclass
class TokenVectors:
    """Packed per-token vectors of several texts: text i owns rows ``starts[i] .. starts[i] + lens[i] - 1`` of ``vectors``."""

    vectors: torch.Tensor      # [sum(lens)][dim], device, bf16 or fp16
    starts: np.ndarray         # int64 [n]
    lens: np.ndarray           # int32 [n]


class ColbertEncoder:
    """Texts (or body token ids, no specials) -> per-token vectors, with the token layout of the module docstring."""

    def __init__(self, weights: ColbertWeights, settings: ColbertConfig, tokenizer, batch_texts: int = 256):
        self.w, self.cc, self.tokenizer = weights, settings, tokenizer
        self.vocab = _Vocabulary(tokenizer)
        self.cfg, self.device = weights.cfg, weights.device
        self._enc = Encoder(weights.encoder)
        self.batch_texts = batch_texts
        self._sfx = _suffix(weights.dtype)

    def _bodies(self, items) -> List[Sequence[int]]:
        return [self.vocab.body(x) if isinstance(x, str) else x for x in items]

    def _forward(self, seqs: List[List[int]], key_len: Optional[np.ndarray]):
        """-> (hidden [n_rows][H], the batch) through the plain forward, or the key-limited one when ``key_len`` is given."""
        batch = pack_tokens(seqs, self.cfg)
        enc = self._enc
        if key_len is None:
            hidden, _ = enc.forward_packed(batch)
            return hidden, batch
        check_key_len(batch.seq_len, key_len)
        dev, w = self.device, ctypes.byref(self.w.encoder.struct)
        ids, pos, types, starts, lens, klen = enc._upload(batch, np.ascontiguousarray(key_len, dtype=np.int32))
        hidden = torch.empty((batch.n_rows, self.cfg.hidden), dtype=self.w.dtype, device=dev)
        name = "tt_encoder_forward_keylen" + self._sfx
        need = getattr(enc.lib, enc.path.workspace)(w, batch.n_rows)
        with enc._enqueue_lock, torch.cuda.device(dev):
            _ws, base = _scratch.get(enc.path.scratch, dev, need)
            rc = getattr(enc.lib, name)(w, ids.data_ptr(), pos.data_ptr(), None, starts.data_ptr(), lens.data_ptr(), klen.data_ptr(),
                                        len(batch.seq_len), batch.n_rows, batch.max_len, hidden.data_ptr(), base, need, _stream(dev))
        _lib.check(rc, name)
        return hidden, batch

    def _encode(self, seqs: List[List[int]], kept: List[Sequence[int]], key_len: Optional[np.ndarray]) -> TokenVectors:
        lens = np.asarray([len(k) for k in kept], dtype=np.int32)
        starts = np.zeros(len(kept), dtype=np.int64)
        np.cumsum(lens[:-1], out=starts[1:])
        parts = []
        for lo in range(0, len(seqs), self.batch_texts):
            hi = min(lo + self.batch_texts, len(seqs))
            hidden, batch = self._forward(seqs[lo:hi], None if key_len is None else key_len[lo:hi])
            rows = np.concatenate([int(s) + np.asarray(k, dtype=np.int32) for s, k in zip(batch.seq_start, kept[lo:hi])])
            parts.append(project(hidden, self.w.linear, rows.astype(np.int32)))
        vecs = parts[0] if len(parts) == 1 else torch.cat(parts)
        return TokenVectors(vecs, starts, lens)

    def query_tokens(self, items) -> Tuple[List[List[int]], np.ndarray]:
        laid = [layout_query(b, self.cc) for b in self._bodies(items)]
        return [ids for ids, _ in laid], np.asarray([k for _, k in laid], dtype=np.int32)

    def document_tokens(self, items) -> Tuple[List[List[int]], List[List[int]]]:
        laid = [layout_document(b, self.cc) for b in self._bodies(items)]
        return [ids for ids, _ in laid], [kept for _, kept in laid]

    def encode_queries(self, items) -> TokenVectors:
        """``items``: query strings, or their body token ids (no specials) -> ``query_length`` vectors per query."""
        if len(items) == 0:
            raise ValueError("encode_queries: no query")
        seqs, key_len = self.query_tokens(items)
        every = [range(self.cc.query_length)] * len(seqs)
        return self._encode(seqs, every, None if self.cc.attend_to_expansion_tokens else key_len)

    def encode_documents(self, items) -> TokenVectors:
        """``items``: passages, or their body token ids (no specials) -> one vector per kept token."""
        if len(items) == 0:
            raise ValueError("encode_documents: no document")
        seqs, kept = self.document_tokens(items)
        return self._encode(seqs, kept, None)


# ---- the store ----------------------------------------------------------------------------------------------------------------------
class TokenVectorStore:
    """Token vectors of indexed passages, in HBM on one device: 2 * dim bytes per kept token (about 46 KB for a 180-token passage
    at dim 128), plus 13 bytes per passage for its start, its length and its ``alive`` byte.  ``add`` appends and grows by doubling; ``remove`` frees the
    id only -- the rows stay where they are and are NOT reclaimed (there is no compaction in this version; re-adding an id
    appends a new copy).  No persistence.  ``search`` is the exact MaxSim top-k over every stored passage
    (``tt_maxsim_scan_topk``): ``alive`` holds one byte per document number, 1 from ``add``, 0 once the id is removed or added
    again, and a number whose byte is 0 is never returned.  ``score`` does not read it: a number no id leads to still scores as
    before through ``tt_maxsim``, it is just never asked for."""

    # the limits of the kernel that scores the store (``tt_maxsim``); ``multivec.MultiVectorStore`` carries ``tt_maxsim_wide``'s
    DIM_STEP, DIM_LIMIT, DOC_LIMIT = 32, MAX_DIM, MAX_DOC_LEN

    def __init__(self, dim: int, dtype: torch.dtype, device: torch.device, capacity_tokens: int = 1 << 16, capacity_docs: int = 1 << 10):
        _suffix(dtype)
        name = type(self).__name__
        if dim <= 0 or dim % self.DIM_STEP or dim > self.DIM_LIMIT:
            raise ValueError(f"{name}: dim={dim} (a multiple of {self.DIM_STEP} up to {self.DIM_LIMIT})")
        if device.type != "cuda":
            raise RuntimeError(f"{name} lives on a HIP device; tensor_truth_amd has no CPU path")
        self.dim, self.dtype, self.device = dim, dtype, device
        self.vectors = torch.empty((max(capacity_tokens, 1), dim), dtype=dtype, device=device)
        self.d_start = torch.zeros(max(capacity_docs, 1), dtype=torch.int64, device=device)
        self.d_len = torch.zeros(max(capacity_docs, 1), dtype=torch.int32, device=device)
        self.alive = torch.zeros(max(capacity_docs, 1), dtype=torch.uint8, device=device)
        self.n_tokens = 0
        self.n_docs = 0
        self._ids = IdTable()
        self._ws: Optional[torch.Tensor] = None          # search's workspace, grown on demand

    def __len__(self) -> int:
        return len(self._ids)

    def add(self, node_ids: Sequence[Any], vectors: torch.Tensor, lens) -> np.ndarray:
        """Append the passages' vectors (packed in order: passage i owns the next ``lens[i]`` rows) -> their document numbers."""
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if len(node_ids) != len(lens):
            raise ValueError("add: one length per node id is needed")
        _check_range("lens", lens, 0, self.DOC_LIMIT)
        total = int(lens.sum())
        if vectors.dtype != self.dtype or vectors.dim() != 2 or tuple(vectors.shape) != (total, self.dim):
            raise ValueError(f"add: vectors {tuple(vectors.shape)} {vectors.dtype} do not match [{total}][{self.dim}] {self.dtype}")
        n = len(lens)
        if n == 0:
            return np.zeros(0, dtype=np.int32)
        self.vectors = grown(self.vectors, self.n_tokens, self.n_tokens + total)
        self.d_start = grown(self.d_start, self.n_docs, self.n_docs + n)
        self.d_len = grown(self.d_len, self.n_docs, self.n_docs + n)
        self.alive = grown(self.alive, self.n_docs, self.n_docs + n)
        starts = np.zeros(n, dtype=np.int64)
        np.cumsum(lens[:-1], out=starts[1:])
        starts += self.n_tokens
        self.vectors[self.n_tokens:self.n_tokens + total].copy_(vectors.to(self.device))
        self.d_start[self.n_docs:self.n_docs + n].copy_(torch.from_numpy(starts))
        self.d_len[self.n_docs:self.n_docs + n].copy_(torch.from_numpy(lens))
        self.alive[self.n_docs:self.n_docs + n].fill_(1)
        docs = np.arange(self.n_docs, self.n_docs + n, dtype=np.int32)
        for old in self._ids.assign(node_ids):           # re-added: the older copy is never returned by ``search`` again
            self.alive[old:old + 1].fill_(0)
        self.n_tokens += total
        self.n_docs += n
        return docs

    def remove(self, node_id: Any) -> bool:
        """Forget ``node_id`` -> whether it was stored.  Its rows are not reclaimed; ``search`` no longer returns its number."""
        doc = self._ids.pop(node_id)
        if doc is None:
            return False
        self.alive[doc:doc + 1].fill_(0)
        return True

    def lookup(self, node_ids: Sequence[Any]) -> np.ndarray:
        """-> document numbers (int32), -1 for an id that is not stored."""
        return self._ids.lookup(node_ids)

    def node_id(self, doc: int) -> Any:
        """The node id of document number ``doc`` (None: removed, or no such document)."""
        return self._ids.node_id(doc)

    @property
    def nbytes(self) -> int:
        """Bytes the store holds in HBM (capacity, not fill)."""
        return sum(t.numel() * t.element_size() for t in (self.vectors, self.d_start, self.d_len, self.alive))

    def score(self, queries: TokenVectors, cand: np.ndarray) -> torch.Tensor:
        """MaxSim of every query against its row of ``cand`` (document numbers, -1 = none) -> fp32 [n_q][n_cand] (device)."""
        cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(len(queries.lens), -1)
        if cand.size and cand.max() >= self.n_docs:
            raise ValueError(f"document number {int(cand.max())} with {self.n_docs} documents stored")
        return maxsim(queries.vectors, queries.starts.astype(np.int32), queries.lens, self.vectors, self.d_start[: self.n_docs],
                      self.d_len[: self.n_docs], cand=cand)

    def search(self, queries: TokenVectors, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The exact MaxSim top-k over every stored passage, in one read of the store for up to eight 32-token queries -> (scores
        fp32 [n_q][k], document numbers int32 [n_q][k]) on the device, ordered by (score descending, document number ascending),
        padded with (-inf, -1).  A score is ``score``'s for the same pair, bit for bit; removed and replaced numbers are never
        returned.  A store whose limits exceed the scan's (``MultiVectorStore``) raises ``NotImplementedError``."""
        if self.DIM_LIMIT > MAX_DIM or self.DOC_LIMIT > MAX_DOC_LEN:
            raise NotImplementedError(f"{type(self).__name__}.search: the exact MaxSim scan (tt_maxsim_scan_topk) serves dim <= {MAX_DIM} "
                                      f"and passages of <= {MAX_DOC_LEN} vectors; this store (dim={self.dim}, up to {self.DOC_LIMIT} "
                                      "vectors per passage) is a rerank-stage store: use score() on candidates")
        need = int(_lib.load_library().tt_maxsim_scan_workspace_bytes(self.n_docs, len(queries.lens)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return maxsim_scan_topk(queries.vectors, np.asarray(queries.starts).astype(np.int32), queries.lens, self.vectors,
                                self.d_start[: self.n_docs], self.d_len[: self.n_docs], k, alive=self.alive[: self.n_docs],
                                workspace=self._ws)


# ---- postprocessor ---------------------------------------------------------------------------------------------------------------
class HipColbertRerank(_StoredRerank):
    """Late-interaction rerank postprocessor with the surface of ``HipSentenceTransformerRerank``: ``postprocess_nodes`` (keyword
    or positional), ``rerank``, ``predict``, ``.model`` (the weights, with ``.parameters()``) -- plus ``index_nodes``, which
    encodes nodes' EMBED-mode content into the instance's ``TokenVectorStore`` (and keeps the nodes, for ``HipColbertRetriever``),
    and ``remove_node``.  At query time a stored node is scored from the
    store and any other node is encoded in the call; both give the same bits for the same text.  Scores are MaxSim sums (of the
    order of the query length), not probabilities."""

    def __init__(self, model: str, top_n: int = 2, device: Optional[str] = None, keep_retrieval_score: bool = False,
                 model_kwargs: Optional[Dict[str, Any]] = None, **_ignored):
        from . import weights as _weights
        from .tokenization import load_tokenizer

        dev = resolve_device(device)
        mk = dict(model_kwargs or {})
        self.model_name, self.top_n, self.device, self.keep_retrieval_score = model, top_n, dev, keep_retrieval_score
        dtype = resolve_dtype(mk)
        if "state_dict" in mk or ("synthetic_seed" in mk and _weights.find_model_dir(model, mk) is None):
            cfg = mk.get("encoder_config")
            if cfg is None:
                raise ValueError(f"no architecture known for '{model}': pass model_kwargs['encoder_config']")
            state = mk["state_dict"] if "state_dict" in mk else synthetic_state(cfg, int(mk["dim"]), int(mk["synthetic_seed"]))
            bert, lin = check_state(cfg, state, "pylate")
            tk = mk.get("tokenizer") or load_tokenizer(None, "bert", cfg.vocab_size)
            cc = parse_settings(None, _Vocabulary(tk), mk, dense_out=int(lin.shape[0]))
        else:
            mdir = _weights.find_model_dir(model, mk)
            if mdir is None:
                raise FileNotFoundError(f"weights for '{model}' not found: no checkpoint directory under model_kwargs['model_dir'], "
                                        "$TT_AMD_MODEL_DIR or the HF cache, and this environment has no network")
            cfg, bert, lin, cc, tk = load_checkpoint(mdir, mk)
        self.config, self.settings = cfg, cc
        self.model = ColbertWeights(cfg, bert, lin, dev, dtype)
        self.encoder = ColbertEncoder(self.model, cc, tk)
        self.store = TokenVectorStore(cc.dim, dtype, dev)
        self.precision = "fp16 (fp32 accumulate)" if dtype == torch.float16 else "bf16 (fp32 accumulate)"
        self.nodes: Dict[Any, Any] = {}      # node id -> the indexed node (what HipColbertRetriever returns)
        self.stats = {"queries": 0, "stored": 0, "encoded": 0}

    def remove_node(self, node_id: Any) -> bool:
        self.nodes.pop(node_id, None)
        return self.store.remove(node_id)

    # ---- what _StoredRerank asks for --------------------------------------------------------------------------------
    def encode_queries(self, texts) -> TokenVectors:
        return self.encoder.encode_queries(texts)

    def encode_documents(self, texts) -> TokenVectors:
        return self.encoder.encode_documents(texts)

    def add_documents(self, nodes, tv: TokenVectors) -> None:
        self.store.add([n.id_ for n in nodes], tv.vectors, tv.lens)
        self.nodes.update((n.id_, n) for n in nodes)

    def lookup(self, ids) -> np.ndarray:
        return self.store.lookup(ids)

    def score_stored(self, qv: TokenVectors, cands) -> np.ndarray:
        return self.store.score(qv, cands[0]).cpu().numpy()

    def score_fresh(self, qv: TokenVectors, tv: TokenVectors, cand) -> np.ndarray:
        return maxsim(qv.vectors, qv.starts.astype(np.int32), qv.lens, tv.vectors, tv.starts, tv.lens, cand=cand).cpu().numpy()


class HipColbertRetriever:
    """Exact late-interaction retrieval over the nodes a ``HipColbertRerank`` indexed: ``retrieve(query)`` encodes the query (one
    key-limited forward), runs ``TokenVectorStore.search`` -- every stored passage is scored, none is approximated -- and returns
    the best ``similarity_top_k`` stored nodes by MaxSim, best first, with the scores ``postprocess_nodes`` gives the same nodes.
    Scores are MaxSim sums and are not thresholded: unlike a lexical zero ("no shared term") a MaxSim value has no such point."""

    def __init__(self, reranker: HipColbertRerank, similarity_top_k: int = 10):
        if not 1 <= int(similarity_top_k) <= MAX_SCAN_K:
            raise ValueError(f"similarity_top_k={similarity_top_k} (1 .. {MAX_SCAN_K})")
        self.reranker, self.similarity_top_k = reranker, int(similarity_top_k)

    def retrieve(self, query):
        from .schema import NodeWithScore, as_query_bundle

        return self._retrieve(as_query_bundle(query), NodeWithScore)

    def _retrieve(self, query_bundle, node_type=None):
        if node_type is None:
            from .schema import NodeWithScore as node_type
        rr = self.reranker
        qv = rr.encode_queries([query_bundle.query_str])
        return top_nodes(rr.store, qv, self.similarity_top_k, rr.nodes, node_type, positive_only=False)


def synthetic_state(cfg: EncoderConfig, dim: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random weights of a ColBERT of ``cfg`` (benchmarks): the encoder's synthetic BERT plus ``linear.weight`` [dim][H]."""
    from .encoder import synthetic_state as bert_state

    sd = dict(bert_state(cfg, seed))
    g = torch.Generator().manual_seed(seed + 1)
    sd["linear.weight"] = torch.randn(dim, cfg.hidden, generator=g) * 0.02
    return sd


# the published geometry of colbert-ir/colbertv2.0 (bert-base-uncased -> 128): tools/colbert_bench.py
COLBERT_V2 = EncoderConfig(arch="bert", vocab_size=30522, hidden=768, layers=12, heads=12, ffn=3072, max_pos=512, type_vocab=2,
                           pad_id=0, ln_eps=1e-12)
