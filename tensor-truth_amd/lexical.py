"""Hybrid (dense + lexical) retrieval with ``BAAI/bge-m3``'s second head on the HIP path.

A BGE-M3 directory ships ``sparse_linear.pt`` beside the encoder: a single H-wide linear layer that turns the forward pass the
embedder already runs into one weight per token, ``t_i = relu(<w, h_i> + b)`` over the last hidden state.  A text's lexical vector
holds, for every distinct token id it contains, the maximum of ``t_i`` over the id's occurrences (``tt_lexical_weights``); a pair's
lexical score is the sum over shared ids of the two weights, and the hybrid score mixes it with the dense dot product
(``tt_lexical_score``).  Passages are encoded ONCE, when they are indexed, into a device-resident CSR store (``LexicalStore``: about
8 bytes per distinct token, against 2 KB for the dense row); a query costs one short forward plus a scoring kernel, and
``tt_lexical_scan_topk`` is the exact lexical top-k over every stored passage.

[UPSTREAM-K] The semantics are written from knowledge of FlagEmbedding's ``BGEM3FlagModel`` (``sparse_linear.pt`` with ``weight``
[1][H] and ``bias`` [1]; ``_process_token_weights``: the maximum per id, the four special ids and weights <= 0 left out;
``compute_lexical_matching_score``; "dense+sparse" in ``compute_score``), which is not installed here and cannot be checked offline.
The loader is therefore strict: a key or a shape it does not know is refused by name, and the two mixing weights are never
defaulted.  ``colbert_linear.pt`` (the model's multi-vector head) may be present and is not read here: ``multivec.py`` reads it.

The dot product is accumulated in fp32 and the weight kept in fp32; upstream's fp16 mode rounds it to fp16.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._hostargs import _check_range, _dev_i, _need_device, _stream, grown
from ._stored import IdTable, _StoredRerank, top_nodes
from .encoder import pack_tokens

SPARSE_FILE = "sparse_linear.pt"
# the kernels' limits (include/tt_hip.h)
MAX_SEQ_LEN, MAX_QUERY_NNZ, MAX_DOC_NNZ, MAX_HIDDEN = 8192, 512, 8192, 1024
MAX_SCAN_QUERIES, MAX_SCAN_K = 64, 1024


# ---- checkpoint --------------------------------------------------------------------------------------------------------------------
def has_lexical_head(model_dir: Optional[str]) -> bool:
    """Whether ``model_dir`` is a directory that ships ``sparse_linear.pt``."""
    return bool(model_dir) and os.path.isfile(os.path.join(model_dir, SPARSE_FILE))


def load_sparse_head(model_dir: str, hidden: int) -> Tuple[torch.Tensor, float]:
    """``sparse_linear.pt`` -> (w fp32 [hidden] on the host, bias).  [UPSTREAM-K] a torch-pickled state dict with ``weight``
    [1][hidden] and ``bias`` [1]; any other key or shape is refused by name."""
    path = os.path.join(model_dir or "", SPARSE_FILE)
    if not has_lexical_head(model_dir):
        raise FileNotFoundError(f"{path} not found: the directory has no lexical head (a BGE-M3 checkpoint ships it beside "
                                "model.safetensors)")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: a state dict is expected, not {type(sd).__name__}")
    unknown = sorted(set(sd) - {"weight", "bias"})
    if unknown:
        raise NotImplementedError(f"{path} carries tensors the lexical head does not compute: {unknown[:4]}")
    missing = [k for k in ("weight", "bias") if k not in sd]
    if missing:
        raise ValueError(f"{path} has no {missing}: not a lexical head")
    w, b = sd["weight"], sd["bias"]
    if not isinstance(w, torch.Tensor) or tuple(w.shape) != (1, hidden):
        raise ValueError(f"{path}: weight {tuple(getattr(w, 'shape', ()))} does not match [1][{hidden}]")
    if not isinstance(b, torch.Tensor) or tuple(b.shape) != (1,):
        raise ValueError(f"{path}: bias {tuple(getattr(b, 'shape', ()))} does not match [1]")
    return w.reshape(hidden).to(torch.float32).contiguous(), float(b.to(torch.float32)[0])


def special_ids(tokenizer) -> Tuple[int, int, int, int]:
    """The ids of ``<s>``, ``</s>``, ``<pad>``, ``<unk>`` -- the ids a lexical vector leaves out -- read from the tokenizer (XLM-R:
    0, 2, 1, 3).  The hashing stand-in of synthetic weights gives its own."""
    hf = getattr(tokenizer, "tk", None)
    if hf is None:
        sp = tokenizer.sp
        return int(sp.bos), int(sp.eos), int(sp.pad), int(sp.unk)
    out = []
    for tok in ("<s>", "</s>", "<pad>", "<unk>"):
        tid = hf.token_to_id(tok)
        if tid is None:
            raise ValueError(f"the tokenizer has no {tok} token: not an XLM-R vocabulary")
        out.append(int(tid))
    return tuple(out)


def check_hybrid_weights(model_kwargs: Optional[dict]) -> Tuple[float, float]:
    """``model_kwargs["hybrid_weights"] = (w_dense, w_lex)``: required, both >= 0, not both 0.  Never defaulted (upstream's
    examples use 0.4 and 0.2)."""
    hw = (model_kwargs or {}).get("hybrid_weights")
    if hw is None:
        raise ValueError("model_kwargs['hybrid_weights'] = (w_dense, w_lex) is missing: the two weights of the hybrid score are the "
                         "caller's and are never defaulted")
    try:
        wd, wl = (float(x) for x in hw)
    except (TypeError, ValueError):
        raise ValueError(f"model_kwargs['hybrid_weights']={hw!r}: two numbers (w_dense, w_lex) are expected") from None
    if not (wd >= 0 and wl >= 0 and wd + wl > 0 and np.isfinite(wd + wl)):
        raise ValueError(f"model_kwargs['hybrid_weights']={hw!r}: both weights >= 0 and not both 0")
    return wd, wl


# ---- host wrappers of the kernels ------------------------------------------------------------------------------------------------
_WEIGHTS_ENTRY = {torch.bfloat16: "tt_lexical_weights", torch.float16: "tt_lexical_weights_f16", torch.float32: "tt_lexical_weights_f32"}


def lexical_weights(hidden: torch.Tensor, w: torch.Tensor, bias: float, ids, seq_start, seq_len, skip: Sequence[int],
                    max_len: Optional[int] = None, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """``tt_lexical_weights[_f16|_f32]``, picked by ``hidden.dtype`` -> (terms int32 [n_rows], weights fp32 [n_rows], nnz int32
    [n_seq]) on the device: sequence b's distinct kept ids in ascending order at ``seq_start[b] ..``, then (-1, 0) up to its
    length.  ``hidden`` [n_rows][H] and ``w`` [H] of one type; ``ids`` int32 [n_rows]; ``skip``: the four ids left out.  Host
    ``seq_start`` / ``seq_len`` are checked against the kernel's limits (lengths 1 .. 8192, rows inside ``hidden``) and uploaded;
    device tensors are taken as they are, with ``max_len`` given.  ``out``: (terms, weights) to write into (rows of no sequence
    are left as they are); default: new arrays of (-1, 0)."""
    name = _WEIGHTS_ENTRY.get(hidden.dtype)
    if name is None or w.dtype != hidden.dtype:
        raise ValueError(f"lexical_weights: hidden {hidden.dtype} and w {w.dtype} must be one of bfloat16, float16, float32")
    if hidden.dim() != 2 or w.dim() != 1 or w.shape[0] != hidden.shape[1] or not w.is_contiguous() or hidden.stride(1) != 1:
        raise ValueError("lexical_weights: hidden [n_rows][H] with unit column stride and w [H] are needed")
    n_rows, H, ld = int(hidden.shape[0]), int(hidden.shape[1]), int(hidden.stride(0))
    if H <= 0 or H % 128 or H > MAX_HIDDEN:
        raise NotImplementedError(f"lexical_weights: hidden size {H}: a multiple of 128 up to {MAX_HIDDEN}")
    if len(skip) != 4:
        raise ValueError("lexical_weights: four ids to leave out are needed (<s>, </s>, <pad>, <unk>)")
    n_seq = len(seq_len)
    if not isinstance(seq_len, torch.Tensor):
        _check_range("seq_len", seq_len, 1, MAX_SEQ_LEN)
        _check_range("seq_start", seq_start, 0, n_rows - np.asarray(seq_len))
        max_len = int(np.max(seq_len)) if n_seq and max_len is None else max_len
    if n_seq and (max_len is None or not 1 <= int(max_len) <= MAX_SEQ_LEN):
        raise ValueError(f"lexical_weights: max_len={max_len} is outside 1 .. {MAX_SEQ_LEN}")
    dev = _need_device("lexical_weights", hidden, w)      # (the host-side refusals above need no device)
    ids_t = _dev_i(ids, torch.int32, dev)
    if ids_t.numel() != n_rows:
        raise ValueError(f"lexical_weights: {ids_t.numel()} token ids for {n_rows} rows")
    st, sl = _dev_i(seq_start, torch.int32, dev), _dev_i(seq_len, torch.int32, dev)
    if out is None:
        terms = torch.full((n_rows,), -1, dtype=torch.int32, device=dev)
        weights = torch.zeros((n_rows,), dtype=torch.float32, device=dev)
    else:
        terms, weights = _dev_i(out[0], torch.int32, dev), out[1]
        if weights.dtype != torch.float32 or weights.device != dev or terms.numel() != n_rows or weights.numel() != n_rows:
            raise ValueError("lexical_weights: out = (int32 [n_rows], float32 [n_rows]) on the device is needed")
    nnz = torch.zeros((n_seq,), dtype=torch.int32, device=dev)
    if n_seq == 0:
        return terms, weights, nnz
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(hidden.data_ptr(), n_rows, ld, H, w.data_ptr(), float(bias), ids_t.data_ptr(), st.data_ptr(),
                                sl.data_ptr(), n_seq, int(max_len), int(skip[0]), int(skip[1]), int(skip[2]), int(skip[3]),
                                terms.data_ptr(), weights.data_ptr(), nnz.data_ptr(), _stream(dev))
    _lib.check(rc, name)
    return terms, weights, nnz


def _check_entries(what: str, terms: torch.Tensor, weights: torch.Tensor, start, nnz, lo: int, hi: int) -> None:
    if terms.dtype != torch.int32 or weights.dtype != torch.float32 or terms.dim() != 1 or weights.shape != terms.shape \
            or not (terms.is_contiguous() and weights.is_contiguous()):
        raise ValueError(f"{what}: terms int32 [n] and weights float32 [n], contiguous, are needed")
    if len(start) != len(nnz):
        raise ValueError(f"{what}: one start per entry is needed")
    if not isinstance(nnz, torch.Tensor):
        _check_range(f"{what}_nnz", nnz, lo, hi)
        _check_range(f"{what}_start", start, 0, terms.shape[0] - np.maximum(np.asarray(nnz), 0))


def lexical_score(q_terms: torch.Tensor, q_weights: torch.Tensor, q_start, q_nnz, d_terms: torch.Tensor, d_weights: torch.Tensor,
                  d_start, d_nnz, cand=None, n_cand: Optional[int] = None, q_dense: Optional[torch.Tensor] = None,
                  d_dense: Optional[torch.Tensor] = None, hybrid_weights: Optional[Tuple[float, float]] = None):
    """``tt_lexical_score`` -> (lex, dense, hybrid), fp32 [n_q][n_cand] on the device; without ``q_dense``: (lex, None, None).
    Entries are (terms int32, weights fp32) device arrays, ascending by term within an entry; ``q_start`` / ``q_nnz`` (int32),
    ``d_start`` (int64) / ``d_nnz`` (int32, -1 = a tombstone), ``cand`` ([n_q][n_cand] int32 document numbers, < 0 = none; None:
    documents 0 .. n_cand-1 for every query): host arrays are checked against the kernel's limits (q_nnz 0 .. 512, d_nnz -1 ..
    8192, entries inside the arrays) and uploaded; device tensors are taken as they are -- their owner (``LexicalStore``,
    ``M3Encoder``) checked them when it made them, and the kernel clamps a length into its range.  ``q_dense`` [n_q][dim],
    ``d_dense`` [n_docs][dim] bfloat16 with ``hybrid_weights`` = (w_dense, w_lex)."""
    _check_entries("q", q_terms, q_weights, q_start, q_nnz, 0, MAX_QUERY_NNZ)
    _check_entries("d", d_terms, d_weights, d_start, d_nnz, -1, MAX_DOC_NNZ)
    n_q, n_docs = len(q_nnz), len(d_nnz)
    dim, wd, wl = 0, 0.0, 0.0
    if q_dense is not None:
        if d_dense is None or hybrid_weights is None:
            raise ValueError("lexical_score: q_dense needs d_dense and hybrid_weights = (w_dense, w_lex)")
        wd, wl = check_hybrid_weights({"hybrid_weights": hybrid_weights})
        if q_dense.dtype != torch.bfloat16 or d_dense.dtype != torch.bfloat16 or q_dense.dim() != 2 or d_dense.dim() != 2 \
                or q_dense.shape[1] != d_dense.shape[1] or not (q_dense.is_contiguous() and d_dense.is_contiguous()):
            raise ValueError("lexical_score: dense vectors must be contiguous bfloat16 [*, dim]")
        dim = int(q_dense.shape[1])
        if dim <= 0 or dim % 128 or dim > MAX_HIDDEN:
            raise NotImplementedError(f"lexical_score: dim={dim}: a multiple of 128 up to {MAX_HIDDEN}")
        if q_dense.shape[0] < n_q or d_dense.shape[0] < n_docs:
            raise ValueError(f"lexical_score: {q_dense.shape[0]} / {d_dense.shape[0]} dense rows for {n_q} queries / {n_docs} documents")
    if cand is None:
        n_cand = n_docs if n_cand is None else int(n_cand)
        if not 0 <= n_cand <= n_docs:
            raise ValueError(f"n_cand={n_cand} with {n_docs} documents")
    elif not isinstance(cand, torch.Tensor):
        cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(n_q, -1)
        if cand.size and cand.max() >= n_docs:
            raise ValueError(f"cand holds document number {int(cand.max())} with {n_docs} documents")
    dev = _need_device("lexical_score", q_terms, q_weights, d_terms, d_weights, *(() if q_dense is None else (q_dense, d_dense)))
    cand_t = None
    if cand is not None:
        cand_t = _dev_i(cand, torch.int32, dev)
        n_cand = int(cand_t.shape[1]) if cand_t.dim() == 2 else int(cand_t.numel() // max(n_q, 1))
    qs, qn = _dev_i(q_start, torch.int32, dev), _dev_i(q_nnz, torch.int32, dev)
    ds, dn = _dev_i(d_start, torch.int64, dev), _dev_i(d_nnz, torch.int32, dev)
    lex = torch.empty((n_q, n_cand), dtype=torch.float32, device=dev)
    dense = torch.empty_like(lex) if q_dense is not None else None
    hybrid = torch.empty_like(lex) if q_dense is not None else None
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        rc = lib.tt_lexical_score(q_terms.data_ptr(), q_weights.data_ptr(), qs.data_ptr(), qn.data_ptr(), n_q, d_terms.data_ptr(),
                                  d_weights.data_ptr(), ds.data_ptr(), dn.data_ptr(), cand_t.data_ptr() if cand_t is not None else None,
                                  n_cand, q_dense.data_ptr() if q_dense is not None else None,
                                  d_dense.data_ptr() if q_dense is not None else None, dim, wd, wl, lex.data_ptr(),
                                  dense.data_ptr() if dense is not None else None,
                                  hybrid.data_ptr() if hybrid is not None else None, _stream(dev))
    _lib.check(rc, "tt_lexical_score")
    return lex, dense, hybrid


def lexical_scan_topk(q_terms: torch.Tensor, q_weights: torch.Tensor, q_start, q_nnz, d_terms: torch.Tensor, d_weights: torch.Tensor,
                      d_start, d_nnz, k: int, workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``tt_lexical_scan_topk`` -> (scores fp32 [n_q][k], document numbers int32 [n_q][k]) on the device: the exact lexical top-k
    over every entry of the document arrays, ordered by (score descending, document number ascending), padded with (-inf, -1);
    tombstones (``d_nnz`` -1) are never returned.  1 .. 64 queries, k 1 .. 1024; the arrays are checked as ``lexical_score``'s."""
    n_q, n_docs = len(q_nnz), len(d_nnz)
    if not 1 <= n_q <= MAX_SCAN_QUERIES:
        raise ValueError(f"lexical_scan_topk: {n_q} queries (1 .. {MAX_SCAN_QUERIES})")
    if not 1 <= int(k) <= MAX_SCAN_K:
        raise ValueError(f"lexical_scan_topk: k={k} (1 .. {MAX_SCAN_K})")
    _check_entries("q", q_terms, q_weights, q_start, q_nnz, 0, MAX_QUERY_NNZ)
    _check_entries("d", d_terms, d_weights, d_start, d_nnz, -1, MAX_DOC_NNZ)
    dev = _need_device("lexical_scan_topk", q_terms, q_weights, d_terms, d_weights)
    qs, qn = _dev_i(q_start, torch.int32, dev), _dev_i(q_nnz, torch.int32, dev)
    ds, dn = _dev_i(d_start, torch.int64, dev), _dev_i(d_nnz, torch.int32, dev)
    lib = _lib.load_library()
    need = int(lib.tt_lexical_scan_workspace_bytes(n_docs, n_q))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    scores = torch.empty((n_q, int(k)), dtype=torch.float32, device=dev)
    idx = torch.empty((n_q, int(k)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.tt_lexical_scan_topk(q_terms.data_ptr(), q_weights.data_ptr(), qs.data_ptr(), qn.data_ptr(), n_q, d_terms.data_ptr(),
                                      d_weights.data_ptr(), ds.data_ptr(), dn.data_ptr(), n_docs, int(k), scores.data_ptr(),
                                      idx.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                      _stream(dev))
    _lib.check(rc, "tt_lexical_scan_topk")
    return scores, idx


def hybrid_scan_topk(q_terms: torch.Tensor, q_weights: torch.Tensor, q_start, q_nnz, d_terms: torch.Tensor, d_weights: torch.Tensor,
                     d_start, d_nnz, q_dense: torch.Tensor, d_dense: torch.Tensor, hybrid_weights: Tuple[float, float], k: int,
                     workspace: Optional[torch.Tensor] = None, max_q_nnz: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``tt_hybrid_scan_topk`` -> (scores fp32 [n_q][k], document numbers int32 [n_q][k]) on the device: the exact top-k by the
    hybrid score ``(w_dense * <q, d> + w_lex * lex(q, d)) / (w_dense + w_lex)`` over every entry of the document arrays, each
    score ``lexical_score``'s hybrid bits for the pair; ordered by (score descending, document number ascending), padded with
    (-inf, -1); tombstones (``d_nnz`` -1) are never returned.  1 .. 64 queries, k 1 .. 1024; the arrays and the dense vectors
    (contiguous bfloat16 ``q_dense`` [n_q][dim], ``d_dense`` [n_docs][dim]) are checked as ``lexical_score``'s.  ``max_q_nnz``: the
    longest query entry, which sizes the kernel's LDS slots -- taken from a host ``q_nnz``; with a device ``q_nnz`` it is the
    caller's promise (default 512, the widest slot).  After the call ``workspace`` (caller-owned, optional) holds every score:
    row q, ``n_docs`` rounded up to 32 floats apart."""
    n_q, n_docs = len(q_nnz), len(d_nnz)
    if not 1 <= n_q <= MAX_SCAN_QUERIES:
        raise ValueError(f"hybrid_scan_topk: {n_q} queries (1 .. {MAX_SCAN_QUERIES})")
    if not 1 <= int(k) <= MAX_SCAN_K:
        raise ValueError(f"hybrid_scan_topk: k={k} (1 .. {MAX_SCAN_K})")
    _check_entries("q", q_terms, q_weights, q_start, q_nnz, 0, MAX_QUERY_NNZ)
    _check_entries("d", d_terms, d_weights, d_start, d_nnz, -1, MAX_DOC_NNZ)
    if not isinstance(q_nnz, torch.Tensor):
        max_q_nnz = int(np.max(q_nnz)) if max_q_nnz is None else max(int(max_q_nnz), int(np.max(q_nnz)))
    elif max_q_nnz is None:
        max_q_nnz = MAX_QUERY_NNZ
    if not 0 <= int(max_q_nnz) <= MAX_QUERY_NNZ:
        raise ValueError(f"hybrid_scan_topk: max_q_nnz={max_q_nnz} (0 .. {MAX_QUERY_NNZ})")
    wd, wl = check_hybrid_weights({"hybrid_weights": hybrid_weights})
    if q_dense is None or d_dense is None or q_dense.dtype != torch.bfloat16 or d_dense.dtype != torch.bfloat16 \
            or q_dense.dim() != 2 or d_dense.dim() != 2 or q_dense.shape[1] != d_dense.shape[1] \
            or not (q_dense.is_contiguous() and d_dense.is_contiguous()):
        raise ValueError("hybrid_scan_topk: dense vectors must be contiguous bfloat16 [*, dim]")
    dim = int(q_dense.shape[1])
    if dim <= 0 or dim % 128 or dim > MAX_HIDDEN:
        raise NotImplementedError(f"hybrid_scan_topk: dim={dim}: a multiple of 128 up to {MAX_HIDDEN}")
    if q_dense.shape[0] < n_q or d_dense.shape[0] < n_docs:
        raise ValueError(f"hybrid_scan_topk: {q_dense.shape[0]} / {d_dense.shape[0]} dense rows for {n_q} queries / {n_docs} documents")
    dev = _need_device("hybrid_scan_topk", q_terms, q_weights, d_terms, d_weights, q_dense, d_dense)
    qs, qn = _dev_i(q_start, torch.int32, dev), _dev_i(q_nnz, torch.int32, dev)
    ds, dn = _dev_i(d_start, torch.int64, dev), _dev_i(d_nnz, torch.int32, dev)
    if q_terms.numel() == 0:      # (queries without a kept token still have a dense score; the entry point takes no null array)
        q_terms, q_weights = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    if d_terms.numel() == 0 and n_docs:
        d_terms, d_weights = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
    lib = _lib.load_library()
    need = int(lib.tt_hybrid_scan_workspace_bytes(n_docs, n_q))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
    scores = torch.empty((n_q, int(k)), dtype=torch.float32, device=dev)
    idx = torch.empty((n_q, int(k)), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.tt_hybrid_scan_topk(q_terms.data_ptr(), q_weights.data_ptr(), qs.data_ptr(), qn.data_ptr(), n_q, int(max_q_nnz),
                                     d_terms.data_ptr(), d_weights.data_ptr(), ds.data_ptr(), dn.data_ptr(), n_docs,
                                     q_dense.data_ptr(), d_dense.data_ptr(), dim, wd, wl, int(k), scores.data_ptr(), idx.data_ptr(),
                                     workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream(dev))
    _lib.check(rc, "tt_hybrid_scan_topk")
    return scores, idx


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
@dataclass
class LexicalWeights:
    """Packed lexical vectors of several texts: text i owns entries ``starts[i] .. starts[i] + nnz[i] - 1`` of ``terms`` (token
    ids, ascending) and ``weights``."""

    terms: torch.Tensor        # int32 [sum(nnz)], device
    weights: torch.Tensor      # float32 [sum(nnz)], device
    starts: np.ndarray         # int64 [n]
    nnz: np.ndarray            # int32 [n]

    def __len__(self) -> int:
        return len(self.nnz)

    def as_dicts(self) -> List[Dict[int, float]]:
        """Upstream's form: one ``{token id: weight}`` per text."""
        t, w = self.terms.cpu().numpy(), self.weights.cpu().numpy()
        return [{int(a): float(b) for a, b in zip(t[s:s + n], w[s:s + n])} for s, n in zip(self.starts, self.nnz)]


class M3Encoder:
    """One forward per batch -> the dense vector AND the lexical weights of every text, on the weights of an existing
    ``HipHuggingFaceEmbedding`` (an XLM-R checkpoint whose directory ships ``sparse_linear.pt``), in whichever precision that
    embedder was built.  Nothing of the embedder is changed: its own methods give the same bits before and after.

    ``head``: (w [H], bias) instead of the directory's file (synthetic weights: benchmarks)."""

    def __init__(self, embedder, head: Optional[Tuple[torch.Tensor, float]] = None):
        cfg = getattr(embedder, "config", None)
        if cfg is None or getattr(cfg, "arch", None) != "xlmr":
            raise NotImplementedError(f"M3Encoder: architecture {getattr(cfg, 'arch', None)!r}: the lexical head belongs to XLM-R "
                                      "checkpoints (BAAI/bge-m3)")
        if embedder.pooling != "cls":
            raise NotImplementedError(f"M3Encoder: pooling '{embedder.pooling}': BGE-M3's dense vector is the CLS row")
        if cfg.hidden % 128 or cfg.hidden > MAX_HIDDEN:
            raise NotImplementedError(f"M3Encoder: hidden size {cfg.hidden}: a multiple of 128 up to {MAX_HIDDEN}")
        if head is None:
            mdir = getattr(embedder, "model_dir", None)
            if not has_lexical_head(mdir):
                raise FileNotFoundError(f"M3Encoder: {embedder.model_name}: directory {mdir!r} has no {SPARSE_FILE} (the lexical head)")
            head = load_sparse_head(mdir, cfg.hidden)
        w, bias = head
        if tuple(w.shape) != (cfg.hidden,):
            raise ValueError(f"M3Encoder: head weight {tuple(w.shape)} does not match [{cfg.hidden}]")
        self.embedder, self.cfg, self.device = embedder, cfg, embedder.device
        self._enc = embedder._encoder
        self.path = self._enc.path
        # the head in the element type of the path's hidden states (upstream's fp16 mode holds it in fp16 too); the bias in fp32
        self.w = w.to(device=self.device, dtype=self.path.hidden).contiguous()
        self.bias = float(bias)
        self.skip = special_ids(embedder._tokenizer)
        self.max_length = min(embedder.max_length, MAX_SEQ_LEN)

    def parameters(self):
        yield self.w

    def _tokens(self, items, is_query: bool) -> List[Sequence[int]]:
        emb = self.embedder
        texts = [x for x in items if isinstance(x, str)]
        if len(texts) == len(items):
            return emb._tokenize(texts, emb.query_instruction if is_query else emb.text_instruction)
        if texts:
            raise ValueError("M3Encoder.encode: either strings or token-id sequences, not both")
        return list(items)

    def _encode_batch(self, seqs: List[Sequence[int]]):
        """-> (dense fp32 [B][H], terms, weights, row of every sequence's first slot, nnz (device))."""
        enc, p, dev, H = self._enc, self.path, self.device, self.cfg.hidden
        # the rows the forward really runs on: the path's own padding (whole GEMM tiles) behind the packed batch's
        batch = enc._padded(pack_tokens(seqs, self.cfg, None, self.max_length))
        hidden, starts, lens = enc.forward_packed(batch, want_lens=True)
        B = len(batch.seq_len)
        dense = torch.empty((B, H), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = getattr(enc.lib, p.pool)(hidden.data_ptr(), H, starts.data_ptr(), B, H, dense.data_ptr(), None, _stream(dev))
        _lib.check(rc, p.pool)
        ids = torch.from_numpy(batch.ids).to(dev)
        terms, weights, nnz = lexical_weights(hidden, self.w, self.bias, ids, starts, lens, self.skip, max_len=batch.max_len)
        self._after_forward(hidden, batch)
        return dense, terms, weights, batch.seq_start, nnz

    def _after_forward(self, hidden: torch.Tensor, batch) -> None:
        """What a subclass reads from a batch's hidden state beside the two heads here (``multivec.M3MultiVectorEncoder``: the
        token vectors).  Nothing in this class."""

    def encode(self, items, is_query: bool = False) -> Tuple[torch.Tensor, LexicalWeights]:
        """``items``: strings (the embedder's query / text instruction is put in front, as its own methods do), or token-id
        sequences that already carry their special tokens (what ``embed_token_batches`` takes) -> (dense fp32 [n][H]
        L2-normalised, on the device; ``LexicalWeights``), original order.  Batches are formed as the embedder forms them; a text's
        result does not depend on the batch it travels in."""
        if len(items) == 0:
            raise ValueError("M3Encoder.encode: nothing to encode")
        emb = self.embedder
        seqs = self._tokens(items, is_query)
        n = len(seqs)
        order = sorted(range(n), key=lambda i: -len(seqs[i]))
        dense = torch.empty((n, self.cfg.hidden), dtype=torch.float32, device=self.device)
        nnz = np.zeros(n, dtype=np.int32)
        pieces: List[Tuple[torch.Tensor, torch.Tensor, np.ndarray, np.ndarray]] = []   # (terms, weights, first slots, texts)
        lo = 0
        while lo < n:
            hi, tokens = lo, 0
            while hi < n and (hi - lo < emb.embed_batch_size or tokens < emb.forward_tokens):
                tokens += min(len(seqs[order[hi]]), self.max_length)
                hi += 1
            sel = np.asarray(order[lo:hi], dtype=np.int64)
            d, t, w, first, cnt = self._encode_batch([seqs[i] for i in sel])
            dense[torch.from_numpy(sel).to(self.device)] = d
            nnz[sel] = cnt.cpu().numpy()
            pieces.append((t, w, np.asarray(first, dtype=np.int64), sel))
            lo = hi
        starts = np.zeros(n, dtype=np.int64)
        np.cumsum(nnz[:-1], out=starts[1:])
        total = int(nnz.sum())
        terms = torch.empty((total,), dtype=torch.int32, device=self.device)
        weights = torch.empty((total,), dtype=torch.float32, device=self.device)
        for t, w, first, sel in pieces:      # one gather per batch: slot first[i] + j of the batch -> starts[text] + j
            cnt = nnz[sel].astype(np.int64)
            if int(cnt.sum()) == 0:
                continue
            within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            src = torch.from_numpy(np.repeat(first, cnt) + within).to(self.device)
            dst = torch.from_numpy(np.repeat(starts[sel], cnt) + within).to(self.device)
            terms[dst] = t[src]
            weights[dst] = w[src]
        return dense, LexicalWeights(terms, weights, starts, nnz)


# ---- the store ----------------------------------------------------------------------------------------------------------------------
class LexicalStore:
    """Lexical vectors and -- with ``dim`` > 0 -- dense rows of indexed passages, in HBM on one device: CSR arrays (``d_start``
    int64, ``d_nnz`` int32 per document; ``terms`` int32 and ``weights`` fp32 per distinct token: 8 bytes) plus one bf16 dense row
    of ``dim`` values per document number (``dim`` 0 or None: no dense rows, ``dense`` is None and ``add`` takes none -- what
    ``splade.SpladeStore`` is).  ``add`` appends and grows by doubling; ``remove`` frees the id and writes ``d_nnz = -1`` on the
    device, so that neither ``score`` nor ``search`` returns the document -- its entries stay where they are and are NOT reclaimed
    (there is no compaction in this version; re-adding an id appends a new copy and buries the older one).  No persistence.

    ``postings=True`` (with ``vocab_size``, the ids' range): ``seal()`` builds posting lists over the documents stored so far
    (``postings.py``: 4 bytes per entry + 12 per vocabulary id), and ``search`` then scores only the documents on the query's own
    lists plus the unsealed tail -- the same scores and document numbers as the full scan, bit for bit.  ``add`` leaves new
    documents in the tail and re-seals once the tail exceeds ``max(65536, n_sealed / 4)`` documents; ``remove`` leaves the lists
    alone (a tombstone on a list scores NaN and is never selected).  ``stats``: the last search's figures."""

    def __init__(self, dim: Optional[int], device: torch.device, capacity_terms: int = 1 << 16, capacity_docs: int = 1 << 10,
                 postings: bool = False, vocab_size: Optional[int] = None):
        name, dim = type(self).__name__, int(dim or 0)
        if dim < 0 or dim % 128 or dim > MAX_HIDDEN:
            raise ValueError(f"{name}: dim={dim} (a multiple of 128 up to {MAX_HIDDEN})")
        self.postings = bool(postings)
        if self.postings and (vocab_size is None or int(vocab_size) < 1):
            raise ValueError(f"postings=True needs vocab_size (every stored id lies in [0, vocab_size)), not {vocab_size!r}")
        if device.type != "cuda":
            raise RuntimeError(f"{name} lives on a HIP device; tensor_truth_amd has no CPU path")
        self.dim, self.device = dim, device
        self.terms = torch.zeros(max(capacity_terms, 1), dtype=torch.int32, device=device)
        self.weights = torch.zeros(max(capacity_terms, 1), dtype=torch.float32, device=device)
        self.d_start = torch.zeros(max(capacity_docs, 1), dtype=torch.int64, device=device)
        self.d_nnz = torch.zeros(max(capacity_docs, 1), dtype=torch.int32, device=device)
        self.dense = torch.zeros((max(capacity_docs, 1), dim), dtype=torch.bfloat16, device=device) if dim else None
        self.n_terms = 0
        self.n_docs = 0
        self._ids = IdTable()
        self._ws: Optional[torch.Tensor] = None
        self.vocab_size = None if vocab_size is None else int(vocab_size)
        self.index = None                    # postings.PostingsIndex over documents [0, index.n_sealed)
        self._pws: Optional[torch.Tensor] = None
        self.stats: Dict[str, int] = {}

    @property
    def n_sealed(self) -> int:
        return 0 if self.index is None else self.index.n_sealed

    def seal(self) -> None:
        """Build the posting lists over every document stored so far (live or tombstoned); ``search`` uses them from now on."""
        from . import postings as _postings

        if not self.postings:
            raise RuntimeError("seal: the store was made without postings=True")
        self.index = None                    # (the old lists are freed before the new ones are allocated)
        self.index = _postings.postings_build(self.terms, self.weights, self.d_start, self.d_nnz, self.n_docs, self.vocab_size,
                                              self.n_terms)

    def _check_vocab(self, lexical: "LexicalWeights") -> None:
        """With postings on, an id outside the vocabulary is refused when it is added, not when a later re-seal meets it."""
        if self.postings and lexical.terms.numel():
            lo, hi = int(lexical.terms.min()), int(lexical.terms.max())
            if lo < 0 or hi >= self.vocab_size:
                raise ValueError(f"add: id {lo if lo < 0 else hi} is outside the vocabulary [0, {self.vocab_size})")

    def _after_add(self) -> None:
        if self.postings and self.n_docs - self.n_sealed > max(65536, self.n_sealed // 4):
            self.seal()

    def __len__(self) -> int:
        return len(self._ids)

    def add(self, node_ids: Sequence[Any], lexical: LexicalWeights, dense: Optional[torch.Tensor] = None) -> np.ndarray:
        """Append the passages' lexical vectors and -- exactly when the store has dense rows -- their dense rows (fp32 or bf16
        [n][dim]; rounded to bf16 to nearest even) -> their document numbers."""
        nnz = np.ascontiguousarray(lexical.nnz, dtype=np.int32)
        n = len(nnz)
        if (dense is None) == bool(self.dim):
            raise ValueError(f"add: dense rows are needed by a store with dim={self.dim}" if self.dim else
                             "add: dense rows are not taken by a store without them (dim=0)")
        if len(node_ids) != n or (dense is not None and (dense.dim() != 2 or tuple(dense.shape) != (n, self.dim))):
            raise ValueError(f"add: {len(node_ids)} node ids, {n} lexical vectors" + (" do not match" if dense is None else
                             f" and dense {tuple(dense.shape)} do not match [n][{self.dim}]"))
        _check_range("nnz", nnz, 0, MAX_DOC_NNZ)
        total = int(nnz.sum())
        if lexical.terms.numel() != total or lexical.weights.numel() != total:
            raise ValueError(f"add: {lexical.terms.numel()} terms for {total} entries")
        want = np.zeros(n, dtype=np.int64)
        np.cumsum(nnz[:-1], out=want[1:])
        if n and not np.array_equal(np.asarray(lexical.starts, dtype=np.int64), want):
            raise ValueError("add: packed lexical vectors are needed (text i right behind text i-1)")
        if n == 0:
            return np.zeros(0, dtype=np.int32)
        self._check_vocab(lexical)
        self.terms = grown(self.terms, self.n_terms, self.n_terms + total)
        self.weights = grown(self.weights, self.n_terms, self.n_terms + total)
        self.d_start = grown(self.d_start, self.n_docs, self.n_docs + n)
        self.d_nnz = grown(self.d_nnz, self.n_docs, self.n_docs + n)
        self.terms[self.n_terms:self.n_terms + total].copy_(lexical.terms.to(self.device))
        self.weights[self.n_terms:self.n_terms + total].copy_(lexical.weights.to(self.device))
        self.d_start[self.n_docs:self.n_docs + n].copy_(torch.from_numpy(want + self.n_terms))
        self.d_nnz[self.n_docs:self.n_docs + n].copy_(torch.from_numpy(nnz))
        if dense is not None:
            self.dense = grown(self.dense, self.n_docs, self.n_docs + n)
            self.dense[self.n_docs:self.n_docs + n].copy_(dense.to(device=self.device, dtype=torch.bfloat16))
        docs = np.arange(self.n_docs, self.n_docs + n, dtype=np.int32)
        for old in self._ids.assign(node_ids):           # re-added: the older copy becomes a tombstone
            self.d_nnz[old:old + 1].fill_(-1)
        self.n_terms += total
        self.n_docs += n
        self._after_add()
        return docs

    def remove(self, node_id: Any) -> bool:
        """Forget ``node_id`` -> whether it was stored.  Its document number becomes a tombstone; its entries are not reclaimed."""
        doc = self._ids.pop(node_id)
        if doc is None:
            return False
        self.d_nnz[doc:doc + 1].fill_(-1)
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
        return sum(t.numel() * t.element_size() for t in (self.terms, self.weights, self.d_start, self.d_nnz, self.dense)
                   if t is not None) + (0 if self.index is None else self.index.nbytes)

    @staticmethod
    def _check_query(lexical: LexicalWeights) -> np.ndarray:
        _check_range("q_nnz", lexical.nnz, 0, MAX_QUERY_NNZ)
        return np.asarray(lexical.starts).astype(np.int32)

    def score(self, lexical: LexicalWeights, cand, dense: Optional[torch.Tensor] = None,
              hybrid_weights: Optional[Tuple[float, float]] = None):
        """Every query against its row of ``cand`` (document numbers, -1 = none) -> (lex, dense, hybrid) fp32 [n_q][n_cand] on
        the device ((lex, None, None) without ``dense``, the queries' fp32 or bf16 [n_q][dim] vectors).  A removed document
        scores -inf."""
        cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(len(lexical), -1)
        if cand.size and cand.max() >= self.n_docs:
            raise ValueError(f"document number {int(cand.max())} with {self.n_docs} documents stored")
        qd = None if dense is None else dense.to(device=self.device, dtype=torch.bfloat16).contiguous()
        return lexical_score(lexical.terms, lexical.weights, self._check_query(lexical), lexical.nnz, self.terms, self.weights,
                             self.d_start[: self.n_docs], self.d_nnz[: self.n_docs], cand=cand, q_dense=qd,
                             d_dense=None if qd is None else self.dense, hybrid_weights=hybrid_weights)

    def search(self, lexical: LexicalWeights, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The exact lexical top-k over every stored document -> (scores fp32 [n_q][k], document numbers int32 [n_q][k]) on the
        device, ordered by (score descending, document number ascending), padded with (-inf, -1).  Removed documents are never
        returned; a document that shares no id with the query scores 0 and is a valid result.  With posting lists built
        (``seal``), only the documents on the query's lists and the unsealed tail are scored -- the same result, bit for bit
        (``postings.search``); ``stats`` then holds the search's figures."""
        if self.index is not None and self.n_docs > 0:
            from . import postings as _postings

            return _postings.search(self, lexical, k)
        need = int(_lib.load_library().tt_lexical_scan_workspace_bytes(self.n_docs, len(lexical)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return lexical_scan_topk(lexical.terms, lexical.weights, self._check_query(lexical), lexical.nnz, self.terms, self.weights,
                                 self.d_start[: self.n_docs], self.d_nnz[: self.n_docs], k, workspace=self._ws)

    def search_hybrid(self, lexical: LexicalWeights, dense: torch.Tensor, k: int,
                      hybrid_weights: Tuple[float, float]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The exact top-k by the hybrid score ``(w_dense * <q, d> + w_lex * lex(q, d)) / (w_dense + w_lex)`` over every stored
        document -> (scores fp32 [n_q][k], document numbers int32 [n_q][k]) on the device, ordered by (score descending, document
        number ascending), padded with (-inf, -1); each score is ``score``'s hybrid bits for the pair.  ``dense``: the queries'
        fp32 or bf16 [n_q][dim] vectors.  Removed documents are never returned.  This is ALWAYS the full scan
        (``tt_hybrid_scan_topk``: one read of the store per pass of queries), also when posting lists are sealed: a passage that
        shares no id with the query still has a dense score, so the lists cannot bound the result.  A store without dense rows
        (``dim`` 0) has no hybrid score."""
        if not self.dim:
            raise ValueError(f"search_hybrid: {type(self).__name__} holds no dense rows (dim=0): there is no hybrid score")
        if dense is None or dense.dim() != 2 or tuple(dense.shape) != (len(lexical), self.dim):
            raise ValueError(f"search_hybrid: dense {None if dense is None else tuple(dense.shape)} does not match "
                             f"[{len(lexical)}][{self.dim}]")
        qs = self._check_query(lexical)
        qd = dense.to(device=self.device, dtype=torch.bfloat16).contiguous()
        n_q = len(lexical)
        need = int(_lib.load_library().tt_hybrid_scan_workspace_bytes(self.n_docs, n_q)) if 1 <= n_q <= MAX_SCAN_QUERIES else 0
        if self._ws is None or self._ws.numel() < need:      # (the scratch `search` caches: either call leaves nothing in it to keep)
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        return hybrid_scan_topk(lexical.terms, lexical.weights, qs, lexical.nnz, self.terms, self.weights,
                                self.d_start[: self.n_docs], self.d_nnz[: self.n_docs], qd, self.dense, hybrid_weights, k,
                                workspace=self._ws)


# ---- postprocessor and retriever ---------------------------------------------------------------------------------------------------
class _M3Model:
    """The weights behind a ``HipM3HybridRerank``: the embedder's encoder and the lexical head (``.parameters()`` for
    ModelManager-style memory accounting)."""

    def __init__(self, embedder, encoder: M3Encoder):
        self.embedder, self.head = embedder, encoder

    def parameters(self):
        yield from self.embedder._model.parameters()
        yield from self.head.parameters()

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.parameters())


class HipM3HybridRerank(_StoredRerank):
    """Hybrid (dense + lexical) rerank postprocessor with the surface of ``HipColbertRerank``: ``postprocess_nodes`` (keyword or
    positional), ``rerank``, ``predict``, ``.model`` (with ``.parameters()``), ``index_nodes``, ``stats``.  ``index_nodes`` encodes
    nodes' EMBED-mode content once into the instance's ``LexicalStore`` (and keeps the nodes, for ``HipLexicalRetriever``).  At
    query time one forward gives the query's dense vector and lexical weights; a stored node is scored from the store and any
    other node is encoded in the call -- both give the same bits for the same text.  The node score is the hybrid score
    ``(w_dense * <q, d> + w_lex * lex(q, d)) / (w_dense + w_lex)`` with ``model_kwargs["hybrid_weights"] = (w_dense, w_lex)``
    (required; ``(0, 1)``: pure lexical scores, ``(1, 0)``: the dense ranking).

    ``model_kwargs["embedder"]``: an existing ``HipHuggingFaceEmbedding`` to share (its weights are not loaded a second time).
    ``model_kwargs["postings"] = True``: the store searches through posting lists (``LexicalStore``; the same results, bit for bit)."""

    def __init__(self, model: str = "BAAI/bge-m3", top_n: int = 2, device: Optional[str] = None, keep_retrieval_score: bool = False,
                 model_kwargs: Optional[Dict[str, Any]] = None, **_ignored):
        mk = dict(model_kwargs or {})
        self.hybrid_weights = check_hybrid_weights(mk)
        mk.pop("hybrid_weights")
        embedder = mk.pop("embedder", None)
        head = mk.pop("sparse_head", None)
        postings = bool(mk.pop("postings", False))
        if embedder is None:
            from .embedding import HipHuggingFaceEmbedding

            embedder = HipHuggingFaceEmbedding(model_name=model, device=device, model_kwargs=mk)
        self.model_name, self.top_n, self.keep_retrieval_score = model, top_n, keep_retrieval_score
        self.embedder, self.device, self.config = embedder, embedder.device, embedder.config
        self.encoder = M3Encoder(embedder, head=head)
        self.model = _M3Model(embedder, self.encoder)
        # model_kwargs["postings"]: the store searches through posting lists (HipLexicalRetriever builds them before its first query)
        self.store = LexicalStore(self.config.hidden, self.device, postings=postings, vocab_size=self.config.vocab_size)
        self.precision = embedder.precision
        self.nodes: Dict[Any, Any] = {}      # node id -> the indexed node (what HipLexicalRetriever returns)
        self.stats = {"queries": 0, "stored": 0, "encoded": 0}

    def remove_node(self, node_id: Any) -> bool:
        self.nodes.pop(node_id, None)
        return self.store.remove(node_id)

    # ---- what _StoredRerank asks for --------------------------------------------------------------------------------
    def encode_queries(self, texts):
        return self.encoder.encode(texts, is_query=True)

    def encode_documents(self, texts):
        return self.encoder.encode(texts, is_query=False)

    def add_documents(self, nodes, encoded) -> None:
        dense, lw = encoded
        self.store.add([n.id_ for n in nodes], lw, dense)
        self.nodes.update((n.id_, n) for n in nodes)

    def lookup(self, ids) -> np.ndarray:
        return self.store.lookup(ids)

    def score_stored(self, q, cands) -> np.ndarray:
        q_dense, q_lw = q
        return self.store.score(q_lw, cands[0], dense=q_dense, hybrid_weights=self.hybrid_weights)[2].cpu().numpy()

    def score_fresh(self, q, d, cand) -> np.ndarray:
        (q_dense, q_lw), (d_dense, d_lw) = q, d
        _check_range("d_nnz", d_lw.nnz, 0, MAX_DOC_NNZ)
        return lexical_score(q_lw.terms, q_lw.weights, LexicalStore._check_query(q_lw), q_lw.nnz, d_lw.terms, d_lw.weights, d_lw.starts,
                             d_lw.nnz, cand=cand, q_dense=q_dense.to(torch.bfloat16), d_dense=d_dense.to(torch.bfloat16),
                             hybrid_weights=self.hybrid_weights)[2].cpu().numpy()


class HipLexicalRetriever:
    """Exact lexical retrieval over the nodes a ``HipM3HybridRerank`` indexed: ``retrieve(query)`` encodes the query (one short
    forward), runs ``LexicalStore.search`` and returns the best ``similarity_top_k`` stored nodes by lexical score, best first.
    Hits with score <= 0 -- passages that share no weighted token with the query -- are dropped."""

    def __init__(self, reranker: HipM3HybridRerank, similarity_top_k: int = 10):
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
        _, lw = rr.encoder.encode([query_bundle.query_str], is_query=True)
        return top_nodes(rr.store, lw, self.similarity_top_k, rr.nodes, node_type)


class HipM3HybridRetriever:
    """Exact retrieval by BGE-M3's hybrid ("dense+sparse") score over the nodes a ``HipM3HybridRerank`` indexed:
    ``retrieve(query)`` encodes the query (one short forward gives both heads), runs ``LexicalStore.search_hybrid`` with the
    reranker's own ``hybrid_weights`` and returns the best ``similarity_top_k`` stored nodes, best first, each with the score
    ``postprocess_nodes`` gives it.  A hybrid score has no "no shared token" point, so every hit is kept -- except with
    ``w_dense == 0``, where the score is the lexical one and the result is ``HipLexicalRetriever``'s (scores <= 0 dropped)."""

    def __init__(self, reranker: HipM3HybridRerank, similarity_top_k: int = 10):
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
        w_dense, w_lex = rr.hybrid_weights
        dense, lw = rr.encoder.encode([query_bundle.query_str], is_query=True)
        return top_nodes(rr.store, lw, self.similarity_top_k, rr.nodes, node_type, positive_only=w_dense == 0,
                         search=lambda q, k: rr.store.search_hybrid(q, dense, k, (w_dense, w_lex)))
