"""Reranking with all three heads of ``BAAI/bge-m3`` on the HIP path: dense + lexical + multi-vector ("colbert+sparse+dense").

Beside the encoder and ``sparse_linear.pt`` (``lexical.py``) a BGE-M3 directory ships ``colbert_linear.pt``: a hidden-size-wide linear
layer WITH a bias that turns the last hidden state the embedder already computes into one L2-normalised vector per token -- every row
but the first (``<s>`` is dropped, ``</s>`` is kept).  A pair's multi-vector score is the MEAN over the query's vectors of the maximum
dot product with the passage's vectors; the combined score mixes it with the dense dot product and the lexical score.  The head is as
wide as the model (1024 for bge-m3) and its texts run to 8192 tokens, which the late-interaction kernels of ``colbert.py`` (dim <= 128,
128 query and 512 document rows, no bias, a sum) do not take: ``tt_multivec_project``, ``tt_maxsim_wide`` and ``tt_m3_mix``
(csrc/multivec.hip) are their wide forms.

Passages are encoded ONCE, when they are indexed, into a ``LexicalStore`` (dense row + lexical vector) and a ``MultiVectorStore``
(2 * dim bytes per kept token plus 12 bytes per passage: a 180-token passage at dim 1024 is about 369 KB -- a rerank-stage store for a
working set, not the corpus).  A query costs one short forward, one projection and three scoring kernels.

[UPSTREAM-K] The semantics are written from knowledge of FlagEmbedding's ``BGEM3FlagModel`` (``colbert_linear.pt`` with ``weight``
[dim][H] and ``bias`` [dim]; ``_process_colbert_vecs`` / ``colbert_score``: ``last_hidden_state[:, 1:]`` projected, normalised, the
mean over the query's tokens of the maxima; "colbert+sparse+dense" in ``compute_score``, example weights (0.4, 0.2, 0.4)), which is not
installed here and cannot be checked offline.  The loader is therefore strict: a key or a shape it does not know is refused by name,
``dim`` is read from the tensor, and the three mixing weights are never defaulted.
"""
from __future__ import annotations

import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._hostargs import _check_range, _dev_i, _stream
from ._stored import _StoredRerank
from .colbert import TokenVectors, TokenVectorStore, _maxsim
from .lexical import (MAX_DOC_NNZ, SPARSE_FILE, LexicalStore, LexicalWeights, M3Encoder, _M3Model, has_lexical_head, lexical_score,
                      load_sparse_head)

COLBERT_FILE = "colbert_linear.pt"
# the kernels' limits (include/tt_hip.h)
MAX_QUERY_LEN, MAX_DOC_LEN, MAX_DIM, MAX_HIDDEN, DIM_STEP = 512, 8192, 1024, 1024, 128
DOC_STEP = 64          # document rows a MaxSim workgroup takes per step (4 waves x 16 rows): what the placement tests straddle


# ---- checkpoint --------------------------------------------------------------------------------------------------------------------
def has_multivector_head(model_dir: Optional[str]) -> bool:
    """Whether ``model_dir`` is a directory that ships ``colbert_linear.pt``."""
    return bool(model_dir) and os.path.isfile(os.path.join(model_dir, COLBERT_FILE))


def load_colbert_head(model_dir: str, hidden: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``colbert_linear.pt`` -> (W fp32 [dim][hidden], b fp32 [dim]) on the host.  [UPSTREAM-K] a torch-pickled state dict with
    ``weight`` [dim][hidden] and ``bias`` [dim]; ``dim`` is the tensor's; any other key or shape is refused by name."""
    path = os.path.join(model_dir or "", COLBERT_FILE)
    if not has_multivector_head(model_dir):
        raise FileNotFoundError(f"{path} not found: the directory has no multi-vector head (a BGE-M3 checkpoint ships it beside "
                                "model.safetensors)")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: a state dict is expected, not {type(sd).__name__}")
    unknown = sorted(set(sd) - {"weight", "bias"})
    if unknown:
        raise NotImplementedError(f"{path} carries tensors the multi-vector head does not compute: {unknown[:4]}")
    missing = [k for k in ("weight", "bias") if k not in sd]
    if missing:
        raise ValueError(f"{path} has no {missing}: not a multi-vector head")
    w, b = sd["weight"], sd["bias"]
    if not isinstance(w, torch.Tensor) or w.dim() != 2 or w.shape[1] != hidden or w.shape[0] < 1:
        raise ValueError(f"{path}: weight {tuple(getattr(w, 'shape', ()))} does not match [dim][{hidden}]")
    dim = int(w.shape[0])
    if not isinstance(b, torch.Tensor) or tuple(b.shape) != (dim,):
        raise ValueError(f"{path}: bias {tuple(getattr(b, 'shape', ()))} does not match [{dim}]")
    return w.to(torch.float32).contiguous(), b.to(torch.float32).contiguous()


def check_m3_weights(model_kwargs: Optional[dict]) -> Tuple[float, float, float]:
    """``model_kwargs["m3_weights"] = (w_dense, w_lex, w_mv)``: required, all >= 0, finite, not all 0.  Never defaulted (upstream's
    example uses 0.4, 0.2, 0.4)."""
    mw = (model_kwargs or {}).get("m3_weights")
    if mw is None:
        raise ValueError("model_kwargs['m3_weights'] = (w_dense, w_lex, w_mv) is missing: the three weights of the combined score are "
                         "the caller's and are never defaulted")
    try:
        vals = tuple(float(x) for x in mw)
    except (TypeError, ValueError):
        raise ValueError(f"model_kwargs['m3_weights']={mw!r}: three numbers (w_dense, w_lex, w_mv) are expected") from None
    if len(vals) != 3:
        raise ValueError(f"model_kwargs['m3_weights']={mw!r}: three numbers (w_dense, w_lex, w_mv) are expected")
    if not (all(v >= 0 for v in vals) and sum(vals) > 0 and np.isfinite(sum(vals))):
        raise ValueError(f"model_kwargs['m3_weights']={mw!r}: all weights >= 0, finite and not all 0")
    return vals


# ---- host wrappers of the kernels ------------------------------------------------------------------------------------------------
_PROJECT_ENTRY = {torch.bfloat16: ("tt_multivec_project", torch.bfloat16), torch.float16: ("tt_multivec_project_f16", torch.float16),
                  torch.float32: ("tt_multivec_project_f32", torch.float16)}


def _check_dim(what: str, dim: int) -> None:
    if dim <= 0 or dim % DIM_STEP or dim > MAX_DIM:
        raise NotImplementedError(f"{what}: dim={dim}: a multiple of {DIM_STEP} up to {MAX_DIM}")


def project(hidden: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, rows) -> torch.Tensor:
    """``tt_multivec_project[_f16|_f32]``, picked by ``hidden.dtype`` -> [n_out][dim]: row n = normalize(weight @ hidden[rows[n]] +
    bias), in the operands' 16-bit type -- fp16 for fp32 operands.  ``hidden`` [n_rows][H] with unit column stride, ``weight``
    [dim][H] of the same type, ``bias`` fp32 [dim]; a row number outside [0, n_rows) gives a zero row."""
    entry = _PROJECT_ENTRY.get(hidden.dtype)
    if entry is None or weight.dtype != hidden.dtype:
        raise ValueError(f"project: hidden {hidden.dtype} and weight {weight.dtype} must be one of bfloat16, float16, float32")
    if hidden.dim() != 2 or weight.dim() != 2 or hidden.shape[1] != weight.shape[1] or hidden.stride(1) != 1 \
            or not weight.is_contiguous():
        raise ValueError("project: hidden [n_rows][H] with unit column stride and weight [dim][H] are needed")
    if bias.dtype != torch.float32 or tuple(bias.shape) != (weight.shape[0],) or not bias.is_contiguous():
        raise ValueError(f"project: bias must be float32 [{weight.shape[0]}]")
    n_rows, H, ld, dim = int(hidden.shape[0]), int(hidden.shape[1]), int(hidden.stride(0)), int(weight.shape[0])
    if H <= 0 or H % 128 or H > MAX_HIDDEN:
        raise NotImplementedError(f"project: hidden size {H}: a multiple of 128 up to {MAX_HIDDEN}")
    _check_dim("project", dim)
    dev = hidden.device                                   # (the host-side refusals above need no device)
    if dev.type != "cuda" or weight.device != dev or bias.device != dev:
        raise RuntimeError("project: device tensors are needed; tensor_truth_amd has no CPU path")
    name, out_dtype = entry
    rows_t = _dev_i(rows, torch.int32, dev)
    n_out = int(rows_t.numel())
    out = torch.empty((n_out, dim), dtype=out_dtype, device=dev)
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(hidden.data_ptr(), n_rows, ld, H, weight.data_ptr(), bias.data_ptr(), dim, rows_t.data_ptr(), n_out,
                                out.data_ptr(), _stream(dev))
    _lib.check(rc, name)
    return out


def maxsim_wide(q_vecs: torch.Tensor, q_start, q_len, d_vecs: torch.Tensor, d_start, d_len, cand=None, n_cand: Optional[int] = None,
                mean: bool = False) -> torch.Tensor:
    """``tt_maxsim_wide[_f16]`` -> scores fp32 [n_q][n_cand] (device): the sum over a query's vectors of the maximum dot product with
    the document's -- its mean with ``mean``.  ``q_vecs`` [*, dim], ``d_vecs`` [*, dim]: 16-bit tensors of one type, dim a multiple
    of 128 up to 1024.  ``q_start`` / ``q_len`` (int32), ``d_start`` (int64) / ``d_len`` (int32), ``cand`` ([n_q][n_cand] int32
    document numbers, < 0 = none; None: documents 0 .. n_cand-1 for every query): host arrays are checked against the kernel's limits
    (q_len 1 .. 512, d_len 0 .. 8192, rows inside the buffers) before anything touches a device, and uploaded; device tensors are
    taken as they are -- their owner (``MultiVectorStore``, ``M3MultiVectorEncoder``) checked them when it made them, and the kernel
    clamps a length into its range."""
    return _maxsim("maxsim_wide", "tt_maxsim_wide", MAX_QUERY_LEN, MAX_DOC_LEN, _check_dim, (1 if mean else 0,), q_vecs, q_start, q_len,
                   d_vecs, d_start, d_len, cand, n_cand)


def m3_mix(dense: torch.Tensor, lex: torch.Tensor, mv: torch.Tensor, weights: Sequence[float]) -> torch.Tensor:
    """``tt_m3_mix`` -> (w_dense * dense + w_lex * lex + w_mv * mv) / (w_dense + w_lex + w_mv), fp32, the inputs' shape; -inf in any
    input gives -inf."""
    wd, wl, wm = check_m3_weights({"m3_weights": weights})
    if not (dense.dtype == lex.dtype == mv.dtype == torch.float32) or dense.shape != lex.shape or dense.shape != mv.shape \
            or not (dense.is_contiguous() and lex.is_contiguous() and mv.is_contiguous()):
        raise ValueError("m3_mix: three contiguous float32 tensors of one shape are needed")
    dev = dense.device
    if dev.type != "cuda" or lex.device != dev or mv.device != dev:
        raise RuntimeError("m3_mix: device tensors are needed; tensor_truth_amd has no CPU path")
    out = torch.empty_like(dense)
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        rc = lib.tt_m3_mix(dense.data_ptr(), lex.data_ptr(), mv.data_ptr(), dense.numel(), wd, wl, wm, out.data_ptr(), _stream(dev))
    _lib.check(rc, "tt_m3_mix")
    return out


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
class M3MultiVectorEncoder(M3Encoder):
    """One forward per batch -> the dense vector, the lexical weights AND the token vectors of every text, on the weights of an
    existing ``HipHuggingFaceEmbedding`` (an XLM-R checkpoint with CLS pooling whose directory ships ``sparse_linear.pt`` and
    ``colbert_linear.pt``), in whichever precision that embedder was built.  Nothing of the embedder is changed.  The batching is
    ``M3Encoder.encode``'s and a batch's forward ``M3Encoder._encode_batch``'s; only the projection of its hidden state is added.

    ``heads``: ((w [H], bias), (W [dim][H], b [dim])) instead of the directory's files (synthetic weights: benchmarks).  The token
    vectors are in the type of the path's hidden states -- fp16 for the reference-precision paths, whose hidden states are fp32."""

    def __init__(self, embedder, heads: Optional[Tuple[Tuple[torch.Tensor, float], Tuple[torch.Tensor, torch.Tensor]]] = None):
        cfg = getattr(embedder, "config", None)
        if cfg is None or getattr(cfg, "arch", None) != "xlmr":
            raise NotImplementedError(f"M3MultiVectorEncoder: architecture {getattr(cfg, 'arch', None)!r}: the multi-vector head belongs "
                                      "to XLM-R checkpoints (BAAI/bge-m3)")
        if embedder.pooling != "cls":
            raise NotImplementedError(f"M3MultiVectorEncoder: pooling '{embedder.pooling}': BGE-M3's dense vector is the CLS row")
        if heads is None:
            mdir = getattr(embedder, "model_dir", None)
            for have, fn, what in ((has_lexical_head, SPARSE_FILE, "lexical"), (has_multivector_head, COLBERT_FILE, "multi-vector")):
                if not have(mdir):
                    raise FileNotFoundError(f"M3MultiVectorEncoder: {embedder.model_name}: directory {mdir!r} has no {fn} (the {what} "
                                            "head)")
            heads = (load_sparse_head(mdir, cfg.hidden), load_colbert_head(mdir, cfg.hidden))
        super().__init__(embedder, head=heads[0])
        W, b = heads[1]
        if W.dim() != 2 or W.shape[1] != cfg.hidden or tuple(b.shape) != (W.shape[0],):
            raise ValueError(f"M3MultiVectorEncoder: head weight {tuple(W.shape)} / bias {tuple(b.shape)} do not match "
                             f"[dim][{cfg.hidden}] / [dim]")
        self.dim = int(W.shape[0])
        _check_dim("M3MultiVectorEncoder", self.dim)
        # the projection in the element type of the path's hidden states, the bias in fp32
        self.mv_w = W.to(device=self.device, dtype=self.path.hidden).contiguous()
        self.mv_b = b.to(device=self.device, dtype=torch.float32).contiguous()
        self.vector_dtype = _PROJECT_ENTRY[self.path.hidden][1]
        self._pieces: Optional[List[Tuple[torch.Tensor, np.ndarray]]] = None

    def parameters(self):
        yield self.w
        yield self.mv_w
        yield self.mv_b

    def _after_forward(self, hidden: torch.Tensor, batch) -> None:
        """The projection of every row but a sequence's first, on the hidden state ``M3Encoder._encode_batch`` just computed."""
        if self._pieces is None:
            return
        kept = batch.seq_len.astype(np.int64) - 1
        within = np.arange(int(kept.sum()), dtype=np.int64) - np.repeat(np.cumsum(kept) - kept, kept)
        rows = (np.repeat(batch.seq_start.astype(np.int64) + 1, kept) + within).astype(np.int32)
        self._pieces.append((project(hidden, self.mv_w, self.mv_b, rows), kept.astype(np.int32)))

    def encode(self, items, is_query: bool = False) -> Tuple[torch.Tensor, LexicalWeights, TokenVectors]:
        """``M3Encoder.encode``'s arguments -> (dense fp32 [n][H], ``LexicalWeights``, ``TokenVectors``: ``len - 1`` L2-normalised
        vectors per text, every token row but ``<s>``), original order.  A text's result does not depend on the batch it travels
        in.  A query (``is_query``) of more than 512 vectors is refused."""
        if len(items) == 0:
            raise ValueError("M3MultiVectorEncoder.encode: nothing to encode")
        seqs = self._tokens(items, is_query)
        n = len(seqs)
        lens = np.asarray([min(len(s), self.max_length) - 1 for s in seqs], dtype=np.int32)
        if is_query:
            _check_range("query vectors", lens, 0, MAX_QUERY_LEN)
        _check_range("vectors", lens, 0, MAX_DOC_LEN)
        self._pieces = []
        try:
            dense, lw = super().encode(seqs, is_query)          # (token ids pass through _tokens as they are)
            pieces = self._pieces
        finally:
            self._pieces = None
        # the batches are consecutive slices of M3Encoder.encode's order: longest first, ties in input order
        order = np.asarray(sorted(range(n), key=lambda i: -len(seqs[i])), dtype=np.int64)
        got = np.concatenate([k for _, k in pieces])
        if len(got) != n or not np.array_equal(got, lens[order]):
            raise RuntimeError("M3MultiVectorEncoder.encode: the batches do not cover the texts in the expected order")
        starts = np.zeros(n, dtype=np.int64)
        np.cumsum(lens[:-1], out=starts[1:])
        packed = pieces[0][0] if len(pieces) == 1 else torch.cat([v for v, _ in pieces])
        src_start = np.zeros(n, dtype=np.int64)             # where text order[k]'s vectors sit in `packed`
        np.cumsum(got[:-1], out=src_start[1:])
        cnt = lens.astype(np.int64)
        within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(starts, cnt)
        where = np.empty(n, dtype=np.int64)
        where[order] = src_start
        src = torch.from_numpy(np.repeat(where, cnt) + within).to(self.device)
        vectors = packed.index_select(0, src) if len(src) else packed[:0]
        return dense, lw, TokenVectors(vectors, starts, lens)


# ---- the store ----------------------------------------------------------------------------------------------------------------------
class MultiVectorStore(TokenVectorStore):
    """``TokenVectorStore`` with ``tt_maxsim_wide``'s limits: dim a multiple of 128 up to 1024, passages of up to 8192 vectors,
    queries of up to 512.  2 * dim bytes per kept token plus 12 bytes per passage -- about 369 KB for a 180-token passage at dim
    1024, some 700 k such passages in 288 GB: a rerank-stage store for a working set, not the corpus.  ``add``, ``remove``,
    ``lookup`` and ``nbytes`` are the base class's.  ``search`` raises ``NotImplementedError``: the exact MaxSim scan
    (``tt_maxsim_scan_topk``) serves dim <= 128 and passages of <= 512 vectors, so the 1024-wide head stays a rerank-stage store."""

    DIM_STEP, DIM_LIMIT, DOC_LIMIT = DIM_STEP, MAX_DIM, MAX_DOC_LEN

    def score(self, queries: TokenVectors, cand: np.ndarray, mean: bool = False) -> torch.Tensor:
        """MaxSim of every query against its row of ``cand`` (document numbers, -1 = none) -> fp32 [n_q][n_cand] (device); the mean
        over the query's vectors instead of the sum with ``mean``."""
        cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(len(queries.lens), -1)
        if cand.size and cand.max() >= self.n_docs:
            raise ValueError(f"document number {int(cand.max())} with {self.n_docs} documents stored")
        return maxsim_wide(queries.vectors, np.asarray(queries.starts).astype(np.int32), queries.lens, self.vectors,
                           self.d_start[: self.n_docs], self.d_len[: self.n_docs], cand=cand, mean=mean)


# ---- postprocessor ---------------------------------------------------------------------------------------------------------------
class HipM3AllRerank(_StoredRerank):
    """Rerank postprocessor over all three heads of BGE-M3, with the surface of ``HipM3HybridRerank``: ``postprocess_nodes`` (keyword
    or positional), ``rerank``, ``predict``, ``.model`` (with ``.parameters()``), ``index_nodes``, ``remove_node``, ``stats``.
    ``index_nodes`` encodes nodes' EMBED-mode content once into the instance's ``LexicalStore`` and ``MultiVectorStore``.  At query
    time one forward gives the query's dense vector, lexical weights and token vectors; a stored node is scored from the stores
    and any other node is encoded in the call -- both give the same bits for the same text.  The node score is

        (w_dense * <q, d> + w_lex * lex(q, d) + w_mv * mv(q, d)) / (w_dense + w_lex + w_mv)

    with ``dense`` and ``lex`` as ``HipM3HybridRerank`` computes them, ``mv`` the mean over the query's vectors of the maximum dot
    product with the passage's (``tt_maxsim_wide``, mean = 1, at every dim), mixed by ``tt_m3_mix``.
    ``model_kwargs["m3_weights"] = (w_dense, w_lex, w_mv)`` is required and never defaulted.

    ``model_kwargs["embedder"]``: an existing ``HipHuggingFaceEmbedding`` to share (its weights are not loaded a second time)."""

    def __init__(self, model: str = "BAAI/bge-m3", top_n: int = 2, device: Optional[str] = None, keep_retrieval_score: bool = False,
                 model_kwargs: Optional[Dict[str, Any]] = None, **_ignored):
        mk = dict(model_kwargs or {})
        self.m3_weights = check_m3_weights(mk)
        mk.pop("m3_weights")
        embedder = mk.pop("embedder", None)
        heads = mk.pop("m3_heads", None)
        if embedder is None:
            from .embedding import HipHuggingFaceEmbedding

            embedder = HipHuggingFaceEmbedding(model_name=model, device=device, model_kwargs=mk)
        self.model_name, self.top_n, self.keep_retrieval_score = model, top_n, keep_retrieval_score
        self.embedder, self.device, self.config = embedder, embedder.device, embedder.config
        self.encoder = M3MultiVectorEncoder(embedder, heads=heads)
        self.model = _M3Model(embedder, self.encoder)
        self.store = LexicalStore(self.config.hidden, self.device)
        self.vectors = MultiVectorStore(self.encoder.dim, self.encoder.vector_dtype, self.device)
        self.precision = embedder.precision
        self.nodes: Dict[Any, Any] = {}
        self.stats = {"queries": 0, "stored": 0, "encoded": 0}

    def remove_node(self, node_id: Any) -> bool:
        self.nodes.pop(node_id, None)
        self.vectors.remove(node_id)
        return self.store.remove(node_id)

    # ---- what _StoredRerank asks for --------------------------------------------------------------------------------
    def encode_queries(self, texts):
        return self.encoder.encode(texts, is_query=True)

    def encode_documents(self, texts):
        return self.encoder.encode(texts, is_query=False)

    def add_documents(self, nodes, encoded) -> None:
        dense, lw, tv = encoded
        ids = [n.id_ for n in nodes]
        self.store.add(ids, lw, dense)
        self.vectors.add(ids, tv.vectors, tv.lens)
        self.nodes.update((n.id_, n) for n in nodes)

    def lookup(self, ids) -> np.ndarray:
        return np.stack((self.store.lookup(ids), self.vectors.lookup(ids)))

    def _mix(self, lex: torch.Tensor, dense: torch.Tensor, mv: torch.Tensor) -> np.ndarray:
        return m3_mix(dense, lex, mv, self.m3_weights).cpu().numpy()

    _HW = (1.0, 1.0)          # (tt_lexical_score's own mix is not read: its lex and dense outputs are)

    def score_stored(self, q, cands) -> np.ndarray:
        q_dense, q_lw, q_tv = q
        lex, dense, _ = self.store.score(q_lw, cands[0], dense=q_dense, hybrid_weights=self._HW)
        return self._mix(lex, dense, self.vectors.score(q_tv, cands[1], mean=True))

    def score_fresh(self, q, d, cand) -> np.ndarray:
        (q_dense, q_lw, q_tv), (d_dense, d_lw, d_tv) = q, d
        _check_range("d_nnz", d_lw.nnz, 0, MAX_DOC_NNZ)
        lex, dense, _ = lexical_score(q_lw.terms, q_lw.weights, LexicalStore._check_query(q_lw), q_lw.nnz, d_lw.terms, d_lw.weights,
                                      d_lw.starts, d_lw.nnz, cand=cand, q_dense=q_dense.to(torch.bfloat16),
                                      d_dense=d_dense.to(torch.bfloat16), hybrid_weights=self._HW)
        mv = maxsim_wide(q_tv.vectors, np.asarray(q_tv.starts).astype(np.int32), q_tv.lens, d_tv.vectors, d_tv.starts, d_tv.lens,
                         cand=cand, mean=True)
        return self._mix(lex, dense, mv)
