"""Learned sparse retrieval with SPLADE checkpoints on the HIP path: ``naver/splade-cocondenser-ensembledistil``,
``naver/splade-v3``, ``prithivida/Splade_PP_en_v1`` and the ``SparseEncoder`` checkpoints of sentence-transformers 5.

A SPLADE model is a ``BertForMaskedLM``.  A text's weight for vocabulary id v is ``max_t log1p(relu(logit[t][v]))`` over ALL of its
tokens, ``[CLS]`` and ``[SEP]`` included, with ``logit = decoder(LayerNorm(gelu(dense(h)))) + bias`` -- so a text activates terms it
does not contain (expansion), which BGE-M3's one-weight-per-token head (``lexical.py``) cannot do by construction.  The encoder is the
BERT forward of the 16-bit path; the head's ``dense -> GELU -> LayerNorm`` runs on ``tt_gemm_*`` (epilogue 1) and ``tt_layernorm_*``;
the vocabulary projection and the maximum over a text's rows are ONE kernel (``tt_splade_pool``: the [tokens][vocabulary] logits,
61 KB per token for BERT-base, are never written), and ``tt_sparse_compact`` turns a weight row into ascending (id, weight) pairs.
Everything behind that is the lexical path's: ``LexicalWeights``, the CSR store, ``tt_lexical_score``, ``tt_lexical_scan_topk``.
bf16 (default) or fp16.

[UPSTREAM-K] The tensor names of ``BertForMaskedLM`` are pinned against the installed class by tests/golden/make_splade_golden.py.
The sentence-transformers layout (``modules.json`` = ``MLMTransformer`` + ``SpladePooling``; ``1_SpladePooling/config.json`` with
``pooling_strategy``, ``activation_function``, ``word_embedding_dimension``; ``SpladePooling.forward``: ``max`` over the tokens of
``log1p(relu(logits))`` times the attention mask) is written from knowledge of sentence-transformers 5, which is not installed here
and cannot be checked offline.  The loader is therefore strict: a tensor, a module or a setting it does not know is refused by name.
"""
from __future__ import annotations

import functools
import json
import os
import re
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._hostargs import _dev_i, _need_device, _stream, _suffix, read_json, resolve_device
from ._hostargs import resolve_dtype as _resolve_dtype
from ._stored import top_nodes
from .colbert import bert_state_names
from .encoder import Encoder, EncoderConfig, EncoderWeights, pack_tokens
from .lexical import MAX_DOC_NNZ, MAX_QUERY_NNZ, MAX_SCAN_K, LexicalStore, LexicalWeights

# the kernels' limits (include/tt_hip.h)
MAX_HIDDEN, MAX_VOCAB, MAX_SEQ_LEN, MAX_SEQS, MAX_TERMS = 1024, 65536, 8192, 65535, 8192
VOCAB_TILE = 128
HEAD = "cls.predictions."
HEAD_NAMES = [HEAD + n for n in ("transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight",
                                 "transform.LayerNorm.bias", "bias")]
# tolerated and unused: BertModel's pooler, the next-sentence head, the position_ids buffer older transformers wrote
_NOT_READ = re.compile(r"^(bert\.)?(pooler\.|embeddings\.position_ids$)|^cls\.seq_relationship\.")
# [UPSTREAM-K] sentence-transformers files of a SparseEncoder directory
_POOLING_READ = frozenset(("pooling_strategy", "activation_function", "word_embedding_dimension"))
_POOLING_UNUSED = frozenset(("chunk_size",))          # how upstream slices its own max over a long batch: no effect on a value
_ST_CONFIG_UNUSED = frozenset(("__version__", "prompts", "default_prompt_name", "model_type"))
_SBERT_READ = frozenset(("max_seq_length", "do_lower_case"))


# ---- checkpoint --------------------------------------------------------------------------------------------------------------------
def detect_layout(model_dir: Optional[str]) -> Optional[str]:
    """"sparse_encoder" for a directory whose ``modules.json`` names a SpladePooling module, "hf" for a plain Hugging Face directory
    whose ``config.json`` names a masked-language-model architecture, else None."""
    if not model_dir or not os.path.isdir(model_dir):
        return None
    mj = os.path.join(model_dir, "modules.json")
    if os.path.exists(mj):
        try:
            with open(mj, encoding="utf-8") as f:
                kinds = [str(m.get("type", "")).rsplit(".", 1)[-1] for m in json.load(f)]
        except (OSError, ValueError, AttributeError):
            return None
        return "sparse_encoder" if "SpladePooling" in kinds else None
    try:
        archs = read_json(os.path.join(model_dir, "config.json")).get("architectures") or []
    except (OSError, ValueError):
        return None
    return "hf" if any(str(a).endswith("ForMaskedLM") for a in archs) else None


resolve_dtype = functools.partial(_resolve_dtype, family="SPLADE")


def check_pooling(model_dir: str) -> Tuple[Optional[int], Optional[int]]:
    """The sentence-transformers files of a SparseEncoder directory -> (``max_seq_length``, ``word_embedding_dimension``; None: not
    given), after refusing a module
    list, a pooling strategy, an activation or a field this path does not compute."""
    with open(os.path.join(model_dir, "modules.json"), encoding="utf-8") as f:
        mods = json.load(f)
    kinds = [str(m.get("type", "")).rsplit(".", 1)[-1] for m in mods]
    if kinds != ["MLMTransformer", "SpladePooling"]:
        raise NotImplementedError(f"modules.json names {kinds}: a SPLADE SparseEncoder is an MLMTransformer and one SpladePooling "
                                  "(inference-free 'doc-only' query encoders -- SparseStaticEmbedding / Router -- are not supported)")
    if mods[0].get("path", "") not in ("", "."):
        raise NotImplementedError(f"modules.json: MLMTransformer module at path {mods[0].get('path')!r} (expected the directory itself)")
    where = os.path.join(str(mods[1].get("path", "1_SpladePooling")), "config.json")
    pc = read_json(os.path.join(model_dir, where))
    unknown = sorted(set(pc) - _POOLING_READ - _POOLING_UNUSED)
    if unknown:
        raise NotImplementedError(f"{where} carries fields the SPLADE path does not know: {unknown[:6]}")
    for key in ("pooling_strategy", "activation_function"):
        if key not in pc:
            raise ValueError(f"{where} has no '{key}' (it is never defaulted)")
    if pc["pooling_strategy"] != "max":
        raise NotImplementedError(f"{where} pooling_strategy={pc['pooling_strategy']!r}: only 'max' is computed (sum pooling is not "
                                  "supported)")
    if pc["activation_function"] != "relu":
        raise NotImplementedError(f"{where} activation_function={pc['activation_function']!r}: only 'relu' -- log1p(relu(x)) -- is "
                                  "computed ('log1p_relu', log1p(log1p(relu(x))), is a different function)")
    p = os.path.join(model_dir, "config_sentence_transformers.json")
    if os.path.exists(p):
        sc = read_json(p)
        unknown = sorted(set(sc) - _ST_CONFIG_UNUSED - {"similarity_fn_name"})
        if unknown:
            raise NotImplementedError(f"config_sentence_transformers.json carries fields the SPLADE path does not know: {unknown[:6]}")
        fn = sc.get("similarity_fn_name")
        if fn is not None and str(fn).lower() != "dot":
            raise NotImplementedError(f"config_sentence_transformers.json similarity_fn_name={fn!r}: only 'dot' is computed")
    max_seq = None
    p = os.path.join(model_dir, "sentence_bert_config.json")
    if os.path.exists(p):
        sb = read_json(p)
        unknown = sorted(set(sb) - _SBERT_READ)
        if unknown:
            raise NotImplementedError(f"sentence_bert_config.json carries fields the SPLADE path does not know: {unknown[:6]}")
        if sb.get("max_seq_length") is not None:
            max_seq = int(sb["max_seq_length"])
            if max_seq < 2:
                raise ValueError(f"sentence_bert_config.json max_seq_length={max_seq}")
    dim = pc.get("word_embedding_dimension")
    return max_seq, (None if dim is None else int(dim))


def check_state(cfg: EncoderConfig, state: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """A ``BertForMaskedLM`` state dict (the body optionally under ``bert.``) -> (the BERT tensors under BertModel's names, the head:
    ``dense.weight`` [H][H], ``dense.bias``, ``LayerNorm.weight``, ``LayerNorm.bias``, ``decoder.weight`` [V][H] -- the file's
    ``cls.predictions.decoder.weight`` if it carries one, else the word embeddings (tied) -- and ``bias`` [V]).  Anything else is
    refused by name."""
    missing = [n for n in HEAD_NAMES if n not in state]
    if missing:
        raise ValueError(f"checkpoint has no {missing[:3]}: not a masked-language-model (SPLADE) checkpoint")
    sd, head_extra = {}, {}
    for k, v in state.items():
        if k in HEAD_NAMES or _NOT_READ.search(k):
            continue
        if k.startswith(HEAD):
            head_extra[k[len(HEAD):]] = v
        else:
            sd[k[len("bert."):] if k.startswith("bert.") else k] = v
    unknown = sorted(set(head_extra) - {"decoder.weight", "decoder.bias"})
    if unknown:
        raise NotImplementedError(f"checkpoint carries tensors the SPLADE path does not compute: {[HEAD + u for u in unknown[:4]]}")
    names = bert_state_names(cfg)
    lost = [n for n in names if n not in sd]
    if lost:
        raise ValueError(f"checkpoint is not a BERT of {cfg}: missing {lost[:4]}")
    extra = sorted(set(sd) - set(names))
    if extra:
        raise NotImplementedError(f"checkpoint carries tensors the SPLADE path does not compute: {extra[:4]}")
    H, V = cfg.hidden, cfg.vocab_size
    bias = state[HEAD + "bias"]
    if "decoder.bias" in head_extra and not torch.equal(head_extra["decoder.bias"].to(torch.float32), bias.to(torch.float32)):
        raise NotImplementedError(f"{HEAD}decoder.bias differs from {HEAD}bias: BertForMaskedLM ties them, and which one a checkpoint "
                                  "that does not means is not known")
    dec = head_extra.get("decoder.weight", sd["embeddings.word_embeddings.weight"])
    head = {"dense.weight": state[HEAD + "transform.dense.weight"], "dense.bias": state[HEAD + "transform.dense.bias"],
            "LayerNorm.weight": state[HEAD + "transform.LayerNorm.weight"], "LayerNorm.bias": state[HEAD + "transform.LayerNorm.bias"],
            "decoder.weight": dec, "bias": bias}
    want = {"dense.weight": (H, H), "dense.bias": (H,), "LayerNorm.weight": (H,), "LayerNorm.bias": (H,), "decoder.weight": (V, H),
            "bias": (V,)}
    for k, shape in want.items():
        if tuple(head[k].shape) != shape:
            raise ValueError(f"{HEAD}{k if k != 'bias' else 'bias'} {tuple(head[k].shape)} does not match {shape}")
    return {n: sd[n] for n in names}, head


def load_checkpoint(model_dir: str, model_kwargs: Optional[dict] = None):
    """A SPLADE directory of either layout -> (EncoderConfig, BERT state dict, head tensors, tokenizer, max_seq_length or None).
    Host work only."""
    from . import weights as _weights
    from .tokenization import load_tokenizer

    resolve_dtype(model_kwargs)
    layout = detect_layout(model_dir)
    if layout is None and os.path.exists(os.path.join(model_dir or "", "modules.json")):
        check_pooling(model_dir)          # (names the module list it refuses)
    hf = read_json(os.path.join(model_dir, "config.json"))
    mt = hf.get("model_type")
    if mt == "distilbert":
        raise NotImplementedError("config.json model_type='distilbert': DistilBERT SPLADE variants (vocab_transform / vocab_projector) "
                                  "are not supported")
    if mt != "bert" or hf.get("position_embedding_type", "absolute") != "absolute":
        raise NotImplementedError(f"config.json model_type={mt!r} position_embedding_type={hf.get('position_embedding_type')!r}: the "
                                  "SPLADE path serves BERT backbones with absolute positions")
    if str(hf.get("hidden_act", "gelu")) != "gelu":
        raise NotImplementedError(f"config.json hidden_act={hf.get('hidden_act')!r}: the encoder and the head's transform compute 'gelu'")
    cfg = _weights._config_from_hf(hf, 0)
    cfg = EncoderConfig(**{**cfg.__dict__, "num_labels": 0})
    if cfg.vocab_size > MAX_VOCAB:
        raise NotImplementedError(f"config.json vocab_size={cfg.vocab_size}: up to {MAX_VOCAB} (multilingual SPLADE variants are not "
                                  "supported)")
    if cfg.hidden % 128 or cfg.hidden > MAX_HIDDEN:
        raise NotImplementedError(f"config.json hidden_size={cfg.hidden}: a multiple of 128 up to {MAX_HIDDEN}")
    max_seq = None
    if layout == "sparse_encoder":
        max_seq, dim = check_pooling(model_dir)
        if dim is not None and dim != cfg.vocab_size:
            raise ValueError(f"1_SpladePooling word_embedding_dimension={dim} does not match vocab_size={cfg.vocab_size}")
    bert, head = check_state(cfg, _weights.load_state(model_dir))
    tk = (model_kwargs or {}).get("tokenizer") or load_tokenizer(model_dir, "bert", cfg.vocab_size)
    return cfg, bert, head, tk, max_seq


# ---- host wrappers of the kernels ------------------------------------------------------------------------------------------------
def splade_pool(t: torch.Tensor, E: torch.Tensor, bias: torch.Tensor, seq_start, seq_len, max_len: Optional[int] = None,
                activation: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``tt_splade_pool[_f16]``, picked by ``t.dtype`` -> fp32 [n_seq][Vp] on the device (``out``: a tensor [n_seq][>= Vp] to write
    into): column v of sequence b is ``act(max over the sequence's rows of <t[r], E[v]> + bias[v])``, ``activation`` 1:
    ``log1p(relu(.))``, 0: the identity.  ``t`` [n_rows][H] (unit column stride) holds the transformed hidden states, ``E`` [Vp][H]
    the decoder matrix in the same type, ``bias`` fp32 [Vp].  Host ``seq_start`` / ``seq_len`` are uploaded as they are (the kernel
    cuts a sequence at ``n_rows`` and gives one with a negative start no rows); ``max_len`` defaults to the largest length."""
    sfx = _suffix(t.dtype)
    if E.dtype != t.dtype or t.dim() != 2 or E.dim() != 2 or E.shape[1] != t.shape[1] or t.stride(1) != 1 or not E.is_contiguous():
        raise ValueError("splade_pool: t [n_rows][H] with unit column stride and a contiguous E [Vp][H] of one 16-bit type are needed")
    if bias.dtype != torch.float32 or bias.dim() != 1 or bias.shape[0] != E.shape[0] or not bias.is_contiguous():
        raise ValueError("splade_pool: bias float32 [Vp] is needed")
    n_rows, H, ld, Vp = int(t.shape[0]), int(t.shape[1]), int(t.stride(0)), int(E.shape[0])
    n_seq = len(seq_len)
    if max_len is None:
        max_len = max(1, int(np.max(seq_len))) if n_seq and not isinstance(seq_len, torch.Tensor) else 1
    dev = _need_device("splade_pool", t, E, bias)
    st, sl = _dev_i(seq_start, torch.int32, dev), _dev_i(seq_len, torch.int32, dev)
    if out is None:
        out = torch.empty((n_seq, Vp), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != n_seq or out.stride(1) != 1 or out.device != dev:
        raise ValueError("splade_pool: out float32 [n_seq][>= Vp] on the device is needed")
    lib = _lib.load_library()
    name = "tt_splade_pool" + sfx
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(t.data_ptr(), n_rows, ld, H, E.data_ptr(), bias.data_ptr(), Vp, st.data_ptr(), sl.data_ptr(), n_seq,
                                int(max_len), int(activation), out.data_ptr(), int(out.stride(0)) if n_seq else Vp, _stream(dev))
    _lib.check(rc, name)
    return out


def sparse_compact(w: torch.Tensor, V: int, max_terms: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``tt_sparse_compact`` -> (terms int32 [n][max_terms], weights fp32 [n][max_terms], nnz int32 [n]) on the device: row b's ids
    < ``V`` with a weight > 0 -- the ``max_terms`` largest by (weight descending, id ascending) if there are more -- in ascending
    order, then (-1, 0)."""
    if w.dtype != torch.float32 or w.dim() != 2 or w.stride(1) != 1:
        raise ValueError("sparse_compact: w float32 [n][>= V] with unit column stride is needed")
    dev = _need_device("sparse_compact", w)
    n = int(w.shape[0])
    terms = torch.empty((n, int(max_terms)), dtype=torch.int32, device=dev)
    weights = torch.empty((n, int(max_terms)), dtype=torch.float32, device=dev)
    nnz = torch.empty((n,), dtype=torch.int32, device=dev)
    if int(V) > w.shape[1]:
        raise ValueError(f"sparse_compact: V={V} with rows of {w.shape[1]}")
    lib = _lib.load_library()
    with torch.cuda.device(dev):
        rc = lib.tt_sparse_compact(w.data_ptr(), int(w.stride(0)) if n else int(V), int(V), n, int(max_terms), terms.data_ptr(),
                                   weights.data_ptr(), nnz.data_ptr(), _stream(dev))
    _lib.check(rc, "tt_sparse_compact")
    return terms, weights, nnz


# ---- weights and encoder ----------------------------------------------------------------------------------------------------------
def pad_vocabulary(decoder: torch.Tensor, bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(decoder [V][H], bias [V]) -> ([Vp][H], [Vp]) with zero rows up to the next multiple of 128 (``tt_splade_pool``'s tile): a
    padding id scores log1p(relu(0 + 0)) = 0, which is never kept, and ``tt_sparse_compact`` does not read ids >= V at all."""
    V, H = decoder.shape
    Vp = (V + VOCAB_TILE - 1) // VOCAB_TILE * VOCAB_TILE
    E = torch.zeros((Vp, H), dtype=decoder.dtype)
    E[:V] = decoder
    b = torch.zeros((Vp,), dtype=torch.float32)
    b[:V] = bias.to(torch.float32)
    return E, b


class SpladeWeights:
    """Device-resident weights of a SPLADE checkpoint: the BERT encoder in the layout of ``tt_encoder_weights`` (bf16 or fp16), the
    head's transform, and the decoder matrix [Vp][H] with its bias [Vp], zero-padded from ``vocab_size`` to a multiple of 128 (a
    padding id scores log1p(relu(0)) = 0 and is never kept)."""

    def __init__(self, cfg: EncoderConfig, bert_state: Dict[str, torch.Tensor], head: Dict[str, torch.Tensor], device: torch.device,
                 dtype: torch.dtype = torch.bfloat16):
        if cfg.arch != "bert" or cfg.num_labels:
            raise ValueError(f"SpladeWeights: a BERT backbone without a classification head is needed, not {cfg}")
        _suffix(dtype)
        H, V = cfg.hidden, cfg.vocab_size
        if H % 128 or H > MAX_HIDDEN or not 1 <= V <= MAX_VOCAB:
            raise NotImplementedError(f"SpladeWeights: hidden {H} (a multiple of 128 up to {MAX_HIDDEN}), vocabulary {V} (up to {MAX_VOCAB})")
        self.encoder = EncoderWeights(cfg, bert_state, device, dtype)
        self.cfg, self.device, self.dtype = cfg, device, dtype
        self.vocab = V
        self.vocab_padded = (V + VOCAB_TILE - 1) // VOCAB_TILE * VOCAB_TILE
        f32 = dict(device=device, dtype=torch.float32)
        self.dense_w = head["dense.weight"].to(device=device, dtype=dtype).contiguous()
        self.dense_b = head["dense.bias"].to(**f32).contiguous()
        self.ln_w = head["LayerNorm.weight"].to(**f32).contiguous()
        self.ln_b = head["LayerNorm.bias"].to(**f32).contiguous()
        E, b = pad_vocabulary(head["decoder.weight"].to(dtype), head["bias"])
        self.decoder, self.bias = E.to(device).contiguous(), b.to(device).contiguous()

    def parameters(self) -> Iterable[torch.Tensor]:
        """For ModelManager-style memory accounting."""
        yield from self.encoder.parameters()
        yield from (self.dense_w, self.dense_b, self.ln_w, self.ln_b, self.decoder, self.bias)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.parameters())


class SpladeEncoder:
    """Texts (or token-id sequences that carry their special tokens) -> ``LexicalWeights``."""

    def __init__(self, weights: SpladeWeights, tokenizer, max_length: Optional[int] = None, embed_batch_size: int = 128,
                 forward_tokens: int = 131072):
        self.w, self.tokenizer = weights, tokenizer
        self.cfg, self.device = weights.cfg, weights.device
        self._enc = Encoder(weights.encoder)
        self.max_length = min(max_length or self.cfg.max_seq_len, self.cfg.max_seq_len, MAX_SEQ_LEN)
        self.embed_batch_size, self.forward_tokens = int(embed_batch_size), int(forward_tokens)
        sfx = _suffix(weights.dtype)
        self._gemm, self._ln = ("tt_gemm_f16", "tt_layernorm_f16") if sfx else ("tt_gemm_bf16", "tt_layernorm_bf16")

    def _tokens(self, items) -> List[Sequence[int]]:
        texts = [x for x in items if isinstance(x, str)]
        if len(texts) == len(items):
            tk = self.tokenizer
            if hasattr(tk, "encode_batch"):
                return tk.encode_batch(texts, self.max_length)
            return [tk.encode(t, self.max_length) for t in texts]
        if texts:
            raise ValueError("SpladeEncoder.encode: either strings or token-id sequences, not both")
        return list(items)

    def transform(self, hidden: torch.Tensor) -> torch.Tensor:
        """The head's ``LayerNorm(gelu(dense(h)))`` of every row of ``hidden`` [n_rows][H] (n_rows as the forward pads them)."""
        w, dev, H = self.w, self.device, self.cfg.hidden
        n_rows = int(hidden.shape[0])
        lib = self._enc.lib
        g = torch.empty_like(hidden)
        t = torch.empty_like(hidden)
        with torch.cuda.device(dev):
            rc = getattr(lib, self._gemm)(hidden.data_ptr(), w.dense_w.data_ptr(), w.dense_b.data_ptr(), None, g.data_ptr(), n_rows, H,
                                          H, 1, _stream(dev))
            _lib.check(rc, self._gemm)
            rc = getattr(lib, self._ln)(g.data_ptr(), t.data_ptr(), w.ln_w.data_ptr(), w.ln_b.data_ptr(), n_rows, H,
                                        float(self.cfg.ln_eps), _stream(dev))
            _lib.check(rc, self._ln)
        return t

    def weights_packed(self, seqs: List[Sequence[int]], activation: int = 1) -> torch.Tensor:
        """One forward over ``seqs`` -> their dense weight rows, fp32 [len(seqs)][Vp] on the device (ids >= vocab_size weigh 0)."""
        enc = self._enc
        batch = enc._padded(pack_tokens(seqs, self.cfg, None, self.max_length))
        if len(batch.seq_len) > MAX_SEQS:
            raise ValueError(f"{len(batch.seq_len)} sequences in one forward (up to {MAX_SEQS})")
        hidden, starts, lens = enc.forward_packed(batch, want_lens=True)
        return splade_pool(self.transform(hidden), self.w.decoder, self.w.bias, starts, lens, max_len=batch.max_len, activation=activation)

    def encode(self, items, is_query: bool = False, max_terms: Optional[int] = None) -> LexicalWeights:
        """``items``: strings, or token-id sequences that already carry ``[CLS]`` and ``[SEP]`` -> ``LexicalWeights``, original order.
        Every row of a sequence takes part in the maximum, ``[CLS]`` and ``[SEP]`` included, as upstream's attention-mask product
        has it.  ``max_terms`` (sentence-transformers' ``max_active_dims``): a text keeps its largest weights, at most this many --
        default 512 for queries and 8192 for passages, the store's own limits.  Batches are formed as ``M3Encoder.encode`` forms
        them; a text's result does not depend on the batch it travels in."""
        if len(items) == 0:
            raise ValueError("SpladeEncoder.encode: nothing to encode")
        limit = MAX_QUERY_NNZ if is_query else MAX_DOC_NNZ
        max_terms = limit if max_terms is None else int(max_terms)
        if not 1 <= max_terms <= limit:
            raise ValueError(f"max_terms={max_terms} is outside 1 .. {limit} ({'queries' if is_query else 'passages'})")
        max_terms = min(max_terms, self.w.vocab)
        seqs = self._tokens(items)
        n = len(seqs)
        order = sorted(range(n), key=lambda i: -len(seqs[i]))
        nnz = np.zeros(n, dtype=np.int32)
        pieces: List[Tuple[torch.Tensor, torch.Tensor, np.ndarray]] = []   # (terms [b][max_terms], weights, texts)
        lo = 0
        while lo < n:
            hi, tokens = lo, 0
            while hi < n and (hi - lo < self.embed_batch_size or tokens < self.forward_tokens):
                tokens += min(len(seqs[order[hi]]), self.max_length)
                hi += 1
            sel = np.asarray(order[lo:hi], dtype=np.int64)
            t, w, cnt = sparse_compact(self.weights_packed([seqs[i] for i in sel]), self.w.vocab, max_terms)
            nnz[sel] = cnt.cpu().numpy()
            pieces.append((t, w, sel))
            lo = hi
        starts = np.zeros(n, dtype=np.int64)
        np.cumsum(nnz[:-1], out=starts[1:])
        total = int(nnz.sum())
        terms = torch.empty((total,), dtype=torch.int32, device=self.device)
        weights = torch.empty((total,), dtype=torch.float32, device=self.device)
        for t, w, sel in pieces:      # one gather per batch: slot j of the batch's row i -> starts[text] + j
            cnt = nnz[sel].astype(np.int64)
            if int(cnt.sum()) == 0:
                continue
            within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            src = torch.from_numpy(np.repeat(np.arange(len(sel), dtype=np.int64) * max_terms, cnt) + within).to(self.device)
            dst = torch.from_numpy(np.repeat(starts[sel], cnt) + within).to(self.device)
            terms[dst] = t.reshape(-1)[src]
            weights[dst] = w.reshape(-1)[src]
        return LexicalWeights(terms, weights, starts, nnz)


# ---- the store ----------------------------------------------------------------------------------------------------------------------
class SpladeStore(LexicalStore):
    """Sparse vectors of indexed passages, in HBM on one device: a ``LexicalStore`` WITHOUT dense rows (``d_start`` int64, ``d_nnz``
    int32 per document; ``terms`` int32 and ``weights`` fp32 per kept id: 8 bytes).  ``add(node_ids, lexical)``, ``remove``, the
    tombstones, ``search`` and the posting lists (``postings=True`` with ``vocab_size``) are ``LexicalStore``'s; ``score`` returns
    the lexical scores alone.  No persistence."""

    def __init__(self, device: torch.device, capacity_terms: int = 1 << 16, capacity_docs: int = 1 << 10, postings: bool = False,
                 vocab_size: Optional[int] = None):
        super().__init__(0, device, capacity_terms, capacity_docs, postings, vocab_size)

    def score(self, lexical: LexicalWeights, cand) -> torch.Tensor:   # noqa: D102 (no dense part here)
        """Every query against its row of ``cand`` (document numbers, -1 = none) -> fp32 [n_q][n_cand] on the device.  A removed
        document scores -inf."""
        return super().score(lexical, cand)[0]


# ---- retriever ----------------------------------------------------------------------------------------------------------------------
class HipSpladeRetriever:
    """Exact learned-sparse retrieval: ``index_nodes`` encodes nodes' EMBED-mode content once into the instance's ``SpladeStore``;
    ``retrieve(query)`` encodes the query (one short forward), runs the exact top-k over every stored passage and returns the best
    ``similarity_top_k`` nodes by ``sum over shared ids of q_w * d_w``, best first.  Hits with score <= 0 are dropped.

    ``model_kwargs``: ``torch_dtype`` (bfloat16, the default, or float16), ``model_dir``, ``max_length``, ``query_max_terms`` /
    ``document_max_terms`` (sentence-transformers' ``max_active_dims``; default 512 / 8192), ``embed_batch_size``,
    ``forward_tokens``, ``postings`` (True: the store searches through posting lists; the same results); ``state_dict`` or ``synthetic_seed`` with ``encoder_config`` (and optionally ``tokenizer``) instead of a
    directory."""

    def __init__(self, model: str, similarity_top_k: int = 10, device: Optional[str] = None,
                 model_kwargs: Optional[Dict[str, Any]] = None, **_ignored):
        from . import weights as _weights
        from .tokenization import load_tokenizer

        if not 1 <= int(similarity_top_k) <= MAX_SCAN_K:
            raise ValueError(f"similarity_top_k={similarity_top_k} (1 .. {MAX_SCAN_K})")
        mk = dict(model_kwargs or {})
        dtype = resolve_dtype(mk)
        dev = resolve_device(device)
        self.model_name, self.similarity_top_k, self.device = model, int(similarity_top_k), dev
        max_seq = None
        if "state_dict" in mk or ("synthetic_seed" in mk and _weights.find_model_dir(model, mk) is None):
            cfg = mk.get("encoder_config")
            if cfg is None:
                raise ValueError(f"no architecture known for '{model}': pass model_kwargs['encoder_config']")
            state = mk["state_dict"] if "state_dict" in mk else synthetic_state(cfg, int(mk["synthetic_seed"]))
            bert, head = check_state(cfg, state)
            tk = mk.get("tokenizer") or load_tokenizer(None, "bert", cfg.vocab_size)
        else:
            mdir = _weights.find_model_dir(model, mk)
            if mdir is None:
                raise FileNotFoundError(f"weights for '{model}' not found: no checkpoint directory under model_kwargs['model_dir'], "
                                        "$TT_AMD_MODEL_DIR or the HF cache, and this environment has no network")
            cfg, bert, head, tk, max_seq = load_checkpoint(mdir, mk)
        self.config = cfg
        self.model = SpladeWeights(cfg, bert, head, dev, dtype)
        self.encoder = SpladeEncoder(self.model, tk, max_length=mk.get("max_length") or max_seq,
                                     embed_batch_size=int(mk.get("embed_batch_size", 128)),
                                     forward_tokens=int(mk.get("forward_tokens", 131072)))
        self.query_max_terms = mk.get("query_max_terms")
        self.document_max_terms = mk.get("document_max_terms")
        # model_kwargs["postings"]: search through posting lists (built at the first query after an ingest that left none)
        self.store = SpladeStore(dev, postings=bool(mk.get("postings", False)), vocab_size=cfg.vocab_size)
        self.precision = "fp16 (fp32 accumulate)" if dtype == torch.float16 else "bf16 (fp32 accumulate)"
        self.nodes: Dict[Any, Any] = {}
        self.stats = {"queries": 0, "indexed": 0}

    def index_nodes(self, nodes) -> int:
        """Encode the nodes' EMBED-mode content into the store (a ``NodeWithScore`` or a bare node) -> how many were added."""
        from .schema import MetadataMode

        bare = [getattr(n, "node", n) for n in nodes]
        if not bare:
            return 0
        lw = self.encoder.encode([n.get_content(metadata_mode=MetadataMode.EMBED) for n in bare], is_query=False,
                                 max_terms=self.document_max_terms)
        self.store.add([n.id_ for n in bare], lw)
        for n in bare:
            self.nodes[n.id_] = n
        self.stats["indexed"] += len(bare)
        return len(bare)

    def remove_node(self, node_id: Any) -> bool:
        self.nodes.pop(node_id, None)
        return self.store.remove(node_id)

    def retrieve(self, query):
        from .schema import NodeWithScore, as_query_bundle

        return self._retrieve(as_query_bundle(query), NodeWithScore)

    def _retrieve(self, query_bundle, node_type=None):
        if node_type is None:
            from .schema import NodeWithScore as node_type
        if self.store.n_docs == 0:
            return []
        lw = self.encoder.encode([query_bundle.query_str], is_query=True, max_terms=self.query_max_terms)
        hits = top_nodes(self.store, lw, self.similarity_top_k, self.nodes, node_type)
        self.stats["queries"] += 1
        return hits


def synthetic_state(cfg: EncoderConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded random weights of a SPLADE of ``cfg`` (benchmarks): the encoder's synthetic BERT plus a tied masked-language-model head
    whose bias (4.5 standard deviations of a logit below zero) keeps a text's active ids to a small share of the vocabulary."""
    from .encoder import synthetic_state as bert_state

    sd = dict(bert_state(cfg, seed))
    g = torch.Generator().manual_seed(seed + 1)
    H = cfg.hidden
    sd[HEAD + "transform.dense.weight"] = torch.randn(H, H, generator=g) * 0.02
    sd[HEAD + "transform.dense.bias"] = torch.zeros(H)
    sd[HEAD + "transform.LayerNorm.weight"] = torch.ones(H)
    sd[HEAD + "transform.LayerNorm.bias"] = torch.zeros(H)
    emb = next(v for k, v in sd.items() if k.endswith("embeddings.word_embeddings.weight"))
    scale = float(emb.float().norm(dim=1).mean())
    # after the head's LayerNorm a row has norm sqrt(H): a logit is ~ N(0, (sqrt(H) std)^2) = N(0, scale^2)
    sd[HEAD + "bias"] = torch.full((cfg.vocab_size,), -4.5 * scale)
    return sd


# the published geometry of naver/splade-cocondenser-ensembledistil (bert-base-uncased + its MLM head): tools/splade_bench.py
SPLADE_BERT_BASE = EncoderConfig(arch="bert", vocab_size=30522, hidden=768, layers=12, heads=12, ffn=3072, max_pos=512, type_vocab=2,
                                 pad_id=0, ln_eps=1e-12)
