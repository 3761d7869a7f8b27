"""Metadata filters for the exact scan: the ``where=`` of the reference's vector-store query.

The reference builds llama-index ``MetadataFilters`` from a filter spec (``_build_metadata_filters``,
``src/tensortruth/rag_engine.py:286-365``) and hands them to ``index.as_retriever(filters=...)``.  Here a filter selects the
rows of the matrix first (``tt_filter_rows``, csrc/filter.hip) and the exact top-k then runs over exactly those rows
(``tt_scan_topk_rows``): bit-identical to ``tt_scan_topk`` over the gathered matching rows.

Matching is defined per row.  A row is a leaf of the matrix; its value ``v`` is ``docstore[leaf_id].metadata[key]``, ``f`` is
the filter's value:

    ==========================  =============================================================================
    Operator                    A row matches when
    ==========================  =============================================================================
    EQ                          ``v == f``
    NE                          the key is present and ``v != f``
    GT, GTE, LT, LTE            both values are numeric, or both are ``str`` (any other pair: no match, no error)
    IN                          ``v`` equals some element of ``f``
    NIN                         the key is present and ``v`` equals no element of ``f``
    CONTAINS                    ``v`` is a list or tuple and ``f`` is in it
    TEXT_MATCH                  both are ``str`` and ``f`` is a substring of ``v``
    ==========================  =============================================================================

Two rules cover every operator: a missing key matches nothing (NE and NIN included), and types stay distinct -- ``bool`` is
neither ``1`` nor ``0``, ``"1"`` is not ``1``; equal ``int`` and ``float`` values are equal (also inside lists).

Encoding.  Every filterable key has one process-wide, append-only vocabulary (``VOCAB``): a value's code is its position + 1
(0 = key absent), so codes mean the same thing in every index and a ``HipIndexGroup`` concatenates its modules' code columns
as they are.  A clause is evaluated ONCE over the vocabulary's distinct values into an allowed-code bitset, which makes every
operator the same device test ``bit[code[row]]``.  A column keeps per-code row counts, so the host knows an upper bound on the
matching rows (the workspace size) without asking the device.
"""
from __future__ import annotations

import math
import threading
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .schema import FilterCondition, FilterOperator, MetadataFilter, MetadataFilters

MAX_CLAUSES = 8          # per filter (tt_filter_rows)

_OPS = ("==", "!=", ">", ">=", "<", "<=", "in", "nin", "contains", "text_match")

# the reference's spec operators (rag_engine.py:286-297)
_SPEC_OPERATORS = {
    "$eq": FilterOperator.EQ,
    "$ne": FilterOperator.NE,
    "$gt": FilterOperator.GT,
    "$gte": FilterOperator.GTE,
    "$lt": FilterOperator.LT,
    "$lte": FilterOperator.LTE,
    "$in": FilterOperator.IN,
    "$nin": FilterOperator.NIN,
    "$contains": FilterOperator.CONTAINS,
    "$text_match": FilterOperator.TEXT_MATCH,
}


def build_metadata_filters(filter_spec: Optional[Dict[str, Any]]) -> Optional[MetadataFilters]:
    """A filter spec -> ``MetadataFilters`` (AND of the entries), or None for an empty spec.

    ``{"doc_type": "library"}`` is EQ, ``{"doc_type": ["library", "book"]}`` is IN, ``{"version": {"$gte": "2.0"}}`` takes the
    operator of the dict's FIRST key (an unknown ``$op`` drops the entry).  A spec whose every entry was dropped gives None."""
    if not filter_spec:
        return None
    out = []
    for key, value in filter_spec.items():
        if isinstance(value, dict):
            first = next(iter(value.items()), None)
            if first is not None and first[0] in _SPEC_OPERATORS:
                out.append(MetadataFilter(key=key, value=first[1], operator=_SPEC_OPERATORS[first[0]]))
        elif isinstance(value, list):
            out.append(MetadataFilter(key=key, value=value, operator=FilterOperator.IN))
        else:
            out.append(MetadataFilter(key=key, value=value))
    if not out:
        return None
    return MetadataFilters(filters=out, condition=FilterCondition.AND)


# ---- typed equality and the per-row rule ---------------------------------------------------------------------------------------
def _kind(v) -> str:
    if isinstance(v, bool):
        return "b"
    if isinstance(v, (int, float)):
        return "n"
    if isinstance(v, str):
        return "s"
    if isinstance(v, list):
        return "L"
    if isinstance(v, tuple):
        return "T"
    if v is None:
        return "0"
    return "o:" + type(v).__name__


def _eq(a, b) -> bool:
    ka = _kind(a)
    if ka != _kind(b):
        return False
    if ka in ("L", "T"):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    try:
        return bool(a == b)
    except Exception:  # noqa: BLE001
        return False


def value_key(v):
    """Hashable key under which equal values (``_eq``) meet: the vocabulary's dictionary key and the filter key's value part."""
    k = _kind(v)
    if k in ("L", "T"):
        return (k, tuple(value_key(x) for x in v))
    if k == "n" and isinstance(v, float) and math.isnan(v):
        return ("nan",)
    if k in ("b", "n", "s"):
        return (k, v)
    if k == "0":
        return ("0",)
    try:
        hash(v)
        return (k, v)
    except TypeError:
        return (k, repr(v))


def _op_name(op) -> str:
    name = getattr(op, "value", op)
    if name not in _OPS:
        raise ValueError(f"unsupported filter operator {op!r}: one of {', '.join(_OPS)}")
    return name


def _ordered(v, f) -> bool:
    kv, kf = _kind(v), _kind(f)
    return kv == kf and kv in ("n", "s")


def row_matches(op, present: bool, v, f) -> bool:
    """The table of the module docstring for one row (``present``: the row's metadata has the key)."""
    op = _op_name(op)
    if not present:
        return False
    if op == "==":
        return _eq(v, f)
    if op == "!=":
        return not _eq(v, f)
    if op in (">", ">=", "<", "<="):
        if not _ordered(v, f):
            return False
        return {">": v > f, ">=": v >= f, "<": v < f, "<=": v <= f}[op]
    if op in ("in", "nin"):
        elems = f if isinstance(f, (list, tuple, set, frozenset)) else [f]
        hit = any(_eq(v, x) for x in elems)
        return hit if op == "in" else not hit
    if op == "contains":
        return isinstance(v, (list, tuple)) and any(_eq(x, f) for x in v)
    return isinstance(v, str) and isinstance(f, str) and f in v        # text_match


def clauses_of(filters) -> Tuple[List[Tuple[str, str, Any]], bool]:
    """``MetadataFilters`` -> ([(key, operator value, filter value)], any); ValueError for nested filters, unknown operators or
    conditions, more than MAX_CLAUSES clauses."""
    cond = getattr(getattr(filters, "condition", "and"), "value", getattr(filters, "condition", "and"))
    cond = "and" if cond is None else str(cond).lower()
    if cond not in ("and", "or"):
        raise ValueError(f"unsupported filter condition {cond!r}: and / or")
    out = []
    for f in list(getattr(filters, "filters", None) or []):
        if hasattr(f, "filters"):
            raise ValueError("nested MetadataFilters are not supported")
        out.append((str(f.key), _op_name(getattr(f, "operator", "==")), f.value))
    if len(out) > MAX_CLAUSES:
        raise ValueError(f"{len(out)} filter clauses: at most {MAX_CLAUSES}")
    return out, cond == "or"


def filter_key(filters):
    """Canonical, hashable key of a ``MetadataFilters`` (None for None or no clauses): equal filters built twice -> equal keys."""
    if filters is None:
        return None
    clauses, any_ = clauses_of(filters)
    if not clauses:
        return None
    return ("or" if any_ else "and", tuple((k, op, value_key(v)) for k, op, v in clauses))


# ---- vocabulary ---------------------------------------------------------------------------------------------------------------
class KeyVocab:
    """Append-only dictionary of one key's distinct values: code = position + 1."""

    def __init__(self):
        self.values: List[Any] = []
        self.index: Dict[Any, int] = {}
        self.lock = threading.Lock()

    def codes(self, values) -> np.ndarray:
        """Codes of ``values`` (``_MISSING`` -> 0), learning the new ones."""
        out = np.zeros(len(values), dtype=np.int32)
        with self.lock:
            for i, v in enumerate(values):
                if v is _MISSING:
                    continue
                vk = value_key(v)
                c = self.index.get(vk)
                if c is None:
                    self.values.append(v)
                    c = self.index[vk] = len(self.values)
                out[i] = c
        return out

    def snapshot(self) -> List[Any]:
        with self.lock:
            return list(self.values)


class Vocabulary:
    def __init__(self):
        self._keys: Dict[str, KeyVocab] = {}
        self._lock = threading.Lock()

    def key(self, name: str) -> KeyVocab:
        with self._lock:
            kv = self._keys.get(name)
            if kv is None:
                kv = self._keys[name] = KeyVocab()
            return kv


VOCAB = Vocabulary()
_MISSING = object()


def metadata_values(docstore, leaf_ids, key: str) -> list:
    """The key's value per row (``_MISSING`` for a deleted row or a node without the key)."""
    out = []
    for nid in leaf_ids:
        nd = docstore.get(nid) if nid is not None else None
        md = getattr(nd, "metadata", None) if nd is not None else None
        out.append(md[key] if isinstance(md, dict) and key in md else _MISSING)
    return out


# ---- clause bitsets -----------------------------------------------------------------------------------------------------------
class _BitsetCache:
    """(key, op, value key) -> allowed-code mask over the vocabulary seen so far, extended as the vocabulary grows; device copies
    per (clause, device, n_codes)."""

    def __init__(self, max_entries: int = 256):
        self.masks: Dict[Any, np.ndarray] = {}
        self.dev: Dict[Any, torch.Tensor] = {}
        self.max_entries = max_entries
        self.lock = threading.Lock()

    def allowed(self, key: str, op: str, f) -> np.ndarray:
        """bool [n_codes]: code c passes the clause (c = 0, key absent, never does)."""
        ck = (key, op, value_key(f))
        values = VOCAB.key(key).snapshot()
        n = len(values) + 1
        with self.lock:
            m = self.masks.get(ck)
        if m is None or len(m) < n:
            old = 0 if m is None else len(m)
            new = np.zeros(n, dtype=bool)
            if m is not None:
                new[:old] = m
            for c in range(max(old, 1), n):
                new[c] = row_matches(op, True, values[c - 1], f)
            m = new
            with self.lock:
                if len(self.masks) >= self.max_entries:
                    self.masks.clear()
                    self.dev.clear()
                self.masks[ck] = m
        return m[:n]

    def device_bits(self, key: str, op: str, f, allowed: np.ndarray, device) -> torch.Tensor:
        ck = (key, op, value_key(f), str(device), len(allowed))
        with self.lock:
            t = self.dev.get(ck)
        if t is None:
            t = torch.from_numpy(pack_bits(allowed).view(np.int32)).to(device)
            with self.lock:
                self.dev[ck] = t
        return t


_BITS = _BitsetCache()


def pack_bits(allowed: np.ndarray) -> np.ndarray:
    """bool [n] -> uint32 [ceil(n / 32)], bit c % 32 of word c // 32 = allowed[c]."""
    n = len(allowed)
    words = max((n + 31) // 32, 1)
    padded = np.zeros(words * 32, dtype=np.uint64)
    padded[:n] = allowed
    w = (padded.reshape(words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    return w.astype(np.uint32)


def compile_clause(key: str, op: str, f) -> np.ndarray:
    return _BITS.allowed(key, op, f)


# ---- code columns -------------------------------------------------------------------------------------------------------------
class CodeColumn:
    """One key's codes for the rows of one index matrix, in row order, plus per-code row counts.  Device storage grows by
    doubling (like the matrix); rows below ``n`` are never rewritten, so a tensor handed to a search stays valid for its rows."""

    def __init__(self, key: str, device, codes: np.ndarray, cap: Optional[int] = None):
        self.key, self.device = key, device
        self.n = len(codes)
        cap = max(cap or 0, self.n, 1024)
        self.dev = torch.zeros(cap, dtype=torch.int32, device=device)
        if self.n:
            self.dev[: self.n] = torch.from_numpy(codes).to(device)
        self.counts = np.bincount(codes, minlength=1).astype(np.int64) if self.n else np.zeros(1, np.int64)

    @classmethod
    def from_device(cls, key: str, device, codes: torch.Tensor, counts: Optional[np.ndarray] = None) -> "CodeColumn":
        """A column over device codes as they are (a compaction's kept rows, a group's concatenated modules); counts computed
        on the device unless given."""
        col = cls.__new__(cls)
        col.key, col.device = key, device
        col.n = int(codes.shape[0])
        col.dev = torch.zeros(max(col.n, 1024), dtype=torch.int32, device=device)
        col.dev[: col.n] = codes
        if counts is None:
            counts = torch.bincount(codes.long(), minlength=1).cpu().numpy().astype(np.int64) if col.n else np.zeros(1, np.int64)
        col.counts = counts
        return col

    def reserve(self, rows: int) -> None:
        if rows > self.dev.shape[0]:
            grown = torch.zeros(max(rows, 2 * self.dev.shape[0]), dtype=torch.int32, device=self.device)
            grown[: self.n] = self.dev[: self.n]
            self.dev = grown

    def append(self, codes: np.ndarray) -> None:
        self.reserve(self.n + len(codes))
        if len(codes):
            self.dev[self.n: self.n + len(codes)] = torch.from_numpy(codes).to(self.device)
            bc = np.bincount(codes)
            if len(bc) > len(self.counts):
                self.counts = np.concatenate([self.counts, np.zeros(len(bc) - len(self.counts), np.int64)])
            self.counts[: len(bc)] += bc
        self.n += len(codes)

    def bound(self, allowed: np.ndarray) -> int:
        """Rows whose code passes (an upper bound on the matching live rows: tombstones keep their codes)."""
        m = min(len(allowed), len(self.counts))
        return int(self.counts[:m][allowed[:m]].sum())


class CompiledFilter:
    """A filter made ready for ``tt_filter_rows``: per clause (device code column, device bitset, n_codes), AND / OR, and the
    host's upper bound on the matching rows."""

    def __init__(self, columns: List[torch.Tensor], bitsets: List[torch.Tensor], n_codes: List[int], any_: bool, bound: int):
        self.columns, self.bitsets, self.n_codes, self.any, self.bound = columns, bitsets, n_codes, any_, bound


def compile_filter(filters, columns_for, n_rows: int, device) -> CompiledFilter:
    """``columns_for(key)`` -> CodeColumn covering at least ``n_rows`` rows (an index's or a group's packed one)."""
    clauses, any_ = clauses_of(filters)
    cols, bits, ncodes, bounds = [], [], [], []
    for key, op, f in clauses:
        col = columns_for(key)
        allowed = compile_clause(key, op, f)
        cols.append(col.dev)
        bits.append(_BITS.device_bits(key, op, f, allowed, device))
        ncodes.append(len(allowed))
        bounds.append(col.bound(allowed))
    bound = min(sum(bounds), n_rows) if any_ else min(min(bounds), n_rows)
    return CompiledFilter(cols, bits, ncodes, any_, bound)
