"""Metadata filters on the host: the filter-spec builder (the reference's ``_build_metadata_filters`` behaviour, restated),
clause bitsets over the vocabulary against a plain per-row evaluator of the matching table, filter keys."""
import itertools

import numpy as np
import pytest

import tensor_truth_amd  # noqa: F401
from tensor_truth_amd import metadata_filter as mf
from tensor_truth_amd.schema import FilterCondition, FilterOperator, MetadataFilter, MetadataFilters


# ---- build_metadata_filters (reference tests/unit/test_rag_engine.py:447-500, restated) ------------------------------------
def test_spec_simple_equality():
    f = mf.build_metadata_filters({"doc_type": "library"})
    assert len(f.filters) == 1
    assert f.filters[0].key == "doc_type" and f.filters[0].value == "library"
    assert mf._op_name(f.filters[0].operator) == "=="
    assert mf.clauses_of(f)[1] is False          # AND


def test_spec_multiple_conditions():
    f = mf.build_metadata_filters({"doc_type": "library", "source": "pytorch"})
    assert len(f.filters) == 2 and getattr(f.condition, "value", f.condition) == "and"


def test_spec_operator_syntax_reads_only_the_first_key():
    f = mf.build_metadata_filters({"version": {"$gte": "2.0", "$lt": "3.0"}})
    assert len(f.filters) == 1
    assert f.filters[0].key == "version" and f.filters[0].value == "2.0" and f.filters[0].operator == FilterOperator.GTE


def test_spec_every_operator():
    want = {"$eq": "==", "$ne": "!=", "$gt": ">", "$gte": ">=", "$lt": "<", "$lte": "<=", "$in": "in", "$nin": "nin",
            "$contains": "contains", "$text_match": "text_match"}
    for op, name in want.items():
        f = mf.build_metadata_filters({"k": {op: 1}})
        assert mf._op_name(f.filters[0].operator) == name


def test_spec_unknown_operator_is_skipped():
    assert mf.build_metadata_filters({"k": {"$regex": "x"}}) is None
    f = mf.build_metadata_filters({"k": {"$regex": "x"}, "j": 3})
    assert [x.key for x in f.filters] == ["j"]
    # the first key decides: a known operator behind an unknown one is not read
    assert mf.build_metadata_filters({"k": {"$regex": "x", "$eq": 1}}) is None


def test_spec_empty_or_none():
    assert mf.build_metadata_filters({}) is None
    assert mf.build_metadata_filters(None) is None


def test_spec_list_values_use_in():
    f = mf.build_metadata_filters({"doc_type": ["library", "book"]})
    assert len(f.filters) == 1 and f.filters[0].operator == FilterOperator.IN and f.filters[0].value == ["library", "book"]


# ---- per-row table vs compiled bitsets ---------------------------------------------------------------------------------------
VALUES = [1, 1.0, 2, 2.5, 0, True, False, "1", "2.0", "library", "lib", "a library book", None, [1, 2], ["x", "y"], (1, "x"),
          [True], [], "", 3.0, -1]
ABSENT = mf._MISSING


def plain_row(op, v, f) -> bool:
    """The matching table, written out independently of metadata_filter's helpers."""
    if v is ABSENT:
        return False

    def kind(x):
        if isinstance(x, bool):
            return "b"
        if isinstance(x, (int, float)):
            return "n"
        return type(x).__name__

    def eq(a, b):
        if kind(a) != kind(b):
            return False
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(eq(x, y) for x, y in zip(a, b))
        return a == b

    if op == "==":
        return eq(v, f)
    if op == "!=":
        return not eq(v, f)
    if op in (">", ">=", "<", "<="):
        if not (kind(v) == kind(f) and kind(v) in ("n", "str")):
            return False
        return {">": v > f, ">=": v >= f, "<": v < f, "<=": v <= f}[op]
    if op == "in":
        return any(eq(v, x) for x in f)
    if op == "nin":
        return not any(eq(v, x) for x in f)
    if op == "contains":
        return isinstance(v, (list, tuple)) and any(eq(x, f) for x in v)
    assert op == "text_match"
    return isinstance(v, str) and isinstance(f, str) and f in v


FILTER_VALUES = {
    "==": [1, 1.0, True, "1", [1, 2], (1, "x"), None, 0],
    "!=": [1, True, "library", [1, 2]],
    ">": [1, 1.5, "2", "l", True],
    ">=": [1.0, "library", 2],
    "<": [2, "b", 0.5, False],
    "<=": [1, "lib", 2.5],
    "in": [[1, "1"], [True], [2.0, "lib"], [[1, 2], None], []],
    "nin": [[1], ["library", False], []],
    "contains": [1, "x", True, 2.0, "y"],
    "text_match": ["lib", "library", "", "1", 1],
}


def _rows(key, values):
    """A fake docstore over rows whose metadata holds `values` (ABSENT: key missing) -> (codes, per-row values)."""
    docstore, ids = {}, []
    for i, v in enumerate(values):
        class N:
            pass
        nd = N()
        nd.metadata = {} if v is ABSENT else {key: v}
        nd.metadata["other"] = i
        docstore[f"n{i}"] = nd
        ids.append(f"n{i}")
    ids.append(None)                                          # a deleted row: no node, code 0
    codes = mf.VOCAB.key(key).codes(mf.metadata_values(docstore, ids, key))
    return codes, list(values) + [ABSENT]


@pytest.mark.parametrize("op", sorted(FILTER_VALUES))
def test_compiled_bitsets_equal_the_per_row_table(op):
    key = f"k_{op}"
    codes, vals = _rows(key, VALUES + [ABSENT, ABSENT])
    assert codes[-1] == 0 and codes[-2] == 0
    for f in FILTER_VALUES[op]:
        allowed = mf.compile_clause(key, op, f)
        assert not allowed[0], "code 0 (key absent) must never pass"
        got = [bool(allowed[c]) if c < len(allowed) else False for c in codes]
        want = [plain_row(op, v, f) for v in vals]
        assert got == want, (op, f)
        # the device form: bit c % 32 of word c // 32
        words = mf.pack_bits(allowed)
        assert [bool((int(words[c >> 5]) >> (c & 31)) & 1) for c in range(len(allowed))] == list(allowed)


def test_types_stay_distinct_in_the_vocabulary():
    kv = mf.VOCAB.key("distinct_types")
    c = kv.codes([1, 1.0, True, "1", 0, False, [1], [True], (1,), [1.0]])
    assert c[0] == c[1], "equal int and float share a code"
    assert len({c[0], c[2], c[3]}) == 3 and c[4] != c[5]
    assert c[6] != c[7] and c[6] != c[8] and c[6] == c[9]


def test_vocabulary_is_append_only_and_shared():
    a = mf.VOCAB.key("shared_key").codes(["x", "y"])
    b = mf.VOCAB.key("shared_key").codes(["y", "z", "x"])
    assert b[0] == a[1] and b[2] == a[0] and b[1] == max(a) + 1


def test_bitset_grows_with_the_vocabulary():
    key = "growing"
    mf.VOCAB.key(key).codes(["a", "b"])
    first = mf.compile_clause(key, "in", ["b", "c"])
    c = mf.VOCAB.key(key).codes(["c"])[0]
    second = mf.compile_clause(key, "in", ["b", "c"])
    assert len(second) > len(first) and second[c] and list(second[: len(first)]) == list(first)


def _combine(any_, per_clause):
    return [any(x) if any_ else all(x) for x in zip(*per_clause)]


@pytest.mark.parametrize("cond", ["and", "or"])
def test_and_or_over_several_keys(cond):
    rng = np.random.default_rng(3)
    n = 300
    a_vals = [ABSENT if rng.random() < 0.1 else int(rng.integers(0, 5)) for _ in range(n)]
    b_vals = [ABSENT if rng.random() < 0.1 else str(rng.choice(["x", "y", "xy", "z"])) for _ in range(n)]
    ca, va = _rows("and_or_a", a_vals)
    cb, vb = _rows("and_or_b", b_vals)
    clauses = [("and_or_a", ">=", 2), ("and_or_b", "text_match", "x")]
    per = []
    for (key, op, f), codes in zip(clauses, (ca, cb)):
        allowed = mf.compile_clause(key, op, f)
        per.append([bool(allowed[c]) if c < len(allowed) else False for c in codes])
    got = _combine(cond == "or", per)
    want = _combine(cond == "or", [[plain_row(">=", v, 2) for v in va], [plain_row("text_match", v, "x") for v in vb]])
    assert got == want
    filt = MetadataFilters(filters=[MetadataFilter(key=k, value=f, operator=op) for k, op, f in clauses],
                           condition=FilterCondition.OR if cond == "or" else FilterCondition.AND)
    assert mf.clauses_of(filt)[1] is (cond == "or")


def test_counts_bound_the_matching_rows():
    key = "bounded"
    vals = ["a"] * 5 + ["b"] * 3 + [ABSENT] * 2
    codes, _ = _rows(key, vals)

    class Col:                      # the CodeColumn arithmetic without a device
        counts = np.bincount(codes).astype(np.int64)
    allowed = mf.compile_clause(key, "==", "a")
    assert mf.CodeColumn.bound(Col(), allowed) == 5
    allowed = mf.compile_clause(key, "!=", "a")
    assert mf.CodeColumn.bound(Col(), allowed) == 3


# ---- filter keys, refusals ---------------------------------------------------------------------------------------------------
def test_filter_key_is_canonical():
    spec = {"doc_type": ["library", "book"], "version": {"$gte": 2}, "flag": True}
    a, b = mf.build_metadata_filters(spec), mf.build_metadata_filters(dict(spec))
    assert mf.filter_key(a) == mf.filter_key(b) and hash(mf.filter_key(a)) == hash(mf.filter_key(b))
    assert mf.filter_key(mf.build_metadata_filters({"v": 1})) == mf.filter_key(mf.build_metadata_filters({"v": 1.0}))
    assert mf.filter_key(mf.build_metadata_filters({"v": 1})) != mf.filter_key(mf.build_metadata_filters({"v": True}))
    assert mf.filter_key(mf.build_metadata_filters({"v": 1})) != mf.filter_key(mf.build_metadata_filters({"v": "1"}))
    assert mf.filter_key(None) is None and mf.filter_key(MetadataFilters(filters=[])) is None
    ored = MetadataFilters(filters=list(a.filters), condition=FilterCondition.OR)
    assert mf.filter_key(ored) != mf.filter_key(a)


def test_nested_filters_and_unknown_operators_raise():
    inner = MetadataFilters(filters=[MetadataFilter(key="a", value=1)])
    with pytest.raises(ValueError):
        mf.filter_key(MetadataFilters(filters=[inner]))
    with pytest.raises(ValueError):
        mf.filter_key(MetadataFilters(filters=[MetadataFilter(key="a", value=1, operator="regex")]))
    with pytest.raises(ValueError):
        mf.row_matches("~", True, 1, 1)
    with pytest.raises(ValueError):
        mf.filter_key(MetadataFilters(filters=[MetadataFilter(key=f"k{i}", value=i) for i in range(9)]))


def test_every_operator_value_is_accepted_as_enum_or_string():
    for op in FilterOperator:
        assert mf._op_name(op) == mf._op_name(op.value)
    assert len(list(itertools.islice(FilterOperator, 20))) >= 10
