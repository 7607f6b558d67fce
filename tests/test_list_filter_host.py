"""`json_contains` / `json_contains_any` / `json_contains_all` on the host: the grammar, the predicate's semantics, the compiled
program against the predicate (restated in numpy over the typed list columns: tests/list_filter_cases.py), `MetaColumn`'s list
part, and the store's host route through the CPU stand-ins of tests/test_filter_route_host.py."""
import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from list_filter_cases import EXPRESSIONS, KEYS, any_per_row, columns_of, expected, interpret, leaf_answers, list_rows
from test_filter_route_host import DIM, VOCAB, _data, _dump, stand_ins  # noqa: F401
from verbatim_rag_amd import vector_stores as vs
from verbatim_rag_amd.store_columns import KIND_BOOL, KIND_NUMBER, KIND_OTHER, KIND_STRING, MetaColumn
from verbatim_rag_amd.store_filter import MAX_LEAVES, compile_filter, parse_filter, parse_filter_ast

ROWS = list_rows(2000, seed=7)
COLUMNS = dict(zip(KEYS, columns_of(ROWS, KEYS)))


# ------------------------------------------------------------------------------------------ grammar
ACCEPTED = {
    'json_contains(metadata["a"], "x")': ("has", "a", ("s", "x")),
    "json_contains(a, 'x')": ("has", "a", ("s", "x")),
    "JSON_CONTAINS(a, 7)": ("has", "a", ("n", 7.0)),
    "json_contains ( a , -2.5e0 )": ("has", "a", ("n", -2.5)),
    "json_contains(a, true)": ("has", "a", ("b", True)),
    "json_contains(a, FALSE)": ("has", "a", ("b", False)),
    'json_contains_any(a, ["x"])': ("has", "a", ("s", "x")),
    'json_contains_any(a, ["x", 1, true])': ("or", ("or", ("has", "a", ("s", "x")), ("has", "a", ("n", 1.0))), ("has", "a", ("b", True))),
    'JSON_CONTAINS_ANY(metadata["a"], [1, 2])': ("or", ("has", "a", ("n", 1.0)), ("has", "a", ("n", 2.0))),
    "json_contains_all(a, [1, 2, 3])": ("and", ("and", ("has", "a", ("n", 1.0)), ("has", "a", ("n", 2.0))), ("has", "a", ("n", 3.0))),
    'JSON_CONTAINS_ALL(a, ["x"])': ("has", "a", ("s", "x")),
    "not json_contains(a, 1)": ("not", ("has", "a", ("n", 1.0))),
    "(json_contains(a, 1))": ("has", "a", ("n", 1.0)),
    "json_contains(a, 1) and b == 2 or json_contains(c, 3)":
        ("or", ("and", ("has", "a", ("n", 1.0)), ("cmp", "b", "==", ("n", 2.0))), ("has", "c", ("n", 3.0))),
    # a bare word is a field name unless a `(` follows one of the six spellings
    "json_contains == 3": ("cmp", "json_contains", "==", ("n", 3.0)),
    "JSON_CONTAINS_ALL != 3": ("cmp", "JSON_CONTAINS_ALL", "!=", ("n", 3.0)),
    "Json_Contains == 3": ("cmp", "Json_Contains", "==", ("n", 3.0)),
    "json_contains_any in [1]": ("in", "json_contains_any", [("n", 1.0)]),
    '(json_contains == 3) and json_contains LIKE "x%"': ("and", ("cmp", "json_contains", "==", ("n", 3.0)), ("like", "json_contains", "x%")),
    "json_contains(json_contains, 1)": ("has", "json_contains", ("n", 1.0)),
}
REFUSED = {
    "Json_Contains(a, 1)": "JSON_CONTAINS",                  # any other casing in front of a `(` names the accepted spellings
    "json_Contains_any(a, [1])": "json_contains_any",
    "JSON_contains_ALL(a, [1])": "JSON_CONTAINS_ALL",
    "json_contains_any(a, [])": "empty list",
    "json_contains_all(a, [])": "empty list",
    "json_contains(a, [1])": "a list or an object",
    "json_contains_any(a, [[1]])": "a list or an object",
    'json_contains(a, {"x": 1})': "cannot parse",
    'json_contains_all(a, [{"x": 1}])': "cannot parse",
    "json_contains(a)": "takes (field, value)",
    "json_contains(a, 1, 2)": "takes (field, value)",
    "json_contains()": "takes a field first",
    "json_contains(1, a)": "takes a field first",
    "json_contains_any(a, 1)": "[value, ...]",
    "json_contains_any(a)": "[value, ...]",
    "json_contains_any(a, [1], [2])": "[value, ...]",
    "json_contains_all(a, [1,])": "a quoted string, a number",
    "json_contains(a, b)": "a quoted string, a number",
    "json_contains(a, 1": "expected ')'",
    "json_contains a, 1": "unsupported filter",
    "json_contains(LIKE, 1)": "takes a field first",
    # out of scope, as before
    "array_length(a) == 2": "GpuVectorStore: ",
    'metadata["a"][0] == 1': "GpuVectorStore: ",
    "a is null": "GpuVectorStore: ",
    "exists a": "GpuVectorStore: ",
    'TEXT_MATCH(a, "x")': "GpuVectorStore: ",
    "json_contains(a, 1) json_contains(a, 2)": "unsupported filter",
}


def test_accepted_spellings_and_their_trees():
    for expr, tree in ACCEPTED.items():
        assert parse_filter_ast(expr) == tree, expr
        parse_filter(expr), compile_filter(expr)


def test_refusals_are_value_errors_on_both_back_ends():
    for expr, piece in REFUSED.items():
        with pytest.raises(ValueError) as one:
            parse_filter(expr)
        with pytest.raises(ValueError) as two:
            compile_filter(expr)
        assert str(one.value) == str(two.value) and str(one.value).startswith("GpuVectorStore: "), expr
        assert piece in str(one.value), (expr, str(one.value))
    message = str(pytest.raises(ValueError, parse_filter, "Json_Contains(a, 1)").value)
    for spelling in ("json_contains", "json_contains_any", "json_contains_all", "JSON_CONTAINS", "JSON_CONTAINS_ANY", "JSON_CONTAINS_ALL"):
        assert spelling in message


def test_a_membership_has_no_value_index_lookup():
    assert not hasattr(parse_filter("json_contains(a, 1)"), "lookup")
    assert not hasattr(parse_filter("json_contains_any(a, [1])"), "lookup")
    assert parse_filter("a == 1").lookup == ("a", [("n", 1.0)])


# ------------------------------------------------------------------------------------------ semantics
NOT_LISTS = [{}, {"b": [1]}, {"a": None}, {"a": 5}, {"a": "5"}, {"a": True}, {"a": {"0": 5}}, {"a": 2020.0}]


@pytest.mark.parametrize("expr, passing, failing", [
    ("json_contains(a, 2020)", [[2020], [2020.0], [1, 2020.0, "x"], (2020,), [2020, 2020]], [["2020"], [2021], [[2020]], [{"v": 2020}], [None], []]),
    ("json_contains(a, 2020.0)", [[2020], [2020.0]], [["2020.0"], []]),
    ('json_contains(a, "5")', [["5"], ["x", "5"], ["5", "5", "5"]], [[5], [5.0], ["55"], [" 5"], [None, ["5"], {"5": "5"}], []]),
    ("json_contains(a, 5)", [[5], [5.0], [True, 5]], [["5"], [True], []]),
    ("json_contains(a, true)", [[True], [False, True], [1, True]], [[1], [1.0], ["true"], [False], []]),
    ("json_contains(a, 1)", [[1], [1.0]], [[True], ["1"], []]),
    ("json_contains(a, false)", [[False]], [[0], [-0.0], [""], [None], []]),
    ("json_contains(a, 0)", [[0], [-0.0], [0.0]], [[False], ["0"], []]),
    ("json_contains(a, -0.0)", [[0], [-0.0], [0.0]], [[False], []]),
    ('json_contains(a, "")', [[""], ["x", ""]], [[None], [[]], [0], []]),
    ('json_contains_any(a, ["x", 5])', [["x"], [5.0], ["x", 5], ["y", "x"]], [["5"], ["y"], [["x"]], []]),
    ('json_contains_all(a, ["x", 5])', [["x", 5], [5.0, "y", "x"], [5, 5, "x", "x"]], [["x"], [5], ["x", "5"], []]),
    ('json_contains_all(a, ["x", "x"])', [["x"]], [["y"], []]),
])
def test_semantics(expr, passing, failing):
    pred, negated = parse_filter(expr), parse_filter(f"not {expr}")
    for value in passing:
        assert pred({"a": value}) is True and negated({"a": value}) is False, (expr, value)
    for value in failing:
        assert pred({"a": value}) is False and negated({"a": value}) is True, (expr, value)
    for md in NOT_LISTS:                     # a missing key, a scalar (also one equal to the value), a dict: never, so `not` holds
        assert pred(md) is False and negated(md) is True, (expr, md)


def test_semantic_rows_through_the_compiled_program_too():
    rows = NOT_LISTS + [{"a": v} for v in ([2020], [2020.0], ["2020"], [5], ["5"], [True], [1], [False], [0], [-0.0], [None, [5], {"5": 5}],
                                           [], (5, "5"), [5, 5, 5], ["x", 5])]
    for expr in ("json_contains(a, 2020)", 'json_contains(a, "5")', "json_contains(a, 5)", "json_contains(a, true)", "json_contains(a, 1)",
                 "json_contains(a, 0)", "json_contains(a, -0.0)", "json_contains(a, false)", 'json_contains_all(a, ["x", 5])',
                 'not json_contains_any(a, ["x", 5])', "not json_contains(a, 5)"):
        prog = compile_filter(expr)
        want = expected(expr, rows)
        assert np.array_equal(interpret(prog, columns_of(rows, prog.keys)), want), expr
        assert want.any() and not want.all(), expr


# ------------------------------------------------------------------------------------------ program parity
def test_the_corpus_is_what_the_parity_test_needs():
    assert len(EXPRESSIONS) >= 20
    for key in ("authors", "tags", "years", "flags"):
        values = [md.get(key) for md in ROWS]
        lists = [v for v in values if isinstance(v, (list, tuple))]
        assert 0.6 < len(lists) / len(ROWS) < 0.8                          # about three rows in ten hold no list
        lengths = {len(v) for v in lists}
        assert {0, 1, 2, 5, 70} <= lengths and max(lengths) == 70
        assert any(isinstance(v, tuple) for v in lists) and any(v is None for v in values) and any(isinstance(v, dict) for v in values)
    kinds = {type(e) for md in ROWS if isinstance(md.get("tags"), (list, tuple)) for e in md["tags"]}
    assert {int, float, str, bool, type(None), list, dict} <= kinds
    assert all(c.exact and c.list_exact and c.encodable for c in COLUMNS.values())
    text = " ".join(EXPRESSIONS)
    for piece in ("json_contains(", "json_contains_any(", "json_contains_all(", "JSON_CONTAINS(", "JSON_CONTAINS_ALL(", " LIKE ", " in [", ">=",
                  "<", "!=", "==", "not ", " and ", " or ", "&&", 'metadata["'):
        assert piece in text, piece


@pytest.mark.parametrize("expr", EXPRESSIONS)
def test_program_equals_the_predicate(expr):
    want = expected(expr, ROWS)
    assert want.any() and not want.all(), expr                             # by the closures alone: no mask that hides a defect
    prog = compile_filter(expr)
    assert prog.over_limit() is None
    got = interpret(prog, [COLUMNS[k] for k in prog.keys])
    assert np.array_equal(got, want), (expr, np.nonzero(got != want)[0][:8])


def test_a_has_is_one_eq_leaf_pushed_as_list_any():
    prog = compile_filter('json_contains_any(a, ["x", 2]) and not b >= 2 and json_contains(b, true)')
    assert prog.keys == ["a", "b"]
    assert prog.ops == [("list_any", 0), ("list_any", 1), ("or", 0), ("leaf", 2), ("not", 0), ("and", 0), ("list_any", 3), ("and", 0)]
    assert prog.leaves[0] == compile_filter('a == "x"').leaves[0] and prog.leaves[1] == compile_filter("a == 2").leaves[0]
    assert prog.leaves[3].column == 1 and prog.leaves[3].bools == (False, True) and prog.leaves[3].other is False
    assert prog.depth() == 2
    many = compile_filter("json_contains_any(a, [" + ", ".join(str(i) for i in range(MAX_LEAVES + 1)) + "])")
    assert "65 leaves" in many.over_limit()                                # a `has` counts as a leaf
    assert compile_filter("json_contains_all(a, [" + ", ".join(str(i) for i in range(MAX_LEAVES)) + "])").over_limit() is None


# ------------------------------------------------------------------------------------------ MetaColumn
def f64(x) -> int:
    return int(np.float64(x).view(np.uint64))


def test_list_encoding_shares_the_dictionary_with_scalars():
    col = MetaColumn("v")
    col.extend([{"v": "x"}, {"v": ["y", "x", 5, True, None, [1], {"a": 1}, -0.0]}, {"v": 5}, {}, {"v": []}, {"v": ("z", False)}, {"v": "y"}])
    assert col.kinds.tolist() == [KIND_STRING, KIND_OTHER, KIND_NUMBER, KIND_OTHER, KIND_OTHER, KIND_OTHER, KIND_STRING]
    assert col.payload.tolist() == [0, 0, f64(5.0), 0, 0, 0, 1]
    assert col.strings == ["x", "y", "z"]                                  # first-seen order, scalar or element
    assert col.elem_off.dtype == np.int64 and col.elem_off.tolist() == [0, 0, 8, 8, 8, 8, 10, 10]
    assert col.elem_kinds.dtype == np.uint8 and col.elem_payload.dtype == np.uint64
    assert col.elem_kinds.tolist() == [KIND_STRING, KIND_STRING, KIND_NUMBER, KIND_BOOL, KIND_OTHER, KIND_OTHER, KIND_OTHER, KIND_NUMBER,
                                       KIND_STRING, KIND_BOOL]
    assert col.elem_payload.tolist() == [1, 0, f64(5.0), 1, 0, 0, 0, 1 << 63, 2, 0]
    assert col.exact and col.list_exact and col.encodable
    assert col.string_table("==", "y").tolist() == [0b010]                 # serves elements and scalars alike
    empty = MetaColumn("w")
    empty.extend([{"v": 1}, {}])
    assert empty.elem_off.tolist() == [0, 0, 0] and len(empty.elem_kinds) == 0 and len(empty.elem_payload) == 0
    assert MetaColumn("w").elem_off.tolist() == [0]


def test_a_column_extended_in_batches_equals_one_built_at_once():
    whole = columns_of(ROWS, ["tags", "authors"])
    for col, key in zip(whole, ["tags", "authors"]):
        pieces = MetaColumn(key)
        at = 0
        for step in (1, 0, 7, 64, 3, 900, len(ROWS)):
            pieces.extend(ROWS[at:at + step])
            at += step
            assert len(pieces.elem_off) == len(pieces) + 1 and pieces.elem_off[0] == 0 and (np.diff(pieces.elem_off) >= 0).all()
            assert pieces.elem_off[-1] == len(pieces.elem_kinds) == len(pieces.elem_payload)
        assert len(pieces) == len(col) == len(ROWS) and pieces.strings == col.strings
        for name in ("kinds", "payload", "elem_off", "elem_kinds", "elem_payload"):
            assert np.array_equal(getattr(pieces, name), getattr(col, name)), (key, name)
    two = MetaColumn("v")
    two.extend([{"v": ["a", 1]}, {"v": 2}])
    two.extend([{"v": [True]}, {"v": ["b", "a"]}])
    assert two.elem_off.tolist() == [0, 2, 2, 3, 5] and two.elem_payload.tolist() == [0, f64(1.0), 1, 1, 0] and two.strings == ["a", "b"]


@pytest.mark.parametrize("keep_of", [lambda n: np.ones(n, bool), lambda n: np.zeros(n, bool), lambda n: np.arange(n) % 2 == 0,
                                     lambda n: np.random.default_rng(3).random(n) < 0.3, lambda n: np.arange(n) < 11])
def test_compact_drops_the_rows_element_ranges_and_rebases_the_offsets(keep_of):
    rows = ROWS[:500]
    keep = keep_of(len(rows))
    col = MetaColumn("tags")
    col.extend(rows)
    col.compact(keep)
    fresh = MetaColumn("tags")
    fresh.extend([md for md, k in zip(rows, keep) if k])
    assert len(col) == int(keep.sum()) and col.elem_off[0] == 0 and col.elem_off.dtype == np.int64
    for name in ("kinds", "elem_off", "elem_kinds"):
        assert np.array_equal(getattr(col, name), getattr(fresh, name)), name
    # payloads through the dictionaries: compaction keeps the codes, a fresh column numbers the surviving strings anew
    decode = lambda c: [c.strings[int(p)] if k == KIND_STRING else int(p) for k, p in zip(c.elem_kinds, c.elem_payload)]   # noqa: E731
    assert decode(col) == decode(fresh)
    col.extend(rows[:40])                                                  # and it goes on growing behind the compacted rows
    assert len(col.elem_off) == len(col) + 1 and col.elem_off[-1] == len(col.elem_kinds)
    expr = 'json_contains(tags, "5") or json_contains(tags, 1.5)'
    kept_rows = [md for md, k in zip(rows, keep) if k] + rows[:40]
    assert np.array_equal(interpret(compile_filter(expr), [col]), expected(expr, kept_rows))


def test_what_cannot_be_represented_turns_the_flags():
    """`list_exact` is `exact` for elements: a NaN or an out-of-range int inside a list sends list filters on the key to the host;
    scalar comparisons never look inside a list, so `exact` stays (tests/test_filter_program_host.py pins that)."""
    col = MetaColumn("v")
    col.extend([{"v": [1.0, "nan"]}, {"v": float("inf")}, {"v": [float("inf")]}])
    assert col.exact and col.list_exact and col.encodable
    col.extend([{"v": [2.0, float("nan")]}])
    assert col.exact and not col.list_exact
    col.extend([{"v": [3.0]}])
    assert not col.list_exact and len(col) == 5 and col.elem_off.tolist() == [0, 2, 2, 3, 5, 6]
    big = MetaColumn("v")
    big.extend([{"v": [10 ** 400, 1]}])                                    # float(value) overflows: the closure raises for this row
    assert big.exact and not big.list_exact and big.elem_kinds.tolist() == [KIND_OTHER, KIND_NUMBER]
    scalar = MetaColumn("v")
    scalar.extend([{"v": float("nan")}, {"v": [1]}])
    assert not scalar.exact and scalar.list_exact
    lone = MetaColumn("v")
    lone.extend([{"v": ["ok", "Zürich"]}])
    assert lone.encodable
    lone.extend([{"v": ["bad \ud800"]}])                                   # a lone surrogate has no UTF-8 form: the dictionary is one
    assert not lone.encodable and lone.list_exact and lone.strings == ["ok", "Zürich", "bad \ud800"]


def test_the_restatement_itself():
    """`any_per_row` and `leaf_answers` on hand-made arrays: the GPU tests rest on them."""
    off = np.asarray([0, 0, 3, 3, 4], np.int64)
    assert any_per_row(off, np.asarray([False, True, False, False])).tolist() == [False, True, False, False]
    assert any_per_row(off, np.asarray([False, False, False, True])).tolist() == [False, False, False, True]
    assert any_per_row(np.zeros(3, np.int64), np.zeros(0, bool)).tolist() == [False, False]
    lf = compile_filter('a == "x"').leaves[0]
    kinds = np.asarray([KIND_STRING, KIND_STRING, KIND_STRING, KIND_NUMBER, KIND_BOOL, KIND_OTHER], np.uint8)
    payload = np.asarray([0, 1, 2, f64(0.0), 1, 0], np.uint64)
    assert leaf_answers(lf, ["y", "x", "x2"], kinds, payload).tolist() == [False, True, False, False, False, False]
    assert leaf_answers(lf, None, kinds, payload, table=[True]).tolist() == [True, False, False, False, False, False]   # codes beyond: 0


# ------------------------------------------------------------------------------------------ the store's host route
STORE_FILTERS = ['json_contains(metadata["authors"], "Adam Kovacs")', 'json_contains_all(tags, [5, "5"]) or json_contains(years, 1999)',
                 'not json_contains_any(authors, ["Ada", "Paul Schmitt"]) and source != "web"', "json_contains(flags, true) and score < 0.5"]


def _store(route, n=403, **kw):
    dense, sparse = _data(n=n)
    st = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_route=route, **kw)
    st.add_vectors([f"id{i}" for i in range(n)], dense.tolist(), sparse, [f"text {i}" for i in range(n)], [f"enh {i}" for i in range(n)],
                   ROWS[:n])
    return st, dense, sparse


def test_host_route_masks_queries_deletes_and_a_save_load(stand_ins, tmp_path):  # noqa: F811
    subset, dense, sparse = _store("subset")
    bitmap, _, _ = _store("bitmap")
    n = len(subset)
    for flt in STORE_FILTERS:
        want = expected(flt, ROWS[:n])
        assert want.any() and not want.all()
        for st in (subset, bitmap):
            assert np.array_equal(st._mask(flt), want), flt
        for kind, kw in (("dense", {"dense_query": dense[3].tolist()}), ("sparse", {"sparse_query": sparse[3]})):
            a = subset.query(top_k=7, search_type=kind, filter=flt, **kw)
            b = bitmap.query(top_k=7, search_type=kind, filter=flt, **kw)
            assert _dump([a]) == _dump([b]) and len(a) == 7
            assert all(want[int(r.id[2:])] for r in a)
            assert a[0].metadata == ROWS[int(a[0].id[2:])]                     # the lists come back with every hit
        everything = subset.query(top_k=n, filter=flt)                        # a filter-only query
        assert sorted(int(r.id[2:]) for r in everything) == np.nonzero(want)[0].tolist()
    flt = STORE_FILTERS[0]
    want = expected(flt, ROWS[:n])
    gone = [int(r) for r in np.nonzero(want)[0][:5]]
    subset.delete([f"id{r}" for r in gone])
    want[gone] = False
    assert np.array_equal(subset._mask(flt), want)
    subset.save(str(tmp_path / "store"))
    back = vs.GpuVectorStore.load(str(tmp_path / "store"))
    alive = [i for i in range(n) if i not in gone]
    for f in STORE_FILTERS:                                                   # tuples came back as lists: the same rows pass
        mask = back._mask(f)
        assert np.array_equal(mask if mask is not None else np.ones(len(alive), bool), expected(f, [ROWS[i] for i in alive])), f
