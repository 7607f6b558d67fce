"""The list-filter kernel at the C ABI (vrag_row_filter_append_lists / _list_rows / _eval_lists, csrc/listfilter.hip) through
`shards.RowFilter`: every answer is compared bit for bit with the numpy restatement of the program over the typed list columns
(tests/list_filter_cases.py) and, where an expression stands behind it, with the Python predicate of `parse_filter`."""
import ctypes as C

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from list_filter_cases import EXPRESSIONS, KEYS, any_per_row, columns_of, expected, interpret, leaf_answers, list_rows
from verbatim_rag_amd import _lib
from verbatim_rag_amd.shards import RowFilter, _bitmap, _vp, program_arrays
from verbatim_rag_amd.store_columns import MetaColumn
from verbatim_rag_amd.store_filter import compile_filter

pytestmark = pytest.mark.gpu

N = 1000
SENTINEL = 0xDEADBEEF
LEAF, AND, OR, NOT, LIST_ANY = 0, 1, 2, 3, 4
ROWS = list_rows(N, seed=7)


def leaf(column, other=0, bools=0, num="never", bound=0.0, mode="never", off=0, codes=0):
    return _lib.FilterLeaf(bound=bound, table_off=off, table_codes=codes, column=column, num_op=_lib.FILTER_NUM_OPS[num],
                           str_mode=_lib.FILTER_STR_MODES[mode], bool_bits=bools, other_bit=other)


def push(i):
    return LEAF | (i << 8)


def any_of(i):
    return LIST_ANY | (i << 8)


def bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def append_lists(rf, at, col, first=0, last=None):
    """Rows [first, last) of the MetaColumn's list part, offsets from 0 as the ABI takes them."""
    last = len(col) if last is None else last
    off = col.elem_off[first:last + 1]
    rf.append_lists(at, off - off[0], col.elem_kinds[off[0]:off[-1]], col.elem_payload[off[0]:off[-1]])


def upload(rf, rows, keys, scalars=True, lists=True):
    """(device column, MetaColumn) per key."""
    out = []
    for col in columns_of(rows, keys):
        at = rf.add_column()
        if scalars:
            rf.append(at, col.kinds, col.payload)
        if lists:
            append_lists(rf, at, col)
        out.append((at, col))
    return out


def check(rf, expr, cols_by_key, rows, n_rows=None, strings="host"):
    n = len(rows) if n_rows is None else n_rows
    prog = compile_filter(expr)
    got = rf.eval_program(prog, [cols_by_key[k] for k in prog.keys], n, strings=strings)
    restated = interpret(prog, [cols_by_key[k][1] for k in prog.keys], n)
    want = expected(expr, rows[:n])
    assert np.array_equal(restated, want), expr
    assert got.dtype == bool and np.array_equal(got, want), (expr, n, np.nonzero(got != want)[0][:8])
    return want


@pytest.fixture(scope="module")
def world():
    rf = RowFilter()
    cols = dict(zip(KEYS, upload(rf, ROWS, KEYS)))
    yield rf, cols
    rf.close()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, N])
def test_row_counts_tail_bits_and_the_word_behind_the_output(world, n):
    rf, cols = world
    expr = 'not (json_contains(tags, 5) and source != "web") or json_contains_any(authors, ["Ada", "Zoë Ölmez"])'
    prog = compile_filter(expr)
    leaves, ops, tables = program_arrays(prog, [cols[k] for k in prog.keys])
    assert (ops & 0xFF == LIST_ANY).sum() == 3
    n_words = (n + 31) // 32
    out = np.full(n_words + 1, SENTINEL, np.uint32)
    assert rf.eval(leaves, ops, tables, n, out=out) is out
    assert out[n_words] == SENTINEL                                    # nothing behind the words of n rows is written
    want = expected(expr, ROWS[:n])
    assert np.array_equal(interpret(prog, [cols[k][1] for k in prog.keys], n), want)
    assert np.array_equal(out[:n_words], _bitmap(want)[:n_words])      # includes: bits at and beyond n are zero
    if n % 32:
        assert int(out[n_words - 1]) >> (n % 32) == 0
    assert n < 255 or (want.any() and not want.all())


@pytest.mark.parametrize("expr", EXPRESSIONS)
def test_every_expression_of_the_host_test(world, expr):
    rf, cols = world
    want = check(rf, expr, cols, ROWS)
    assert want.any() and not want.all()


def test_no_rows_is_ok_without_a_launch(world):
    rf, cols = world
    at = cols["tags"][0]
    assert rf.eval([leaf(at, num="==", bound=5.0)], [any_of(0)], np.zeros(0, np.uint32), 0).tolist() == []


LENGTHS = (0, 1, 2, 63, 64, 65, 5000)


def test_list_lengths_around_a_wave_and_one_of_5000_elements():
    rows = [{"a": list(range(length))} for length in LENGTHS] * 20 + [{"a": [4999.0]}, {"a": 3}, {}]     # 143 rows: three waves
    rf = RowFilter()
    try:
        cols = dict(zip(["a"], upload(rf, rows, ["a"], scalars=False)))
        assert rf.list_rows(cols["a"][0]) == (len(rows), 20 * sum(LENGTHS) + 1) and rf.rows(cols["a"][0]) == 0
        for value, lists in ((0, 120), (1, 100), (62, 80), (63, 60), (64, 40), (65, 20), (4999, 21), (5000, 0), (-1, 0)):
            want = check(rf, f"json_contains(a, {value})", cols, rows)
            assert int(want.sum()) == lists
            check(rf, f"not json_contains(a, {value})", cols, rows)
        check(rf, "json_contains_all(a, [0, 64, 4999]) or json_contains_any(a, [-1, 1])", cols, rows)
    finally:
        rf.close()


def test_a_shard_where_no_row_holds_a_list():
    rows = [{"a": v} for v in (5, "5", True, None, {"0": 5})] * 30 + [{}] * 3
    rf = RowFilter()
    try:
        cols = dict(zip(["a"], upload(rf, rows, ["a"])))
        assert rf.list_rows(cols["a"][0]) == (len(rows), 0)
        for expr in ("json_contains(a, 5)", 'json_contains(a, "5")', "json_contains(a, true)"):
            assert not check(rf, expr, cols, rows).any()
            assert check(rf, f"not {expr}", cols, rows).all()
        want = check(rf, "json_contains(a, 5) or a == 5", cols, rows)
        assert int(want.sum()) == 30
    finally:
        rf.close()


def test_lists_appended_in_pieces_continue_the_offsets_across_a_capacity_growth():
    rows = ROWS[:329]
    whole = columns_of(rows, ["tags", "authors"])
    rf = RowFilter()
    try:
        at = [rf.add_column() for _ in whole]
        done = 0
        for piece in (3, 61, 64, 1, 200):                              # 256 offsets / elements fit the first allocation, 329 rows do not
            for a, col in zip(at, whole):
                append_lists(rf, a, col, done, done + piece)
            done += piece
            assert [rf.list_rows(a) for a in at] == [(done, int(col.elem_off[done])) for col in whole]
            cols = {"tags": (at[0], whole[0]), "authors": (at[1], whole[1])}
            for n in sorted({done, done - 1, min(done, 64)}):          # the list part's prefix only
                check(rf, 'json_contains(tags, "5") or json_contains_all(authors, ["Ada", "5"])', cols, rows, n)
        rf.append_lists(at[0], np.zeros(1, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.uint64))     # no rows: nothing changes
        assert rf.list_rows(at[0]) == (329, int(whole[0].elem_off[329]))
    finally:
        rf.close()


# ------------------------------------------------------------------------------------------ hand-made leaves
def handmade():
    """One column, 70 rows x 3: strings "s0" .. "s39" as codes, numbers, bools and others as elements."""
    col = MetaColumn("v")
    col.extend([{"v": [f"s{(i * 7) % 40}", float(i % 5), bool(i % 2), None, f"s{i % 40}"][: i % 6]} for i in range(210)])
    return col


def test_number_bool_and_string_leaves_per_element():
    col = handmade()
    rf = RowFilter()
    try:
        at = rf.add_column()
        append_lists(rf, at, col)
        n = len(col)
        table_bits = np.asarray([c % 3 == 0 for c in range(len(col.strings))], dtype=bool)
        table = _bitmap(table_bits)
        cases = {
            "number ==": (leaf(at, num="==", bound=3.0), dict(other=False, bools=(False, False), num_op="==", bound=3.0, str_op="never")),
            "number <": (leaf(at, num="<", bound=1.0), dict(other=False, bools=(False, False), num_op="<", bound=1.0, str_op="never")),
            "bool true": (leaf(at, bools=2), dict(other=False, bools=(False, True), num_op="never", bound=0.0, str_op="never")),
            "bool false": (leaf(at, bools=1), dict(other=False, bools=(True, False), num_op="never", bound=0.0, str_op="never")),
            "other": (leaf(at, other=1), dict(other=True, bools=(False, False), num_op="never", bound=0.0, str_op="never")),
            "string always": (leaf(at, mode="always"), dict(other=False, bools=(False, False), num_op="never", bound=0.0, str_op="always")),
            "string table": (leaf(at, mode="table", off=0, codes=len(table_bits)),
                             dict(other=False, bools=(False, False), num_op="never", bound=0.0, str_op="table")),
            "a table shorter than the dictionary": (leaf(at, mode="table", off=0, codes=7),
                                                    dict(other=False, bools=(False, False), num_op="never", bound=0.0, str_op="short")),
        }
        from types import SimpleNamespace
        for name, (lf, meaning) in cases.items():
            words = rf.eval([lf], [any_of(0)], table, n)
            tbl = {"table": table_bits, "short": table_bits[:7]}.get(meaning["str_op"])
            answers = leaf_answers(SimpleNamespace(**meaning), col.strings, col.elem_kinds, col.elem_payload, table=tbl)
            want = any_per_row(col.elem_off, answers)
            assert np.array_equal(bits(words, n), want), name
            assert want.any() and not want.all(), name
            flipped = rf.eval([lf], [any_of(0), NOT], table, n)
            assert np.array_equal(bits(flipped, n), ~want), name
        # every bit of the table words set, also behind the leaf's 7 codes: codes at or beyond table_codes still answer 0
        full = np.full(len(table), 0xFFFFFFFF, np.uint32)
        words = rf.eval([leaf(at, mode="table", off=0, codes=7)], [any_of(0)], full, n)
        is_str = col.elem_kinds == 2
        want = any_per_row(col.elem_off, is_str & (col.elem_payload < 7))
        assert np.array_equal(bits(words, n), want) and want.any() and not want.all()
    finally:
        rf.close()


def test_a_string_absent_from_the_dictionary_and_tables_made_by_the_match_kernel():
    rf = RowFilter()
    try:
        cols = dict(zip(["authors", "tags"], upload(rf, ROWS, ["authors", "tags"])))
        assert not check(rf, 'json_contains(authors, "nobody at all")', cols, ROWS).any()
        assert check(rf, 'not json_contains(authors, "nobody at all")', cols, ROWS).all()
        # filter_strings="device": the leaf's table is written by a VRAG_FILTER_MATCH_EQ launch over the dictionary in HBM
        for expr in ('json_contains(authors, "Adam Kovacs")', 'json_contains(authors, "nobody at all")',
                     'json_contains_any(authors, ["Zoë Ölmez", "日本 太郎", ""]) and not json_contains(tags, "medical-nlp")'):
            check(rf, expr, cols, ROWS, strings="device")
        prog = compile_filter('json_contains(authors, "Ada")')
        leaves, ops, tables, matches, texts = program_arrays(prog, [cols["authors"]], device_strings=True)
        assert len(matches) == 1 and matches[0].op == _lib.FILTER_MATCH_OPS["=="] and texts == b"Ada" and not tables.any()
        words = rf.eval(leaves, ops, tables, N, matches=matches, texts=texts)
        assert np.array_equal(bits(words, N), expected('json_contains(authors, "Ada")', ROWS))
        assert rf.strings(cols["authors"][0])[0] == len(cols["authors"][1].strings)
    finally:
        rf.close()


def test_a_program_at_stack_depth_32_and_one_of_64_list_leaves(world):
    rf, cols = world

    def nested(depth):
        return 'json_contains(flags, true)' if depth == 1 else f"not json_contains(years, {1990 + depth}) and ({nested(depth - 1)})"

    assert compile_filter(nested(32)).depth() == 32
    want = check(rf, nested(32), cols, ROWS)
    assert want.any() and not want.all()
    deep = "score < 0.9 and (" * 31 + "json_contains(tags, 5)" + ")" * 31
    assert compile_filter(deep).depth() == 32
    check(rf, deep, cols, ROWS)
    sixty_four = "json_contains_any(years, [" + ", ".join(str(1990 + i) for i in range(64)) + "])"
    assert len(compile_filter(sixty_four).leaves) == 64
    check(rf, sixty_four, cols, ROWS)
    at = cols["tags"][0]
    lf = leaf(at, num="==", bound=5.0)
    one = rf.eval([lf], [any_of(0)], np.zeros(0, np.uint32), N)
    assert rf.eval([lf], [any_of(0)] * 32 + [OR] * 31, np.zeros(0, np.uint32), N).tolist() == one.tolist()
    assert rf.eval([lf], [any_of(0), push(0), OR, any_of(0), AND], np.zeros(0, np.uint32), N).tolist() == \
        _bitmap(expected("(json_contains(tags, 5) or tags == 5) and json_contains(tags, 5)", ROWS)).tolist()


# ------------------------------------------------------------------------------------------ refusals
def test_append_lists_refusals_change_nothing():
    rf = RowFilter()
    try:
        at = rf.add_column()
        rf.append_lists(at, np.asarray([0, 2, 2], np.int64), np.asarray([1, 2], np.uint8), np.asarray([0, 0], np.uint64))
        k, p = np.asarray([1, 2, 3], np.uint8), np.zeros(3, np.uint64)
        for name, (off, kinds) in {"not from 0": ([1, 2, 3], k), "decreasing": ([0, 2, 1, 3], k), "negative": ([0, -1, 3], k),
                                   "kind 4": ([0, 3], np.asarray([1, 4, 0], np.uint8))}.items():
            with pytest.raises(_lib.VragError) as err:
                rf.append_lists(at, np.asarray(off, np.int64), kinds, p)
            assert err.value.status == -1 and "vrag_row_filter_append_lists" in str(err.value), name
            assert rf.list_rows(at) == (2, 2), name
        with pytest.raises(_lib.VragError) as err:
            rf.append_lists(at + 1, np.asarray([0, 0], np.int64), k[:0], p[:0])
        assert err.value.status == -1
        with pytest.raises(_lib.VragError):
            rf.list_rows(at + 1)
    finally:
        rf.close()


def test_eval_refusals_leave_the_output_alone(world):
    rf, cols = world
    tags, source = cols["tags"][0], cols["source"][0]
    ok = leaf(tags, num="==", bound=5.0)
    table = np.zeros(2, np.uint32)
    short = RowFilter()
    try:
        (sc, smeta), = upload(short, ROWS[:130], ["tags"], scalars=False)
        out = np.full(160, SENTINEL, np.uint32)
        bad = {
            "list rows beyond the list part": (short, [leaf(sc, num="==", bound=5.0)], [any_of(0)], table, 131),
            "a list leaf on a column without a list part": (short, [leaf(short.add_column(), num="==")], [any_of(0)], table, 1),
            "leaf index": (rf, [ok], [any_of(1)], table, 64),
            "leaf column": (rf, [leaf(99, num="<")], [any_of(0)], table, 64),
            "table range": (rf, [leaf(source, mode="table", off=1, codes=33)], [any_of(0)], table, 64),
            "underflow and": (rf, [ok], [any_of(0), AND], table, 64),
            "underflow not": (rf, [ok], [NOT, any_of(0)], table, 64),
            "two values left": (rf, [ok], [any_of(0), push(0)], table, 64),
            "depth 33": (rf, [ok], [any_of(0)] * 33 + [AND] * 32, table, 64),
            "unknown op": (rf, [ok], [any_of(0), 7], table, 64),
            "unknown op 5": (rf, [ok], [any_of(0), 5 | (0 << 8), OR], table, 64),
            "an operand on a binary op": (rf, [ok], [any_of(0), any_of(0), OR | (1 << 8)], table, 64),
            "rows beyond a column": (rf, [ok], [any_of(0), push(0), OR], table, N + 1),
            "65 leaves": (rf, [ok] * 65, [any_of(0)], table, 64),
            "257 ops": (rf, [ok], [any_of(0)] + [NOT] * 256, table, 64),
            "bad field": (rf, [leaf(tags, bools=4)], [any_of(0)], table, 64),
        }
        for name, (handle, leaves, ops, tables, n) in bad.items():
            with pytest.raises(_lib.VragError) as err:
                handle.eval(leaves, np.asarray(ops, np.uint32), tables, n, out=out)
            assert err.value.status == -1 and "vrag_row_filter_eval_lists" in str(err.value), name
            assert (out == SENTINEL).all(), name
        # a column with a list part alone serves a list leaf; a LEAF push of the same leaf needs the rows it does not hold
        assert short.eval([leaf(sc, num="==", bound=5.0)], [any_of(0)], table, 130).tolist() == \
            _bitmap(expected("json_contains(tags, 5)", ROWS[:130])).tolist()
        with pytest.raises(_lib.VragError, match="holds 0 rows"):
            short.eval([leaf(sc, num="==", bound=5.0)], [any_of(0), push(0), OR], table, 130, out=out)
        assert (out == SENTINEL).all()
        # vrag_row_filter_eval and _eval_matched keep refusing op 4
        lib = _lib.load()
        arr = (_lib.FilterLeaf * 1)(ok)
        ops = np.asarray([any_of(0)], np.uint32)
        assert lib.vrag_row_filter_eval(rf._h, arr, 1, _vp(ops), 1, None, 0, 64, _vp(out), None) == -1
        assert "vrag_row_filter_eval:" in _lib.last_error() and "no operation" in _lib.last_error()
        assert lib.vrag_row_filter_eval_matched(rf._h, arr, 1, _vp(ops), 1, None, 0, None, 0, None, 0, 64, _vp(out), None) == -1
        assert "vrag_row_filter_eval_matched:" in _lib.last_error() and (out == SENTINEL).all()
        # and without a list op eval_lists is eval_matched
        plain = np.asarray([push(0)], np.uint32)
        a, b = np.zeros(2, np.uint32), np.zeros(2, np.uint32)
        empty = (_lib.FilterMatch * 1)()
        assert lib.vrag_row_filter_eval_lists(rf._h, arr, 1, _vp(plain), 1, None, 0, empty, 0, None, 0, 64, _vp(a), None) == 0
        assert lib.vrag_row_filter_eval_matched(rf._h, arr, 1, _vp(plain), 1, None, 0, empty, 0, None, 0, 64, _vp(b), None) == 0
        assert a.tolist() == b.tolist() == _bitmap(expected("tags == 5", ROWS[:64])).tolist()
    finally:
        short.close()


# ------------------------------------------------------------------------------------------ compaction
def test_a_bitmap_shorter_than_the_list_part_is_refused_and_changes_nothing():
    """A keep-bitmap that covers only a prefix of what a column holds is VRAG_ERR_INVALID, for a list part as for the rows."""
    rows = ROWS[:200]
    rf = RowFilter()
    try:
        (at, col), = upload(rf, rows, ["tags"], scalars=False)                      # a list part alone
        with pytest.raises(_lib.VragError, match="the bitmap covers 150 rows, a column holds 200") as err:
            rf.compact(np.arange(150) % 2 == 0)
        assert err.value.status == -1 and rf.list_rows(at) == (200, int(col.elem_off[-1]))
        check(rf, "json_contains(tags, 5)", {"tags": (at, col)}, rows)
    finally:
        rf.close()


KEEPS = {"all": lambda n: np.ones(n, bool), "none": lambda n: np.zeros(n, bool), "alternating": lambda n: np.arange(n) % 2 == 0,
         "random": lambda n: np.random.default_rng(5).random(n) < 0.4}


@pytest.mark.parametrize("which", list(KEEPS) + ["a column shorter than the bitmap"])
def test_compact_then_a_list_filter_on_the_kept_rows(which):
    """The chosen design: a compaction that drops a row drops the list parts; they are appended again from the compacted host
    column, and the filter then answers for the renumbered rows."""
    rows = ROWS[:500]
    held = 300 if which == "a column shorter than the bitmap" else len(rows)       # rows the device holds of the 500 the bitmap covers
    keep = (np.arange(len(rows)) % 3 != 0) if held < len(rows) else KEEPS[which](len(rows))
    rf = RowFilter()
    try:
        cols = dict(zip(["tags", "source"], upload(rf, rows[:held], ["tags", "source"])))
        expr = 'json_contains_any(tags, [5, "x"]) and source != "web" or json_contains(tags, false)'
        check(rf, expr, cols, rows[:held])
        before = rf.list_rows(cols["tags"][0])
        assert before == (held, int(cols["tags"][1].elem_off[-1]))
        rf.compact(keep)
        kept = [md for md, k in zip(rows[:held], keep) if k]
        for at, col in cols.values():
            col.compact(keep[:held])
            assert rf.rows(at) == len(kept) == len(col)
            if which == "all":
                assert rf.list_rows(at) == (held, int(col.elem_off[-1]))             # nothing dropped: the list part stays
            else:
                assert rf.list_rows(at) == (0, 0)
                append_lists(rf, at, col)
            assert rf.list_rows(at) == (len(kept), int(col.elem_off[-1]))
        if kept:
            want = check(rf, expr, cols, kept)
            assert which == "none" or (want.any() and not want.all())
        more = rows[held - 50:held]                                                  # and the column goes on growing
        for at, col in cols.values():
            col.extend(more)
            rf.append(at, col.kinds[len(kept):], col.payload[len(kept):])
            append_lists(rf, at, col, len(kept))
        check(rf, expr, cols, kept + more)
    finally:
        rf.close()
