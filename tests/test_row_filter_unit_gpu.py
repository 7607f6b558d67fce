"""The row-filter kernel through `shards.RowFilter` (vrag_row_filter_*, csrc/rowfilter.hip): every answer is compared bit for bit
with the Python predicate of `parse_filter` (or, for hand-made leaves, with the leaf's stated meaning)."""
import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from filter_cases import KEYS, columns_of, expected, random_expressions, random_rows
from verbatim_rag_amd import _lib
from verbatim_rag_amd.shards import RowFilter, _bitmap, program_arrays
from verbatim_rag_amd.store_filter import compile_filter

pytestmark = pytest.mark.gpu

N = 4097
SENTINEL = 0xDEADBEEF
LEAF, AND, OR, NOT = 0, 1, 2, 3


def leaf(column, other=0, bools=0, num="never", bound=0.0, mode="never", off=0, codes=0):
    return _lib.FilterLeaf(bound=bound, table_off=off, table_codes=codes, column=column, num_op=_lib.FILTER_NUM_OPS[num],
                           str_mode=_lib.FILTER_STR_MODES[mode], bool_bits=bools, other_bit=other)


def push(i):
    return LEAF | (i << 8)


def upload(rf, rows, keys):
    """(device column, MetaColumn) per key, every row uploaded."""
    out = []
    for col in columns_of(rows, keys):
        at = rf.add_column()
        rf.append(at, col.kinds, col.payload)
        out.append((at, col))
    return out


def check(rf, expr, cols_by_key, rows, n_rows=None):
    n = len(rows) if n_rows is None else n_rows
    prog = compile_filter(expr)
    got = rf.eval_program(prog, [cols_by_key[k] for k in prog.keys], n)
    want = expected(expr, rows[:n])
    assert got.dtype == bool and np.array_equal(got, want), (expr, n, np.nonzero(got != want)[0][:8])
    return want


@pytest.fixture(scope="module")
def world():
    rows = random_rows(N, seed=23)
    rf = RowFilter()
    cols = dict(zip(KEYS, upload(rf, rows, KEYS)))
    yield rf, rows, cols
    rf.close()


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, N])
def test_row_counts_tail_bits_and_the_word_behind_the_output(world, n):
    rf, rows, cols = world
    expr = 'not (year >= 2020 and source != "web") or peer == true'
    prog = compile_filter(expr)
    leaves, ops, tables = program_arrays(prog, [cols[k] for k in prog.keys])
    n_words = (n + 31) // 32
    out = np.full(n_words + 1, SENTINEL, np.uint32)
    assert rf.eval(leaves, ops, tables, n, out=out) is out
    assert out[n_words] == SENTINEL                                    # nothing behind the words of n rows is written
    want = expected(expr, rows[:n])
    assert np.array_equal(out[:n_words], _bitmap(want)[:n_words])      # includes: bits at and beyond n are zero
    if n % 32:
        assert int(out[n_words - 1]) >> (n % 32) == 0
    assert n < N or (want.any() and not want.all())


def test_columns_appended_in_pieces_across_a_capacity_growth():
    rows = random_rows(329, seed=4)
    whole = columns_of(rows, ["year", "source"])
    with_growth = RowFilter()
    try:
        at = [with_growth.add_column() for _ in whole]
        done = 0
        for piece in (3, 61, 64, 1, 200):                              # 129 rows fit the first allocation (256), 329 do not
            for a, col in zip(at, whole):
                with_growth.append(a, col.kinds[done:done + piece], col.payload[done:done + piece])
            done += piece
            assert [with_growth.rows(a) for a in at] == [done, done]
            cols = {"year": (at[0], whole[0]), "source": (at[1], whole[1])}
            for n in sorted({done, done - 1, min(done, 64), 0}):       # the column's prefix only
                check(with_growth, 'year < 2020 or source >= "b"', cols, rows, n)
        with_growth.append(at[0], np.zeros(0, np.uint8), np.zeros(0, np.uint64))
        assert with_growth.rows(at[0]) == 329
        with pytest.raises(_lib.VragError) as err:
            with_growth.append(at[0], np.asarray([4], np.uint8), np.asarray([0], np.uint64))
        assert err.value.status == -1 and with_growth.rows(at[0]) == 329
    finally:
        with_growth.close()


VALUES = [float("-inf"), -1, -0.0, 0.0, 1, 1.5, 2020, 2020.0, float("inf"), 2 ** 53 + 1, "", "a", "b", "2020", "Zürich", True, False, None,
          [1], {"a": 1}]
LITERALS = ["-1e999", "-1", "0", "-0.0", "1.5", "2020", "2.02e3", "1e999", "9007199254740993", '""', '"a"', '"b"', '"2020"', '"Zürich"',
            "true", "false"]


def test_every_operator_against_every_kind_of_value():
    rows = [{"v": v} for v in VALUES] + [{}, {"w": 1}] + [{"v": v} for v in VALUES[::-1]] * 3
    rf = RowFilter()
    try:
        cols = dict(zip(["v"], upload(rf, rows, ["v"])))
        hits = 0
        for op in ("==", "!=", "<", "<=", ">", ">="):
            for lit in LITERALS:
                if op not in ("==", "!=") and lit in ("true", "false"):
                    continue
                hits += int(check(rf, f"v {op} {lit}", cols, rows).sum())
                check(rf, f'not metadata["v"] {op} {lit}', cols, rows)
        assert hits > 500
        missing = check(rf, 'v != "a"', cols, rows)                    # `!=` holds for missing keys, None, lists and dicts
        assert missing[len(VALUES)] and missing[len(VALUES) + 1] and missing[VALUES.index(None)] and missing[VALUES.index([1])]
        check(rf, 'v in [2020, "2020", true, -0.0]', cols, rows)
    finally:
        rf.close()


def test_every_number_op_and_every_per_kind_constant():
    """Hand-made leaves: each kind's answer is what the leaf states for that kind alone."""
    numbers = np.asarray([-np.inf, -1.0, -0.0, 0.0, 1.0, 2020.0, np.inf], np.float64)
    kinds = np.asarray([1] * 7 + [2, 2, 3, 3, 0], np.uint8)
    payload = np.concatenate([numbers.view(np.uint64), np.asarray([0, 1, 0, 1, 0], np.uint64)])
    reps = 70                                                          # > one wave: 840 rows
    rf = RowFilter()
    try:
        at = rf.add_column()
        rf.append(at, np.tile(kinds, reps), np.tile(payload, reps))
        py = {"never": lambda x, b: False, "always": lambda x, b: True, "==": lambda x, b: x == b, "!=": lambda x, b: x != b,
              "<": lambda x, b: x < b, "<=": lambda x, b: x <= b, ">": lambda x, b: x > b, ">=": lambda x, b: x >= b}
        table = np.asarray([0b10], np.uint32)                          # code 1 matches, code 0 does not
        for num in py:
            for bound in (0.0, -0.0, 2020.0, np.inf, -np.inf):
                for other in (0, 1):
                    for bools in (0, 1, 2, 3):
                        for mode in ("never", "always", "table"):
                            lf = leaf(at, other, bools, num, float(bound), mode, 0, 2 if mode == "table" else 0)
                            words = rf.eval([lf], [push(0)], table, len(kinds) * reps)
                            got = np.unpackbits(words.view(np.uint8), bitorder="little")[: len(kinds) * reps].astype(bool)
                            strs = {"never": [False, False], "always": [True, True], "table": [False, True]}[mode]
                            want = [py[num](float(x), float(bound)) for x in numbers] + strs + \
                                   [bool(bools & 1), bool(bools & 2), bool(other)]
                            assert np.array_equal(got, np.tile(np.asarray(want, dtype=bool), reps)), (num, bound, other, bools, mode)
    finally:
        rf.close()


@pytest.mark.parametrize("distinct", [1, 33, 100])
def test_string_tables_of_one_word_two_words_and_more(distinct):
    rows = [{"s": f"name{(i * 7) % distinct:03d}"} for i in range(300)] + [{"s": 5}, {}]
    rf = RowFilter()
    try:
        cols = dict(zip(["s"], upload(rf, rows, ["s"])))
        assert len(cols["s"][1].strings) == distinct
        for expr in ('s == "name000"', 's != "name000"', 's < "name020"', 's >= "name032"', 's > "name064"', 's <= "name099"',
                     's in ["name032", "name099", "nobody"]', 's > "name000" and not s >= "name070"'):
            check(rf, expr, cols, rows)
    finally:
        rf.close()


def test_a_table_shorter_than_the_largest_code_matches_nothing_beyond_itself():
    codes = np.arange(100, dtype=np.uint64)
    rf = RowFilter()
    try:
        at = rf.add_column()
        rf.append(at, np.full(100, 2, np.uint8), codes)
        tables = np.full(3, 0xFFFFFFFF, np.uint32)                     # every bit set, also behind the leaf's 40 codes
        for off, n_codes in ((0, 40), (1, 40), (2, 32), (3, 0), (0, 1), (0, 96)):
            words = rf.eval([leaf(at, mode="table", off=off, codes=n_codes)], [push(0)], tables, 100)
            got = np.unpackbits(words.view(np.uint8), bitorder="little")[:100].astype(bool)
            assert np.array_equal(got, codes < n_codes), (off, n_codes)
    finally:
        rf.close()


def test_a_program_of_64_leaves_and_one_at_stack_depth_32():
    rows = [{"a": i % 90, "b": i % 7} for i in range(700)]
    rf = RowFilter()
    try:
        cols = dict(zip(["a", "b"], upload(rf, rows, ["a", "b"])))
        sixty_four = " or ".join(f"a == {2 * i}" for i in range(64))
        assert len(compile_filter(sixty_four).leaves) == 64
        check(rf, sixty_four, cols, rows)
        check(rf, "a in [" + ", ".join(str(3 * i) for i in range(64)) + "]", cols, rows)

        def nested(depth):
            return "b != 3" if depth == 1 else f"a != {depth} and ({nested(depth - 1)})"

        assert compile_filter(nested(32)).depth() == 32
        want = check(rf, nested(32), cols, rows)
        assert want.any() and not want.all()

        def nested_or(depth):                                          # the bottom of a full stack decides
            return "b == 3" if depth == 1 else f"({nested_or(depth - 1)}) or a == {depth}" if depth % 2 else \
                f"a == {depth} or ({nested_or(depth - 1)})"

        check(rf, nested_or(32), cols, rows)
        deep = "a < 80 and (" * 31 + "b == 2" + ")" * 31
        assert compile_filter(deep).depth() == 32
        check(rf, deep, cols, rows)
    finally:
        rf.close()


def test_two_columns_of_different_lengths():
    rows = [{"a": i, "b": i % 5} for i in range(200)]
    rf = RowFilter()
    try:
        (ca, ma), = upload(rf, rows, ["a"])
        (cb, mb), = upload(rf, rows[:130], ["b"])
        cols = {"a": (ca, ma), "b": (cb, mb)}
        check(rf, "a >= 64 and b != 2", cols, rows, 130)
        check(rf, "a >= 64", cols, rows, 200)
        out = np.full(8, SENTINEL, np.uint32)
        prog = compile_filter("a >= 64 and b != 2")
        with pytest.raises(_lib.VragError, match="holds 130 rows") as err:
            rf.eval(*program_arrays(prog, [cols[k] for k in prog.keys]), 131, out=out)
        assert err.value.status == -1 and (out == SENTINEL).all()
    finally:
        rf.close()


def test_validation_errors_leave_the_output_alone(world):
    rf, rows, cols = world
    year, source = cols["year"][0], cols["source"][0]
    ok_leaf = leaf(year, num=">=", bound=2020.0)
    table = np.zeros(2, np.uint32)
    bad = {
        "leaf index": ([ok_leaf], [push(1)], table, 64),
        "leaf column": ([leaf(99, num="<")], [push(0)], table, 64),
        "negative column": ([leaf(-1, num="<")], [push(0)], table, 64),
        "table range": ([leaf(source, mode="table", off=1, codes=33)], [push(0)], table, 64),
        "table offset": ([leaf(source, mode="table", off=3, codes=0)], [push(0)], table, 64),
        "negative table": ([leaf(source, mode="table", off=-1, codes=1)], [push(0)], table, 64),
        "underflow and": ([ok_leaf], [push(0), AND], table, 64),
        "underflow not": ([ok_leaf], [NOT, push(0)], table, 64),
        "two values left": ([ok_leaf], [push(0), push(0)], table, 64),
        "depth 33": ([ok_leaf], [push(0)] * 33 + [AND] * 32, table, 64),
        "unknown op": ([ok_leaf], [push(0), 7], table, 64),
        "rows beyond a column": ([ok_leaf], [push(0)], table, N + 1),
        "65 leaves": ([ok_leaf] * 65, [push(0)], table, 64),
        "257 ops": ([ok_leaf], [push(0)] + [NOT] * 256, table, 64),
        "bad field": ([leaf(year, bools=4)], [push(0)], table, 64),
    }
    extra = RowFilter()
    try:
        for _ in range(17):
            extra.append(extra.add_column(), np.zeros(64, np.uint8), np.zeros(64, np.uint64))
        out = np.full(160, SENTINEL, np.uint32)
        bad["17 columns"] = ([leaf(c, num="<") for c in range(17)], [push(0)], table, 64)
        for name, (leaves, ops, tables, n) in bad.items():
            with pytest.raises(_lib.VragError) as err:
                (extra if name == "17 columns" else rf).eval(leaves, np.asarray(ops, np.uint32), tables, n, out=out)
            assert err.value.status == -1 and "vrag_row_filter_eval" in str(err.value), name
            assert (out == SENTINEL).all(), name
        # sixteen columns, depth 32 and 256 ops are inside the limits
        sixteen = extra.eval([leaf(c, other=1) for c in range(16)], [push(i) for i in range(16)] + [AND] * 15, table, 64)
        assert sixteen.tolist() == [0xFFFFFFFF, 0xFFFFFFFF]
        assert rf.eval([ok_leaf], [push(0)] * 32 + [OR] * 31, table, 64).tolist() == rf.eval([ok_leaf], [push(0)], table, 64).tolist()
        assert rf.eval([ok_leaf], [push(0)] + [NOT] * 255, table, 64).tolist() == \
            [int(w) ^ 0xFFFFFFFF for w in rf.eval([ok_leaf], [push(0)], table, 64)]
    finally:
        extra.close()
    assert rf.eval([ok_leaf], [push(0)], table, 0).tolist() == []        # no rows: OK, nothing launched


def test_random_expressions_are_exact_on_the_device(world):
    rf, rows, cols = world
    split = 0
    for expr in random_expressions(300, seed=5):
        want = check(rf, expr, cols, rows)
        split += int(want.any() and not want.all())
    assert split > 100
