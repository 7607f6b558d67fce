"""The string-match kernel through `shards.RowFilter` (vrag_row_filter_append_strings / _match / _eval_matched, csrc/strmatch.hip):
every table is compared bit for bit with the reference matcher of tests/like_cases.py (LIKE) or Python's own string operators
(the six comparisons).

What runs where: a text beyond the kernel's limits (VRAG_FILTER_MATCH_MAX_PATTERN = 256 bytes) is refused by the library, and
`RowFilter.match(column=...)` / `eval_program(strings="device")` answer it with the host table.  Of the fixture that is the two
300-byte patterns and the 300-byte comparison text; `test_texts_over_the_limit_...` pins which, so every other case below is the
kernel's own answer."""
import operator
import random

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from filter_cases import expected
from like_cases import COMPARE_OPS, COMPARE_TEXTS, PAT, STR, dictionary, like_ref, table_bits
from verbatim_rag_amd import _lib
from verbatim_rag_amd.shards import RowFilter, match_on_device, program_arrays
from verbatim_rag_amd.store_columns import MetaColumn
from verbatim_rag_amd.store_filter import compile_filter

pytestmark = pytest.mark.gpu

N = 4097
SENTINEL = 0xDEADBEEF
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 129, N]
PY = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
CASES = [("like", p) for p in PAT] + [(op, t) for op in COMPARE_OPS for t in COMPARE_TEXTS]


def answers(op, text, strings):
    return [like_ref(s, text) if op == "like" else bool(PY[op](s, text)) for s in strings]


def column_of(strings, key="t"):
    col = MetaColumn(key)
    col.extend([{key: s} for s in strings])
    assert col.strings == list(strings)
    return col


@pytest.fixture(scope="module")
def world():
    """The dictionary of N strings on the device, and the reference answers of every case over it (computed once)."""
    strings = dictionary(N)
    assert len(set(strings)) == N
    col = column_of(strings)
    rf = RowFilter()
    at = rf.add_column()
    rf.append_strings(at, *col.string_bytes())
    want = {case: np.asarray(answers(*case, strings), dtype=bool) for case in CASES}
    yield rf, at, col, want
    rf.close()


def test_texts_over_the_limit_are_the_only_ones_the_host_answers(world):
    rf, at, _col, _want = world
    over = [case for case in CASES if match_on_device(*case) is not None]
    assert sorted(over) == sorted([("like", "%" + "x" * 300), ("like", "x" * 299 + "_")] + [(op, "x" * 300) for op in COMPARE_OPS])
    out = np.full(4, SENTINEL, np.uint32)
    for op, text in over:
        with pytest.raises(_lib.VragError, match="bytes") as err:
            rf.match(at, op, text, 64, out=out)
        assert err.value.status == -1 and (out == SENTINEL).all()


@pytest.mark.parametrize("n", SIZES)
def test_every_pattern_and_comparison_at_every_dictionary_size(world, n):
    rf, at, col, want = world
    n_words = (n + 31) // 32
    out = np.full(n_words + 1, SENTINEL, np.uint32)
    for case in CASES:
        out[:] = SENTINEL
        assert rf.match(at, *case, n, out=out, column=col) is out       # a prefix of the column's dictionary when n < N
        assert out[n_words] == SENTINEL, case                           # nothing behind the words of n codes is written
        assert np.array_equal(out[:n_words], table_bits(want[case][:n])[:n_words]), (case, n)   # includes: tail bits zero
        if n % 32:
            assert int(out[n_words - 1]) >> (n % 32) == 0
    if n == N:
        for case in CASES:
            hits = int(want[case].sum())
            assert (hits == N) == (case in (("like", "%"), ("like", "%%"), (">=", ""))), case
            assert (hits == 0) == (case in (("like", "%  %"), ("like", "Z__rich"), ("<", ""))), case


def test_a_dictionary_appended_in_pieces_across_a_capacity_growth():
    strings = dictionary(329)
    col = column_of(strings)
    data, off = col.string_bytes()
    assert off[-1] > 4096 and len(off) > 257                            # both first allocations (4096 bytes, 257 offsets) are outgrown
    rf = RowFilter()
    try:
        at = rf.add_column()
        assert rf.strings(at) == (0, 0)
        done = 0
        for piece in (3, 61, 64, 1, 200):
            part = MetaColumn("t")
            part.extend([{"t": s} for s in strings[done:done + piece]])
            rf.append_strings(at, *part.string_bytes())
            done += piece
            assert rf.strings(at) == (done, int(off[done]))
            newest = next(s for s in reversed(strings[:done]) if len(s) < 40)          # the last short string that arrived
            for case in (("like", "%ab%"), ("like", "_%#_"), ("like", "%語%"), ("<", "b"), ("==", newest)):
                for n in sorted({done, done - 1, min(done, 64)}):
                    got = rf.match(at, *case, n)
                    assert np.array_equal(got, table_bits(answers(*case, strings[:n]))), (case, n, done)
        assert done == 329 and rf.strings(at) == (329, len(data))
        rf.append_strings(at, np.zeros(0, np.uint8), np.zeros(1, np.int64))
        assert rf.strings(at) == (329, len(data))
        assert np.array_equal(rf.match(at, "like", "%"), table_bits([True] * 329))      # n_codes defaults to the whole dictionary
    finally:
        rf.close()


def test_one_very_long_string_among_short_ones():
    long = "start" + "ab" * 17500 + "MIDDLE" + "é日" * 7000 + "x" * 5 + "the end"
    assert len(long.encode()) >= 70000
    strings = ["a", "start", long, "the end", "MIDDLE", "é日", ""] + [f"s{i}" for i in range(70)]
    rf = RowFilter()
    try:
        at = rf.add_column()
        rf.append_strings(at, *column_of(strings).string_bytes())
        for p in ("start%", "%MIDDLE%", "%the end", "start%MIDDLE%the end", "%日xxxxx%", "%é日x_xxx%end", "_tart%", "%en_", "%MIDDLE",
                  "start", "%ab%ab%MIDDLE%é日%é日%x%", "%ba_%", "%MIDDLEab%"):
            want = answers("like", p, strings)
            assert np.array_equal(rf.match(at, "like", p), table_bits(want)), p
            assert want[2] == (p != "%MIDDLE" and p != "start" and p != "%MIDDLEab%"), p
        for op in COMPARE_OPS:
            for t in ("start", "startab", "startb", long[:200], "the end"):
                assert np.array_equal(rf.match(at, op, t), table_bits(answers(op, t, strings))), (op, t[:20])
    finally:
        rf.close()


def test_validation_errors_leave_the_outputs_and_the_handle_alone(world):
    rf, at, col, want = world
    empty = rf.add_column()                                             # a column without a dictionary
    lib, h = rf._lib, rf._h
    out = np.full(160, SENTINEL, np.uint32)
    outp = out.ctypes.data_as(_lib.C.c_void_p)

    def refused(name, status):
        assert status == -1 and name in _lib.last_error(), (name, status, _lib.last_error())
        assert (out == SENTINEL).all(), name

    def match(text, op=6, n=64, column=at):
        return lib.vrag_row_filter_match(h, column, op, text, len(text), n, outp, None)

    refused("vrag_row_filter_match", match(b"a%", n=N + 1))                         # more codes than the dictionary holds
    refused("vrag_row_filter_match", match(b"a%", column=empty, n=1))
    refused("vrag_row_filter_match", match(b"a%", column=99))
    refused("vrag_row_filter_match", match(b"x" * 257))                             # the text limit
    refused("vrag_row_filter_match", match(b"x" * 257, op=0))
    refused("vrag_row_filter_match", match("%".join("a" * 17).encode()))            # the segment limit
    refused("vrag_row_filter_match", match(b"abc\\"))                               # a trailing backslash
    refused("vrag_row_filter_match", match(b"a\xff%"))                              # invalid UTF-8 in a pattern
    refused("vrag_row_filter_match", match(b"\xc3", op=2))
    refused("vrag_row_filter_match", match(b"\xed\xa0\x80"))                        # a surrogate is no UTF-8 either
    refused("vrag_row_filter_match", match(b"a", op=7))
    refused("vrag_row_filter_match", match(b"a", op=-1))
    assert match(b"x" * 256) == 0 and match("%".join("a" * 16).encode()) == 0 and match(b"a\\\\") == 0    # at the limits
    out[:] = SENTINEL

    def append(data, off, column=empty):
        d, o = np.frombuffer(data, np.uint8), np.asarray(off, np.int64)
        return lib.vrag_row_filter_append_strings(h, column, d.ctypes.data_as(_lib.C.c_void_p) if len(d) else None,
                                                  o.ctypes.data_as(_lib.C.c_void_p), len(o) - 1)

    refused("vrag_row_filter_append_strings", append(b"abc", [1, 3]))               # offsets start at 0
    refused("vrag_row_filter_append_strings", append(b"abc", [0, 2, 1, 3]))         # and ascend
    refused("vrag_row_filter_append_strings", append(b"ab\xffc", [0, 4]))           # invalid UTF-8
    refused("vrag_row_filter_append_strings", append("aé".encode(), [0, 2, 3]))     # a string boundary inside a code point
    refused("vrag_row_filter_append_strings", append(b"abc", [0, 3], column=99))
    assert rf.strings(empty) == (0, 0) and rf.strings(at)[0] == N

    source = rf.add_column()
    rows = [{"t": s} for s in dictionary(100)]
    meta = column_of([md["t"] for md in rows])
    rf.append(source, meta.kinds, meta.payload)
    rf.append_strings(source, *meta.string_bytes(0)[:1], meta.string_bytes(0)[1][:41])          # rows of 100 codes, a dictionary of 40
    assert rf.strings(source)[0] == 40
    leaves, ops, tables, matches, texts = program_arrays(compile_filter('t LIKE "a%" or t == 5'), [(source, meta)], device_strings=True)
    assert len(matches) == 1 and matches[0].leaf == 0 and texts == b"a%"
    res = np.full(8, SENTINEL, np.uint32)

    def refused_eval(mt, tx=texts, lv=leaves):
        with pytest.raises(_lib.VragError) as err:
            rf.eval(lv, ops, tables, 100, out=res, matches=mt, texts=tx)
        assert err.value.status == -1 and "vrag_row_filter_eval_matched" in str(err.value) and (res == SENTINEL).all()

    refused_eval(matches)                                                           # the leaf's 100 codes against 40 held
    rf.append_strings(source, meta.string_bytes(40)[0], meta.string_bytes(40)[1])
    M = _lib.FilterMatch
    refused_eval([M(text_off=0, text_len=2, leaf=1, op=6)])                         # leaf 1 (`== 5`) is no table leaf
    refused_eval([M(text_off=0, text_len=2, leaf=2, op=6)])                         # no such leaf
    refused_eval([M(text_off=1, text_len=2, leaf=0, op=6)])                         # the text lies outside `texts`
    refused_eval([M(text_off=0, text_len=2, leaf=0, op=9)])
    refused_eval([M(text_off=0, text_len=3, leaf=0, op=6)], tx=b"ab\\")
    refused_eval([M(text_off=0, text_len=2, leaf=0, op=6)] * 3)                     # more matches than leaves
    short = [_lib.FilterLeaf.from_buffer_copy(lf) for lf in leaves]
    short[0].table_off = len(tables)                                                # the leaf's range lies outside the table words
    refused_eval(matches, lv=short)
    # and the handle still answers
    got = rf.eval(leaves, ops, tables, 100, matches=matches, texts=texts)
    assert np.array_equal(got, table_bits(expected('t LIKE "a%" or t == 5', rows)))
    assert np.array_equal(rf.match(at, "like", "%a%", 65), table_bits(want[("like", "%a%")][:65]))


def random_program(rng):
    titles = ["%a%", "a%", "%b", "_", "%é%", "日%", "%BERT%", "a_b", "%\\%%", "%#1%", "%" * 3, "x%x"]
    atoms = [lambda: f'title LIKE "{rng.choice(titles)}"', lambda: f'odd LIKE "{rng.choice(titles)}"',
             lambda: f'title {rng.choice(COMPARE_OPS)} "{rng.choice(["a", "b", "", "é", "BERT", "x" * 10])}"',
             lambda: f'odd {rng.choice(COMPARE_OPS)} "{rng.choice(["a", "ab", "日本"])}"',
             lambda: f"year {rng.choice(COMPARE_OPS)} {rng.choice([2001, 2010.5, 2020])}", lambda: f"peer == {rng.choice(['true', 'false'])}",
             lambda: f'title not in ["a", "BERT", {rng.choice([1, 2])}]']

    def tree(depth):
        if depth == 0 or rng.random() < 0.3:
            return rng.choice(atoms)()
        kind = rng.random()
        if kind < 0.2:
            return f"not ({tree(depth - 1)})"
        return f"({tree(depth - 1)}) {rng.choice(['and', 'or', '&&', '||'])} ({tree(depth - 1)})"
    return tree(3)


def test_device_strings_equal_host_strings_on_random_programs():
    rng = random.Random(17)
    pool = dictionary(900)
    rows = []
    for i in range(N):
        md = {"title": rng.choice(pool), "odd": rng.choice(STR), "year": 2000 + i % 25, "peer": bool(i % 3)}
        if i % 11 == 0:
            md["title"] = rng.choice([None, 7, True, ["a"]])
        if i % 13 == 0:
            del md["title"]
        if i % 97 == 5:
            md["odd"] = "lone \ud800 surrogate"                         # no UTF-8 form: this column's leaves keep host tables
        rows.append(md)
    metas = {k: MetaColumn(k) for k in ("title", "odd", "year", "peer")}
    rf = RowFilter()
    try:
        cols = {}
        for k, m in metas.items():
            m.extend(rows)
            cols[k] = (rf.add_column(), m)
            rf.append(cols[k][0], m.kinds, m.payload)
        assert metas["title"].encodable and not metas["odd"].encodable
        exprs = [random_program(rng) for _ in range(60)]
        exprs += ['title LIKE "%a%" and odd LIKE "%a%"', f'title LIKE "%{"y" * 299}" or title LIKE "a%"', f'title < "{"b" * 300}" and peer == true']
        assert sum("LIKE" in e for e in exprs) > 30 and sum("year" in e for e in exprs) > 10
        split = 0
        for expr in exprs:
            prog = compile_filter(expr)
            columns = [cols[k] for k in prog.keys]
            kept = []
            host = rf.eval_program(prog, columns, N)
            dev = rf.eval_program(prog, columns, N, strings="device", kept=kept)
            want = expected(expr, rows)
            assert np.array_equal(host, want) and np.array_equal(dev, want), (expr, np.nonzero(dev != want)[0][:8])
            split += int(want.any() and not want.all())
            n_odd = sum(1 for lf in prog.leaves if prog.keys[lf.column] == "odd" and lf.str_op not in ("never", "always"))
            n_long = sum(1 for lf in prog.leaves if len(lf.text) >= 300)
            assert len(kept) == n_odd + n_long, (expr, kept)            # exactly those leaves stayed on the host
        assert split > 40
        assert rf.strings(cols["title"][0])[0] == len(metas["title"].strings) and rf.strings(cols["odd"][0]) == (0, 0)
        with pytest.raises(ValueError, match="strings must be"):
            rf.eval_program(compile_filter("year > 1"), [cols["year"]], N, strings="gpu")
    finally:
        rf.close()
