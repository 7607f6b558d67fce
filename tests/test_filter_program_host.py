"""`compile_filter` and the typed columns answer what `parse_filter` answers, row for row -- checked on the host with a numpy
interpreter of the program (tests/filter_cases.py); the same property runs on the device in test_row_filter_unit_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from filter_cases import BAD_FILTERS, KEYS, columns_of, expected, interpret, random_expressions, random_rows
from verbatim_rag_amd import _lib
from verbatim_rag_amd.store_columns import MetaColumn
from verbatim_rag_amd.store_filter import MAX_COLUMNS, MAX_DEPTH, MAX_LEAVES, compile_filter, parse_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = random_rows(600, seed=11)
COLUMNS = dict(zip(KEYS, columns_of(ROWS, KEYS)))
EXPRESSIONS = random_expressions(300, seed=5)


def test_the_random_expressions_cover_the_grammar():
    text = " ".join(EXPRESSIONS)
    for piece in ("==", "!=", "<=", ">=", " < ", " > ", " in [", "not ", " and ", " or ", "&&", "||", 'metadata["', "metadata['", "true", "'"):
        assert piece in text, piece
    assert max(compile_filter(e).depth() for e in EXPRESSIONS) >= 6
    assert len(set(EXPRESSIONS)) > 250
    # and the rows hold what the comparisons are typed on
    kinds = {type(v) for md in ROWS for v in md.values()}
    assert {int, float, str, bool, type(None), list, dict} <= kinds
    assert any(len(md) < len(KEYS) for md in ROWS)


def test_program_equals_the_predicate_on_every_random_expression():
    wrong = []
    some = 0
    for expr in EXPRESSIONS:
        prog = compile_filter(expr)
        assert prog.over_limit() is None, expr
        got = interpret(prog, [COLUMNS[k] for k in prog.keys])
        want = expected(expr, ROWS)
        some += int(want.any() and not want.all())
        if not np.array_equal(got, want):
            wrong.append((expr, int((got != want).sum())))
    assert not wrong, wrong[:5]
    assert some > 100          # most expressions split the rows: the comparison is no all-zeros against all-zeros


@pytest.mark.parametrize("expr", [
    "year == 2020.0", 'tag == "5"', "tag == 5", "year != 2020", "misc != 1",
    "score >= -0.0", "score < 1e999", "score > -1e999", "score == 9007199254740993",
    'source < "b"', 'source >= ""', 'source > "Zürich"', "peer == true", "peer != false",
    'year in [2020, "2020", true]', "not year < 2000"])
def test_named_edge_cases(expr):
    prog = compile_filter(expr)
    assert np.array_equal(interpret(prog, [COLUMNS[k] for k in prog.keys]), expected(expr, ROWS)), expr


def test_leaf_answers_per_kind():
    ne = compile_filter('a != "x"').leaves[0]
    assert ne.other is True and ne.bools == (True, True) and ne.num_op == "always" and (ne.str_op, ne.text) == ("!=", "x")
    eq = compile_filter("a == true").leaves[0]
    assert eq.other is False and eq.bools == (False, True) and eq.num_op == "never" and eq.str_op == "never"
    lt = compile_filter("a < 3").leaves[0]
    assert lt.other is False and lt.bools == (False, False) and (lt.num_op, lt.bound) == ("<", 3.0) and lt.str_op == "never"
    prog = compile_filter('a in [1, "1", false] and not b >= 2')
    assert prog.keys == ["a", "b"] and len(prog.leaves) == 4
    assert prog.ops == [("leaf", 0), ("leaf", 1), ("or", 0), ("leaf", 2), ("or", 0), ("leaf", 3), ("not", 0), ("and", 0)]
    assert prog.depth() == 2


def test_a_column_extended_in_several_inserts_equals_one_built_at_once():
    whole = MetaColumn("source")
    whole.extend(ROWS)
    pieces = MetaColumn("source")
    at = 0
    for step in (1, 0, 7, 64, 3, 200, len(ROWS)):
        pieces.extend(ROWS[at:at + step])
        at += step
    assert len(pieces) == len(whole) == len(ROWS)
    assert np.array_equal(pieces.kinds, whole.kinds) and np.array_equal(pieces.payload, whole.payload)
    assert pieces.strings == whole.strings and pieces.exact and whole.exact
    for op, text in (("<", "b"), ("==", "web"), ("!=", "")):
        assert np.array_equal(pieces.string_table(op, text), whole.string_table(op, text))
    # a table asked for before an insert covers the strings that arrived since
    col = MetaColumn("k")
    col.extend([{"k": "a"}])
    assert col.string_table("<", "b").tolist() == [1]
    col.extend([{"k": "c"}, {"k": "a"}, {"k": "aa"}])
    assert col.strings == ["a", "c", "aa"] and col.string_table("<", "b").tolist() == [0b101]
    assert col.kinds.tolist() == [2, 2, 2, 2] and col.payload.tolist() == [0, 1, 0, 2]


def test_column_kinds_and_payloads():
    col = MetaColumn("v")
    col.extend([{"v": 2020}, {"v": 2020.0}, {"v": True}, {"v": False}, {"v": "x"}, {"v": None}, {}, {"v": [1]}, {"v": -0.0},
                {"v": float("inf")}, {"v": 2 ** 53 + 1}, {"v": ""}])
    assert col.kinds.tolist() == [1, 1, 3, 3, 2, 0, 0, 0, 1, 1, 1, 2]
    f = lambda x: int(np.float64(x).view(np.uint64))   # noqa: E731
    assert col.payload.tolist() == [f(2020.0), f(2020.0), 1, 0, 0, 0, 0, 0, f(-0.0), f(np.inf), f(2.0 ** 53), 1]
    assert col.payload[8] == 1 << 63 and col.exact


def test_a_nan_marks_the_column_inexact():
    col = MetaColumn("v")
    col.extend([{"v": 1.0}, {"v": "nan"}, {"v": [float("nan")]}])
    assert col.exact                                       # a NaN inside a list is not a number of this column
    col.extend([{"v": float("nan")}])
    assert not col.exact
    col.extend([{"v": 2.0}])
    assert not col.exact and len(col) == 5
    big = MetaColumn("v")
    big.extend([{"v": 10 ** 400}])                         # float(value) overflows: parse_filter's closure raises for this row
    assert not big.exact and len(big) == 1


def test_each_limit_is_reported():
    seventeen = " or ".join(f"k{i} > {i}" for i in range(MAX_COLUMNS + 1))
    assert "17 columns" in compile_filter(seventeen).over_limit()
    assert compile_filter(" or ".join(f"k{i} > {i}" for i in range(MAX_COLUMNS))).over_limit() is None
    sixty_five = " or ".join(f"a == {i}" for i in range(MAX_LEAVES + 1))
    assert "65 leaves" in compile_filter(sixty_five).over_limit()
    assert "65 leaves" in compile_filter("a in [" + ", ".join(str(i) for i in range(MAX_LEAVES + 1)) + "]").over_limit()
    assert compile_filter(" or ".join(f"a == {i}" for i in range(MAX_LEAVES))).over_limit() is None

    def nested(depth):                                     # a and (a and (a and ...)): every level keeps one value waiting
        return "a > 0" if depth == 1 else f"a > {depth} and ({nested(depth - 1)})"

    assert compile_filter(nested(MAX_DEPTH)).depth() == MAX_DEPTH and compile_filter(nested(MAX_DEPTH)).over_limit() is None
    deep = compile_filter(nested(MAX_DEPTH + 1))
    assert deep.depth() == MAX_DEPTH + 1 and "33 stack depth" in deep.over_limit()
    ops = compile_filter(" and ".join(["not not not a > 1"] * 52))
    assert len(ops.ops) > 256 and "ops" in ops.over_limit()
    # over the limits is no error of the filter: the predicate still answers, and the program still equals it
    rows = [{"a": i} for i in range(-3, 70)]
    for expr in (sixty_five, nested(MAX_DEPTH + 1)):
        prog = compile_filter(expr)
        assert np.array_equal(interpret(prog, columns_of(rows, prog.keys)), expected(expr, rows))


def test_parse_filter_still_refuses_what_it_refused():
    for bad in BAD_FILTERS + ("a < true", "a >= false"):
        with pytest.raises(ValueError) as one:
            parse_filter(bad)
        with pytest.raises(ValueError) as two:
            compile_filter(bad)
        assert str(one.value) == str(two.value) and str(one.value).startswith("GpuVectorStore: ")
    assert "ordering comparison with a boolean" in str(pytest.raises(ValueError, parse_filter, "a < true").value)
    assert "cannot parse filter at" in str(pytest.raises(ValueError, parse_filter, "a == $").value)
    assert parse_filter('a == "x"').lookup == ("a", [("s", "x")])
    assert parse_filter('a in [1, "x"]').lookup == ("a", [("n", 1.0), ("s", "x")])
    assert not hasattr(parse_filter("a != 1"), "lookup") and not hasattr(parse_filter("a == 1 and b == 2"), "lookup")


def test_filter_leaf_layout_matches_ctypes(tmp_path):
    """vrag_filter_leaf crosses the ctypes boundary of every device filter: sizeof and every offsetof as the host C compiler lays
    the struct out must equal _lib.FilterLeaf, and the header declares no field the ctypes side lacks."""
    from test_capi_abi import _host_cc

    if _host_cc() is None:
        pytest.skip("no host C compiler")
    S, cname = _lib.FilterLeaf, "vrag_filter_leaf"
    names = [f[0] for f in S._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"vrag_amd.h\"\nint main(void) {\n"
                   f"  printf(\"sizeof %zu\\n\", sizeof({cname}));\n"
                   + "".join(f"  printf(\"{n} %zu\\n\", offsetof({cname}, {n}));\n" for n in names)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([_host_cc(), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(S) == 32
    assert {n: int(v) for n, v in got.items()} == {n: getattr(S, n).offset for n in names}
    hdr = open(os.path.join(ROOT, "include", "vrag_amd.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct " + cname):hdr.index("} " + cname + ";")], flags=re.S)
    assert re.findall(r"\b([a-z_0-9A-Z]+)\s*;", body.split("{", 1)[1]) == names
    # the constants the binding repeats
    defines = dict(re.findall(r"#define VRAG_FILTER_(\w+) (\d+)", hdr))
    assert [int(defines["MAX_" + n]) for n in ("COLUMNS", "LEAVES", "OPS", "DEPTH")] == \
        [_lib.FILTER_MAX_COLUMNS, _lib.FILTER_MAX_LEAVES, _lib.FILTER_MAX_OPS, _lib.FILTER_MAX_DEPTH] == [16, 64, 256, 32]
    for prefix, table in (("KIND_", _lib.FILTER_KINDS), ("STR_", _lib.FILTER_STR_MODES), ("OP_", _lib.FILTER_OPS)):
        assert {k.upper(): v for k, v in table.items()} == {k[len(prefix):]: int(v) for k, v in defines.items() if k.startswith(prefix)}
    names_of = {"==": "EQ", "!=": "NE", "<": "LT", "<=": "LE", ">": "GT", ">=": "GE", "never": "NEVER", "always": "ALWAYS"}
    assert {names_of[k]: v for k, v in _lib.FILTER_NUM_OPS.items()} == {k[4:]: int(v) for k, v in defines.items() if k.startswith("NUM_")}


def test_row_filter_create_reports_a_missing_device():
    lib = _lib.load()
    if lib.vrag_device_count() > 0:
        pytest.skip("GPU present")
    h = ctypes.c_void_p()
    assert lib.vrag_row_filter_create(0, ctypes.byref(h)) == -4 and not h.value
    assert "no HIP device" in _lib.last_error()
    from verbatim_rag_amd.shards import RowFilter

    with pytest.raises(RuntimeError, match="no HIP device"):
        RowFilter()


def test_eval_kernel_uses_no_scratch():
    """tools/kernel_resources.py on csrc/rowfilter.hip: the evaluation stack is one register, so the kernel has no scratch and
    spills nothing."""
    from test_kernel_resources import HIPCC

    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "verbatim-rag_amd", "csrc", "rowfilter.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [line.split(None, 6) for line in out.stdout.splitlines()[1:]]
    kernels = [r for r in rows if "row_filter_eval_kernel" in r[6]]
    assert len(kernels) == 1 and len(rows) == 1, out.stdout
    vgpr, _agpr, _sgpr, spill, scratch, occ, _name = kernels[0]
    assert int(spill) == 0 and int(scratch) == 0 and int(occ) == 8 and int(vgpr) <= 32, kernels[0]
