"""`field LIKE "pattern"` and `field not in [...]` on the host: the parser, the predicate, the leaf `compile_filter` emits and the
host table the device route uses -- against a dynamic-programming matcher written without `re` (tests/like_cases.py) and an
independent `re` translation written here."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from filter_cases import interpret
from like_cases import MATCH_ALL, MATCH_NONE, PAT, STR, elements, like_ref, random_pairs
from verbatim_rag_amd import _lib
from verbatim_rag_amd.store_columns import MetaColumn
from verbatim_rag_amd.store_filter import STRING_COMPARE, FilterLeaf, compile_filter, parse_filter, parse_filter_ast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every kind of value tests/test_row_filter_unit_gpu.py stores (its VALUES), restated
VALUES = [float("-inf"), -1, -0.0, 0.0, 1, 1.5, 2020, 2020.0, float("inf"), 2 ** 53 + 1, "", "a", "b", "2020", "Zürich", True, False, None,
          [1], {"a": 1}]
PAIRS = random_pairs(24000, seed=3)


def quoted(pattern):
    """The pattern as a filter literal: the tokenizer's strings have no escapes, so one holding a `"` goes into '...'."""
    assert not ('"' in pattern and "'" in pattern)
    return f"'{pattern}'" if '"' in pattern else f'"{pattern}"'


def like(pattern, key="t"):
    return parse_filter(f"{key} LIKE {quoted(pattern)}")


def re_translation(pattern):
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == "\\":
            i += 1
            out.append(re.escape(pattern[i]))
        else:
            out.append(".*" if c == "%" else "." if c == "_" else re.escape(c))
        i += 1
    return re.compile("".join(out), re.S)


def test_the_fixture_splits_the_strings():
    """Every pattern matches at least one string and rejects at least one, but for the two that match all and the two that match
    none: a matcher that answers a constant cannot pass the tests below."""
    for p in PAT:
        hits = [like_ref(s, p) for s in STR]
        assert all(hits) == (p in MATCH_ALL) and (not any(hits)) == (p in MATCH_NONE), p
    assert len(set(STR)) == len(STR) and len(set(PAT)) == len(PAT)


def test_the_closure_equals_the_reference_matcher_on_the_fixture():
    for p in PAT:
        pred, rx = like(p), re_translation(p)
        for s in STR:
            want = like_ref(s, p)
            assert pred({"t": s}) is want, (p, s)
            assert (rx.fullmatch(s) is not None) is want, (p, s)


def test_the_closure_equals_the_reference_matcher_on_random_pairs():
    assert len(PAIRS) >= 20000
    hits = 0
    preds = {}
    for p, s in PAIRS:
        pred = preds.get(p) or preds.setdefault(p, (parse_filter(f'metadata["t"] LIKE "{p}"'), re_translation(p)))
        want = like_ref(s, p)
        hits += want
        assert pred[0]({"t": s}) is want and (pred[1].fullmatch(s) is not None) is want, (p, s)
    assert 1000 < hits < len(PAIRS) - 1000
    assert any("\\" in p for p, _s in PAIRS) and any("日" in s for _p, s in PAIRS)


def test_a_character_is_one_code_point_and_a_newline_is_a_character():
    assert like("Z_rich")({"t": "Zürich"}) and not like("Z__rich")({"t": "Zürich"})
    assert like("_")({"t": "😀"}) and like("_")({"t": "\n"}) and like("a%b")({"t": "a\n\nb"})
    assert not like("bert%")({"t": "BERT-base"}) and like("BERT%")({"t": "BERT-base"})      # case-sensitive
    assert like("BERT")({"t": "BERT"}) and not like("BERT")({"t": "BERT-base"})             # the whole string
    assert like('say "%')({"t": 'say "hi"'})                                                # a `"` inside '...'


def test_only_a_stored_string_matches():
    rows = [{"v": v} for v in VALUES] + [{}, {"w": "a"}]
    for p in ("%", "_%", "2020", "%a%", "1", "True", ""):
        pred, negated = like(p, "v"), parse_filter(f'not (metadata["v"] LIKE "{p}")')
        for md in rows:
            v = md.get("v")
            want = isinstance(v, str) and like_ref(v, p)
            assert pred(md) is want and negated(md) is (not want), (p, md)
    # so the negation holds for every row that holds no string, exactly as `not (v == "x")` does
    assert [parse_filter('not (v LIKE "x%")')(md) for md in rows] == [parse_filter('not (v == "x")')(md) for md in rows]


def test_not_in_is_the_negation_of_in():
    assert parse_filter_ast('x not in [1, "a", true]') == ("not", parse_filter_ast('x in [1, "a", true]'))
    assert parse_filter_ast('metadata["x"] NOT IN ["a"]') == ("not", ("in", "x", [("s", "a")]))
    rows = [{"x": v} for v in VALUES] + [{}]
    for lst in ('[1, "a", true]', '["2020", 2020]', "[false]", '["nobody"]'):
        a, b = parse_filter(f"x not in {lst}"), parse_filter(f"not (x in {lst})")
        got = [a(md) for md in rows]
        assert got == [b(md) for md in rows] == [not parse_filter(f"x in {lst}")(md) for md in rows]
        assert any(got) and got[-1]                                     # a missing key is in no list
    assert not all(parse_filter('x not in [1, "a", true]')(md) for md in rows)
    prog = compile_filter('x not in [1, "a"]')
    assert prog.ops == [("leaf", 0), ("leaf", 1), ("or", 0), ("not", 0)] and not hasattr(parse_filter('x not in [1]'), "lookup")


def test_like_combines_with_the_rest_of_the_grammar_in_both_dialects():
    rows = [{"title": t, "year": 2000 + i % 30, "lang": ("en", "de", None)[i % 3]} for i, t in enumerate(STR * 3)] + [{"year": 2025}]

    def sel(expr):
        return [i for i, md in enumerate(rows) if parse_filter(expr)(md)]

    def brute(f):
        return [i for i, md in enumerate(rows) if f(md)]

    def t(md):
        return md.get("title") if isinstance(md.get("title"), str) else None

    assert sel('title LIKE "%BERT%" and year >= 2010') == brute(lambda md: t(md) is not None and "BERT" in t(md) and md["year"] >= 2010)
    assert sel('metadata["title"] LIKE "a%" || metadata["lang"] == "de"') == \
        brute(lambda md: (t(md) is not None and t(md).startswith("a")) or md.get("lang") == "de")
    assert sel('not (title LIKE "%a%" or title LIKE "%b%") && lang not in ["de"]') == \
        brute(lambda md: not (t(md) is not None and ("a" in t(md) or "b" in t(md))) and md.get("lang") != "de")
    assert sel("(title LIKE '_' or title LIKE '__') and not year < 2005") == \
        brute(lambda md: t(md) is not None and len(t(md)) in (1, 2) and md["year"] >= 2005)
    for expr in ('title LIKE "%BERT%" and year >= 2010', 'not (title LIKE "%a%" or title LIKE "%b%") && lang not in ["de"]'):
        assert 0 < len(sel(expr)) < len(rows)
        prog = compile_filter(expr)
        cols = []
        for k in prog.keys:
            cols.append(MetaColumn(k))
            cols[-1].extend(rows)
        assert np.flatnonzero(interpret(prog, cols)).tolist() == sel(expr)


def test_errors():
    for bad, word in (('t LIKE "abc\\"', "backslash"), ('t LIKE "\\"', "backslash"), ("t LIKE 5", "quoted pattern"), ("t LIKE", ""),
                      ("t LIKE true", "quoted pattern"), ('t LIKE "a" "b"', ""), ('LIKE "a"', ""), ('t LIKE LIKE "a"', ""),
                      ("t not [1]", ""), ("t not in 1", ""), ('t not LIKE "a"', "")):
        with pytest.raises(ValueError) as one:
            parse_filter(bad)
        with pytest.raises(ValueError) as two:
            compile_filter(bad)
        assert str(one.value) == str(two.value) and str(one.value).startswith("GpuVectorStore: ") and word in str(one.value), bad
    for casing in ("like", "Like", "lIKE", "liKe"):
        with pytest.raises(ValueError, match="LIKE"):
            parse_filter(f'metadata["x"] {casing} "y%"')
        with pytest.raises(ValueError, match="LIKE"):
            parse_filter(f'x {casing} "y%"')
    # a key that is spelled like the keyword stays reachable
    assert parse_filter('metadata["LIKE"] LIKE "a%"')({"LIKE": "abc"}) and parse_filter('metadata["like"] == 1')({"like": 1})
    assert parse_filter("like == 1")({"like": 1})


def test_the_leaf_of_a_like_and_its_host_table():
    prog = compile_filter('metadata["t"] LIKE "%a\\%_"')
    assert prog.keys == ["t"] and prog.ops == [("leaf", 0)]
    assert prog.leaves == [FilterLeaf(column=0, other=False, bools=(False, False), num_op="never", bound=0.0, str_op="like",
                                      text="%a\\%_")]
    assert "like" in STRING_COMPARE
    col = MetaColumn("t")
    col.extend([{"t": s} for s in STR] + [{"t": 5}, {}, {"t": STR[3]}])
    assert col.strings == STR
    for p in PAT:
        bits = np.unpackbits(col.string_table("like", p).view(np.uint8), bitorder="little")
        assert bits[: len(STR)].tolist() == [int(like(p)({"t": s})) for s in STR] and not bits[len(STR):].any(), p
    col.extend([{"t": "BERT again"}])                                   # a table asked for before an insert covers the new string
    assert np.unpackbits(col.string_table("like", "BERT%").view(np.uint8), bitorder="little")[len(STR)] == 1
    prog = compile_filter('t LIKE "BERT%" or not t LIKE "%a%"')
    rows = [{"t": s} for s in STR] + [{"t": 5}, {}, {"t": STR[3]}, {"t": "BERT again"}]
    assert interpret(prog, [col]).tolist() == [parse_filter('t LIKE "BERT%" or not t LIKE "%a%"')(md) for md in rows]


def test_the_dictionary_bytes_a_column_hands_out():
    col = MetaColumn("t")
    col.extend([{"t": s} for s in STR[:10]])
    data, off = col.string_bytes()
    assert data.dtype == np.uint8 and off.dtype == np.int64 and off[0] == 0 and len(off) == 11
    assert [bytes(data[off[i]:off[i + 1]]).decode() for i in range(10)] == STR[:10]
    col.extend([{"t": s} for s in STR])
    data, off = col.string_bytes(10)                                    # only the codes from 10 on
    assert off[0] == 0 and [bytes(data[off[i]:off[i + 1]]).decode() for i in range(len(off) - 1)] == STR[10:]
    data, off = col.string_bytes(len(STR))
    assert len(data) == 0 and off.tolist() == [0]
    assert col.encodable
    col.extend([{"t": "ok"}, {"t": "lone \ud800 surrogate"}, {"t": "later"}])
    assert not col.encodable and col.strings[-3:] == ["ok", "lone \ud800 surrogate", "later"]      # it still has its code
    assert np.unpackbits(col.string_table("like", "lone%").view(np.uint8), bitorder="little")[len(STR) + 1] == 1


def test_match_constants_and_struct_layout_match_the_header(tmp_path):
    from test_capi_abi import _host_cc

    hdr = open(os.path.join(ROOT, "include", "vrag_amd.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"#define VRAG_FILTER_MATCH_(\w+) (\d+)", hdr)}
    names_of = {"==": "EQ", "!=": "NE", "<": "LT", "<=": "LE", ">": "GT", ">=": "GE", "like": "LIKE"}
    assert {names_of[k]: v for k, v in _lib.FILTER_MATCH_OPS.items()} == {k: v for k, v in defines.items() if not k.startswith("MAX_")}
    assert (defines["MAX_PATTERN"], defines["MAX_SEGMENTS"]) == (_lib.FILTER_MATCH_MAX_PATTERN, _lib.FILTER_MATCH_MAX_SEGMENTS) == (256, 16)
    assert set(_lib.FILTER_MATCH_OPS) == set(STRING_COMPARE)
    for name in ("vrag_row_filter_append_strings", "vrag_row_filter_strings", "vrag_row_filter_match", "vrag_row_filter_eval_matched"):
        assert name in _lib.SIGNATURES and re.search(r"\bint " + name + r"\(", hdr), name
    assert _lib.load().vrag_abi_version() == 6
    if _host_cc() is None:
        pytest.skip("no host C compiler")
    S, cname = _lib.FilterMatch, "vrag_filter_match"
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
    assert int(got.pop("sizeof")) == ctypes.sizeof(S) == 24
    assert {n: int(v) for n, v in got.items()} == {n: getattr(S, n).offset for n in names}
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct " + cname):hdr.index("} " + cname + ";")], flags=re.S)
    assert re.findall(r"\b([a-z_0-9A-Z]+)\s*;", body.split("{", 1)[1]) == names


def test_the_device_limits_python_applies_are_the_library_s():
    from verbatim_rag_amd.shards import match_on_device
    from verbatim_rag_amd.store_filter import like_segments

    assert match_on_device("like", "%a%") is None and match_on_device("==", "x" * 256) is None
    assert "257 bytes" in match_on_device("==", "x" * 257) and "bytes" in match_on_device("like", "é" * 129)
    assert match_on_device("like", "%".join("a" * 16)) is None and "17 segments" in match_on_device("like", "%".join("a" * 17))
    assert match_on_device("<", "%".join("a" * 17)) is None             # a comparison's text has no segments
    assert "UTF-8" in match_on_device("like", "\ud800")
    assert [like_segments(p) for p in ("", "%", "%%", "a", "a%", "%a%%b_", "a\\%b", "\\%%\\%")] == [0, 0, 0, 1, 1, 2, 1, 2]
    assert all(len(elements(p)) >= like_segments(p) for p in PAT)


def test_match_kernel_uses_no_scratch_and_the_eval_file_still_holds_one_kernel():
    """tools/kernel_resources.py on csrc/strmatch.hip: the pattern lives in LDS, so no kernel of the file spills or has scratch."""
    from test_kernel_resources import HIPCC

    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "verbatim-rag_amd", "csrc", "strmatch.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [line.split(None, 6) for line in out.stdout.splitlines()[1:]]
    assert rows and any("str_match_kernel" in r[6] for r in rows), out.stdout
    for _vgpr, _agpr, _sgpr, spill, scratch, _occ, name in rows:
        assert int(spill) == 0 and int(scratch) == 0, name
