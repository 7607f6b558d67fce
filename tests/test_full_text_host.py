"""CPU checks of the full-text analyzer: the committed character table, the analyzer's semantics on the host restatement, and
the register / scratch budget of every csrc/fulltext.hip kernel."""
import os
import re
import shutil
import subprocess
import sys
import unicodedata

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import full_text_oracle as O  # noqa: E402

ROOT = O.ROOT
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _generator():
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_unicode_word_table", os.path.join(ROOT, "tools", "gen_unicode_word_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(unicodedata.unidata_version != O.UNIDATA_VERSION,
                    reason=f"the table was generated from Unicode {O.UNIDATA_VERSION}, this Python has {unicodedata.unidata_version}")
def test_committed_table_is_the_generator_output():
    with open(O.TABLE, encoding="utf-8") as f:
        assert f.read() == _generator().render()


@pytest.mark.skipif(unicodedata.unidata_version != O.UNIDATA_VERSION, reason="different Unicode version")
def test_table_restates_str_isalnum_and_single_code_point_lower():
    for cp in range(0x110000):
        ch = chr(cp)
        assert O.is_alnum(cp) == ch.isalnum(), hex(cp)
        low = ch.lower()
        assert O.to_lower(cp) == (ord(low) if len(low) == 1 else cp), hex(cp)


def test_analyzer_cases():
    assert O.tokens("Hello, World! hello-WORLD") == ["hello", "world", "hello", "world"]
    assert O.tokens("a_b c.d e'f") == ["a", "b", "c", "d", "e", "f"]                 # only alphanumerics join
    assert O.tokens("İstanbul") == ["İstanbul"]       # U+0130 lowercases to two code points: kept as it is
    assert O.tokens("\u03a3\u0391\u03a3 \u01c5 \u01c4 \u1e9e") == ["\u03c3\u03b1\u03c3", "\u01c6", "\u01c6", "\u00df"]   # per code point (no final sigma)
    assert O.tokens("½x ² ① ٣ 中文。日本") == ["½x", "²", "①", "٣", "中文", "日本"]      # numerics are alphanumeric
    assert O.tokens("e\u0301te\u0301") == ["e", "te"]                        # combining marks are not alphanumeric
    assert O.tokens("🙂 𝐀𝐛 𐐀") == ["𝐀𝐛", "𐐨"]
    assert O.tokens("") == [] and O.tokens(" \t.\n") == []
    assert O.term_keys("ABC") == O.term_keys("abc") == [O.fnv1a64(b"abc")]
    assert O.fnv1a64(b"") == 0xCBF29CE484222325 and O.fnv1a64(b"a") == 0xAF63DC4C8601EC8C


def test_bm25_oracle_statistics_follow_liveness():
    import numpy as np

    rows = [O.term_keys(t) for t in ("a b c", "a a", "b", "c c c d")]
    o = O.Bm25Oracle(rows)
    assert o.N == 4 and o.df(O.term_keys("a")[0]) == 2
    o.set_live(np.array([True, False, True, True]))
    assert o.N == 3 and o.df(O.term_keys("a")[0]) == 1
    rows_hit, scores = o.search(O.term_keys("a c"), 10)
    assert rows_hit.tolist() == [0, 3] or rows_hit.tolist() == [3, 0]
    assert (scores > 0).all() and scores.dtype == np.float32


def _resources(src):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(ROOT, "verbatim-rag_amd", "csrc", src),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(?:[^:]+:\d+:\d+:\s+)?(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_full_text_kernels_use_no_scratch():
    rows = _resources("fulltext.hip")
    names = " ".join(r["name"] for r in rows)
    for k in ("tok_count_kernel", "tok_emit_kernel", "radix_scatter_kernel", "rle_scatter_kernel", "df_kernel", "kd_kernel",
              "ft_lookup_kernel", "ft_score_kernel"):
        assert k in names, k
    for r in rows:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
