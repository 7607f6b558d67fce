"""Generates verbatim-rag_amd/csrc/wordpiece_table.inc: the per-code-point table of the device WordPiece tokenizer
(csrc/wordpiece.hip) -- what HF `BertNormalizer` + `BertPreTokenizer` do to ONE code point, for every code point.

For a code point c and a variant v = 2 * strip_accents + lowercase the table gives
  * the output code points (0 .. K of them): NFD(c) without its Mn code points when strip_accents, then str.lower() of each
    when lowercase (per character, as `NormalizedString::lowercase` does: no final-sigma context);
  * class bits: WS (White_Space: a separator), PUNCT (ASCII punctuation or category P*, of the output: a word of its own),
    CJK (the `handle_chinese_chars` ranges, of the input: a word of its own), REMOVE (`clean_text` drops it: U+0000, U+FFFD,
    Cc / Cf other than tab, LF, CR), NOTCOV (not covered: the text that holds it is tokenised on the host).
The prediction comes from `unicodedata`; it is then VERIFIED against what `tokenizers` does to c alone and inside
"a" + c + "b", for every variant with clean_text and handle_chinese_chars on, and for two variants with each of them off.
A code point is NOTCOV, never guessed at, when the two disagree, when it is unassigned in this `unicodedata` (or private
use / surrogate), when it has a non-zero combining class without being Mn (NFD would reorder it), when it expands to
more than K code points or to more code points than its UTF-8 form has bytes (the kernel's token scratch is indexed by
source byte), or when it is a Hangul syllable under strip_accents (algorithmic NFD: left to the host).

Layout: kWpPage[c >> 7] -> page; kWpCell[page * 128 + (c & 127)] -> record; kWpRec[record][v] = class | n << 8 | off << 16
(n = 255: the output is c itself; else kWpOut[off .. off + n)).  Both library versions are recorded in the file.
`python tools/gen_wordpiece_table.py` rewrites the file; `--check` exits 1 when it differs from what this interpreter generates."""
from __future__ import annotations

import os
import sys
import unicodedata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "verbatim-rag_amd", "csrc", "wordpiece_table.inc")
MAX_CP = 0x110000
K = 3
PAGE_SHIFT = 7
WS, PUNCT, CJK, NOTCOV, REMOVE = 1, 2, 4, 8, 16
IDENT = 255
_CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
               (0x2B920, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
_SENTINEL = "xqx"


def is_cjk(c: int) -> bool:
    return any(a <= c <= b for a, b in _CJK_RANGES)


def is_punct(c: int) -> bool:
    return 33 <= c <= 47 or 58 <= c <= 64 or 91 <= c <= 96 or 123 <= c <= 126 or unicodedata.category(chr(c)).startswith("P")


def is_space(c: int) -> bool:
    # the White_Space property: str.isspace() minus the four separators U+001C .. U+001F (bidi classes, not White_Space)
    return chr(c).isspace() and not 0x1C <= c <= 0x1F


def is_removed(c: int) -> bool:
    return c == 0 or c == 0xFFFD or (unicodedata.category(chr(c)) in ("Cc", "Cf") and c not in (9, 10, 13))


def by_rule_not_covered(c: int) -> bool:
    cat = unicodedata.category(chr(c))
    if cat in ("Cn", "Co", "Cs"):
        return True
    return unicodedata.combining(chr(c)) != 0 and cat != "Mn"


def predict(c: int, strip: bool, lower: bool):
    """(output code points, class bits) of c under one variant; None = not covered by rule."""
    if by_rule_not_covered(c):
        return None
    if strip and 0xAC00 <= c <= 0xD7A3:
        return None
    s = chr(c)
    if strip:
        s = "".join(ch for ch in unicodedata.normalize("NFD", s) if unicodedata.category(ch) != "Mn")
    if lower:
        s = "".join(ch.lower() for ch in s)
    out = tuple(ord(ch) for ch in s)
    if len(out) > K or len(out) > len(chr(c).encode("utf-8")):
        return None
    cls = 0
    if is_removed(c):
        cls |= REMOVE
    if is_space(c):
        cls |= WS
    if is_cjk(c):
        cls |= CJK
    if len(out) == 1 and is_punct(out[0]):
        cls |= PUNCT
    return out, cls


def expected_pieces(c: int, pred, clean: bool, chinese: bool):
    """The pre-tokenised pieces of `"a" + c + "b"` and of c alone that the prediction stands for."""
    out, cls = pred
    s = "".join(map(chr, out))
    if (clean and cls & REMOVE) or not out:
        return ["ab"], []
    if cls & WS:
        return ["a", "b"], []
    if (chinese and cls & CJK) or cls & PUNCT:
        return ["a", s, "b"], [s]
    return ["a" + s + "b"], [s]


def _pieces(norm, pre, text: str):
    return [p for p, _span in pre.pre_tokenize_str(norm.normalize_str(text))]


def _groups(pieces):
    groups, cur = [], []
    for p in pieces:
        if p == _SENTINEL:
            groups.append(cur)
            cur = []
        else:
            cur.append(p)
    return groups, cur


def verify(preds, strip: bool, lower: bool, clean: bool, chinese: bool, bad: set, only: int = 0) -> None:
    """Adds to `bad` every code point whose prediction is not what `tokenizers` does (`only`: just the code points with one
    of these class bits -- the ones an option that is off treats differently)."""
    from tokenizers.normalizers import BertNormalizer
    from tokenizers.pre_tokenizers import BertPreTokenizer

    norm = BertNormalizer(clean_text=clean, handle_chinese_chars=chinese, strip_accents=strip, lowercase=lower)
    pre = BertPreTokenizer()
    cps = [c for c in sorted(preds) if c not in bad and (not only or preds[c][1] & only)]
    step = 4096
    for i in range(0, len(cps), step):
        chunk = cps[i:i + step]
        text = "".join(f"a{chr(c)}b {_SENTINEL} {chr(c)} {_SENTINEL} " for c in chunk)
        groups, rest = _groups(_pieces(norm, pre, text))
        if len(groups) == 2 * len(chunk) and not rest:
            for j, c in enumerate(chunk):
                inside, alone = expected_pieces(c, preds[c], clean, chinese)
                if groups[2 * j] != inside or groups[2 * j + 1] != alone:
                    bad.add(c)
            continue
        for c in chunk:     # a code point of this chunk disturbed the sentinels: one at a time
            inside, alone = expected_pieces(c, preds[c], clean, chinese)
            if _pieces(norm, pre, f"a{chr(c)}b") != inside or _pieces(norm, pre, chr(c)) != alone:
                bad.add(c)


def build():
    """(per code point: 4 (class, n, out) triples; code points the verification rejected)."""
    preds = [dict() for _ in range(4)]
    for c in range(MAX_CP):
        if by_rule_not_covered(c):
            continue
        for v in range(4):
            p = predict(c, bool(v & 2), bool(v & 1))
            if p is not None:
                preds[v][c] = p
    bad: set = set()
    for v in range(4):
        verify(preds[v], bool(v & 2), bool(v & 1), True, True, bad)
    for v in (0, 3):
        verify(preds[v], bool(v & 2), bool(v & 1), False, True, bad, only=REMOVE | WS)
        verify(preds[v], bool(v & 2), bool(v & 1), True, False, bad, only=CJK)
    return preds, bad


def render() -> str:
    import tokenizers

    preds, bad = build()
    pool, pool_at = [], {}
    recs, rec_at = [], {}
    cell_of = []
    for c in range(MAX_CP):
        words = []
        for v in range(4):
            p = None if c in bad else preds[v].get(c)
            if p is None:
                words.append(NOTCOV | IDENT << 8)
                continue
            out, cls = p
            if out == (c,):
                words.append(cls | IDENT << 8)
                continue
            if out not in pool_at:
                pool_at[out] = len(pool)
                pool.extend(out)
            words.append(cls | len(out) << 8 | pool_at[out] << 16)
        key = tuple(words)
        if key not in rec_at:
            rec_at[key] = len(recs)
            recs.append(key)
        cell_of.append(rec_at[key])
    assert len(pool) < 65536 and len(recs) < 65536
    psize = 1 << PAGE_SHIFT
    pages, page_at, page_of = [], {}, []
    for p0 in range(0, MAX_CP, psize):
        key = tuple(cell_of[p0:p0 + psize])
        if key not in page_at:
            page_at[key] = len(pages)
            pages.append(key)
        page_of.append(page_at[key])
    assert len(pages) < 65536

    def rows(vals, per, fmt):
        return ["  " + ",".join(fmt(x) for x in vals[i:i + per]) + "," for i in range(0, len(vals), per)]

    lines = [
        "// Generated by tools/gen_wordpiece_table.py -- do not edit.",
        "// What BertNormalizer + BertPreTokenizer do to one code point (csrc/wordpiece.hip), predicted from Python's unicodedata",
        "// and verified against the `tokenizers` library; a code point on which the two disagree is marked not covered.",
        f"// unicodedata.unidata_version = {unicodedata.unidata_version}; tokenizers {tokenizers.__version__};"
        f" {len(bad)} code points rejected by the verification",
        f'#define VRAG_WP_UNIDATA_VERSION "{unicodedata.unidata_version}"',
        f'#define VRAG_WP_TOKENIZERS_VERSION "{tokenizers.__version__}"',
        f"#define VRAG_WP_K {K}",
        f"#define VRAG_WP_PAGE_SHIFT {PAGE_SHIFT}",
        f"#define VRAG_WP_PAGES {len(pages)}",
        f"#define VRAG_WP_RECS {len(recs)}",
        f"#define VRAG_WP_OUTS {len(pool)}",
        "// page of code point c: kWpPage[c >> VRAG_WP_PAGE_SHIFT]",
        f"WORDPIECE_TABLE_STORAGE unsigned short kWpPage[{len(page_of)}] = {{",
    ]
    lines += rows(page_of, 32, str)
    lines += ["};", "// record of code point c: kWpCell[page << VRAG_WP_PAGE_SHIFT | (c & (1 << VRAG_WP_PAGE_SHIFT) - 1)]",
              "WORDPIECE_TABLE_STORAGE unsigned short kWpCell[VRAG_WP_PAGES << VRAG_WP_PAGE_SHIFT] = {"]
    for pg in pages:
        lines += rows(list(pg), 32, str)
    lines += ["};", "// [variant 2 * strip_accents + lowercase]: class bits | n << 8 (255: the code point itself) | offset into kWpOut << 16",
              "WORDPIECE_TABLE_STORAGE unsigned kWpRec[VRAG_WP_RECS][4] = {"]
    lines += ["  {" + ",".join(f"0x{w:X}" for w in r) + "}," for r in recs]
    lines += ["};", "WORDPIECE_TABLE_STORAGE unsigned kWpOut[VRAG_WP_OUTS] = {"]
    lines += rows(pool, 16, lambda x: f"0x{x:X}")
    lines += ["};", ""]
    return "\n".join(lines)


def recorded_versions():
    """(unidata version, tokenizers version) the committed file was generated with."""
    import re

    with open(OUT, encoding="utf-8") as f:
        head = f.read(4096)
    return (re.search(r'VRAG_WP_UNIDATA_VERSION "([^"]+)"', head).group(1),
            re.search(r'VRAG_WP_TOKENIZERS_VERSION "([^"]+)"', head).group(1))


def main(argv) -> int:
    text = render()
    if "--check" in argv:
        with open(OUT, encoding="utf-8") as f:
            return 0 if f.read() == text else 1
    with open(OUT, "w", encoding="utf-8") as f:
        f.write(text)
    print(f"wrote {OUT}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
