"""Generates verbatim-rag_amd/csrc/bpe_table.inc: the per-code-point table of the device byte-level BPE tokenizer
(csrc/bpe.hip) -- what HF's `NFC` normalizer and the GPT-2 pattern of `ByteLevel(use_regex=True)` need to know about ONE code point.

For a code point c the table gives
  * the class the pattern sees: L (`\\p{L}`: general category L*), N (`\\p{N}`: N*), W (`\\s`: the White_Space property) or
    O (anything else);
  * NFC_Quick_Check != Yes (No: NFC(c) != c; Maybe: c can combine with a code point in front of it -- the second code point
    of a primary composite, or a Hangul vowel / trailing consonant jamo) and the canonical combining class: what the
    UAX #15 quick check reads to PROVE that a text is already NFC;
  * "not covered": the text that holds c is tokenised on the host.  Unassigned, private-use and surrogate code points of this
    `unicodedata` are not covered (a newer regex engine may class them differently), and neither is
      - U+FFFD: the device's UTF-8 decoder reports ill-formed input as U+FFFD, and ill-formed input goes to the host.
The prediction comes from `unicodedata`; it is then VERIFIED against `tokenizers`: the class by pre-tokenising c between two
letters, two digits and two punctuation marks and doubled between letters, NFC_QC = Yes by normalising "a" + c + "a".  A
code point on which the two disagree is marked not covered, never guessed at (none does with the versions recorded in the file).

Layout: kBpePage[c >> 7] -> page; kBpeCell[page << 7 | (c & 127)] = class | qc << 2 | notcov << 3 | ccc << 8.
`python tools/gen_bpe_table.py` rewrites the file; `--check` exits 1 when it differs from what this interpreter generates."""
from __future__ import annotations

import os
import sys
import unicodedata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "verbatim-rag_amd", "csrc", "bpe_table.inc")
MAX_CP = 0x110000
PAGE_SHIFT = 7
O, L, N, W = 0, 1, 2, 3
QC_BIT, NOTCOV_BIT = 4, 8
# code points that are assigned but left to the host on purpose (see the module docstring)
LEFT_TO_HOST = (0xFFFD,)

_maybe = None


def is_space(c: int) -> bool:
    # the White_Space property: str.isspace() minus the four separators U+001C .. U+001F
    return chr(c).isspace() and not 0x1C <= c <= 0x1F


def char_class(c: int) -> int:
    cat = unicodedata.category(chr(c))
    if cat[0] == "L":
        return L
    if cat[0] == "N":
        return N
    return W if is_space(c) else O


def assigned(c: int) -> bool:
    return unicodedata.category(chr(c)) not in ("Cn", "Co", "Cs")


def _qc_maybe() -> set:
    """NFC_Quick_Check = Maybe: every code point that is the second of a primary composite's canonical decomposition, and the
    Hangul jamo that compose algorithmically."""
    global _maybe
    if _maybe is None:
        _maybe = set(range(0x1161, 0x1176)) | set(range(0x11A8, 0x11C3))
        for c in range(MAX_CP):
            d = unicodedata.decomposition(chr(c))
            if not d or d.startswith("<"):
                continue
            parts = d.split()
            if len(parts) == 2 and unicodedata.normalize("NFC", chr(c)) == chr(c):
                _maybe.add(int(parts[1], 16))
    return _maybe


def nfc_qc_yes(c: int) -> bool:
    return unicodedata.normalize("NFC", chr(c)) == chr(c) and c not in _qc_maybe()


def covered(c: int) -> bool:
    return assigned(c) and c not in LEFT_TO_HOST


def verify(cells) -> set:
    """The code points whose predicted cell is not what `tokenizers` does."""
    from tokenizers.normalizers import NFC
    from tokenizers.pre_tokenizers import ByteLevel

    pre = ByteLevel(add_prefix_space=False, use_regex=True)
    nfc = NFC()

    def spans(text):
        return [o for _p, o in pre.pre_tokenize_str(text)]

    bad = set()
    for c, cell in enumerate(cells):
        if cell & NOTCOV_BIT:
            continue
        ch = chr(c)
        got = L if len(spans("a" + ch + "b")) == 1 else N if len(spans("1" + ch + "1")) == 1 else O if len(spans("!" + ch + "!")) == 1 else W
        # white space doubled between letters: all but the last go to one piece, and only U+0020 joins the piece behind it
        doubled = [(0, 1), (1, 2), (2, 4)] if c == 0x20 else [(0, 1), (1, 2), (2, 3), (3, 4)]
        if got != (cell & 3) or (got == W and spans("a" + ch + ch + "b") != doubled):
            bad.add(c)
        if not cell & QC_BIT and nfc.normalize_str("a" + ch + "a") != "a" + ch + "a":
            bad.add(c)
    return bad


def build():
    cells = []
    for c in range(MAX_CP):
        if not covered(c):
            cells.append(NOTCOV_BIT)
            continue
        cells.append(char_class(c) | (0 if nfc_qc_yes(c) else QC_BIT) | unicodedata.combining(chr(c)) << 8)
    bad = verify(cells)
    for c in bad:
        cells[c] = NOTCOV_BIT
    return cells, bad


def render() -> str:
    import tokenizers

    cells, bad = build()
    psize = 1 << PAGE_SHIFT
    pages, page_at, page_of = [], {}, []
    for p0 in range(0, MAX_CP, psize):
        key = tuple(cells[p0:p0 + psize])
        if key not in page_at:
            page_at[key] = len(pages)
            pages.append(key)
        page_of.append(page_at[key])
    assert len(pages) < 65536

    def rows(vals, per):
        return ["  " + ",".join(str(x) for x in vals[i:i + per]) + "," for i in range(0, len(vals), per)]

    lines = [
        "// Generated by tools/gen_bpe_table.py -- do not edit.",
        "// What the NFC quick check and the GPT-2 pre-tokenisation pattern read of one code point (csrc/bpe.hip), predicted from",
        "// Python's unicodedata and verified against the `tokenizers` library; a code point on which the two disagree is not covered.",
        f"// unicodedata.unidata_version = {unicodedata.unidata_version}; tokenizers {tokenizers.__version__};"
        f" {len(bad)} code points rejected by the verification",
        f'#define VRAG_BPE_UNIDATA_VERSION "{unicodedata.unidata_version}"',
        f'#define VRAG_BPE_TOKENIZERS_VERSION "{tokenizers.__version__}"',
        f"#define VRAG_BPE_PAGE_SHIFT {PAGE_SHIFT}",
        f"#define VRAG_BPE_PAGES {len(pages)}",
        "// page of code point c: kBpePage[c >> VRAG_BPE_PAGE_SHIFT]",
        f"BPE_TABLE_STORAGE unsigned short kBpePage[{len(page_of)}] = {{",
    ]
    lines += rows(page_of, 32)
    lines += ["};", "// kBpeCell[page << VRAG_BPE_PAGE_SHIFT | (c & (1 << VRAG_BPE_PAGE_SHIFT) - 1)] ="
              " class (0 other, 1 letter, 2 number, 3 white space) | NFC_QC != Yes << 2 | not covered << 3 | combining class << 8",
              "BPE_TABLE_STORAGE unsigned short kBpeCell[VRAG_BPE_PAGES << VRAG_BPE_PAGE_SHIFT] = {"]
    for pg in pages:
        lines += rows(list(pg), 32)
    lines += ["};", ""]
    return "\n".join(lines)


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
