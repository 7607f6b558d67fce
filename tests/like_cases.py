"""What the `LIKE` tests share: a reference matcher written without `re`, the fixture of strings and patterns, and a seeded
generator of random pattern / string pairs."""
import random
from functools import lru_cache

import numpy as np

STR = ["", "a", "b", "ab", "ba", "aa", "aaa", "aab", "aaab", "abab", "ababab", "abcabc", "a%b", "a_b", "a\\b", "%", "_", "__", "BERT", "bert",
       "BERT-base", "A BERT model", "SciBERT", "BERTology 2025", "2025", "é", "éa", "aé", "日本語", "日本", "本語", "a日b", "Zürich", "😀", "a😀b",
       "line\nbreak", "\n", " a", " ", "a ", "x" * 300, "ab" * 150 + "c", "\x00", "a\x00b"]
PAT = ["%", "%%", "_", "__", "_%", "%_", "_%_", "a", "a%", "%a", "%a%", "a%a", "a%a%a", "%ab%ab", "%ab%ab%", "%aab", "%aa", "aa%", "%aba%ab",
       "ab%ab", "%abc", "abc%abc", "%BERT%", "BERT%", "%BERT", "%2025%", "BERT_base", "%\\%%", "a\\%b", "a\\_b", "a_b", "a\\\\b", "\\%", "\\_",
       "_é", "é_", "%é%", "日%", "%語", "日_語", "__語", "%本%", "a_b%", "_😀_", "%\n%", "line_break", " %", "% ", "%  %", "x%x", "%" + "x" * 300,
       "x" * 299 + "_", "%c", "%" + "ab" * 8 + "c", "Z_rich", "Z__rich", "", "%\x00%"]
MATCH_ALL, MATCH_NONE = ("%", "%%"), ("%  %", "Z__rich")
ALPHABET = "ab%_\\é日"
COMPARE_OPS = ("==", "!=", "<", "<=", ">", ">=")
COMPARE_TEXTS = ("", "a", "ab", "b", "é", "日本", "x" * 300)


def elements(pattern):
    """[(kind, char)]: kind "%" / "_" / "c" (the character itself).  ValueError for a trailing lone backslash."""
    out, i = [], 0
    while i < len(pattern):
        if pattern[i] == "\\":
            if i + 1 >= len(pattern):
                raise ValueError("trailing backslash")
            out.append(("c", pattern[i + 1]))
            i += 2
        else:
            out.append((pattern[i], "") if pattern[i] in "%_" else ("c", pattern[i]))
            i += 1
    return out


@lru_cache(maxsize=None)
def _positions(stored):
    """char -> the bit set of the j with stored[j] == char."""
    where = {}
    for j, ch in enumerate(stored):
        where[ch] = where.get(ch, 0) | (1 << j)
    return where


@lru_cache(maxsize=None)
def _elements_cached(pattern):
    return tuple(elements(pattern))


def like_ref(stored, pattern):
    """Dynamic programming over code points, the row of the table held as the bits of one int: bit j of `reach` = the elements so
    far can consume exactly stored[:j].  `%` sets every bit from the lowest set one up, `_` shifts, a literal shifts the bits
    that stand in front of that character."""
    full = (1 << (len(stored) + 1)) - 1
    where = _positions(stored)
    reach = 1
    for kind, ch in _elements_cached(pattern):
        if kind == "%":
            reach = full & ~((reach & -reach) - 1) if reach else 0
        elif kind == "_":
            reach = (reach << 1) & full
        else:
            reach = ((reach & where.get(ch, 0)) << 1) & full
    return bool(reach >> len(stored) & 1)


def random_pairs(n, seed):
    """`n` (pattern, string) pairs over ALPHABET; patterns never end in a lone backslash."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        pattern = "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 7)))
        try:
            elements(pattern)
        except ValueError:
            continue
        out.append((pattern, "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 9)))))
    return out


def dictionary(n):
    """`n` distinct strings: STR cycled, every later round suffixed with its number."""
    return [STR[i % len(STR)] + ("" if i < len(STR) else f"#{i // len(STR)}") for i in range(n)]


def table_bits(answers):
    """bool per code -> the uint32 words of `MetaColumn.string_table`: bit code % 32 of word code // 32, tail bits zero."""
    bits = np.packbits(np.asarray(answers, dtype=bool), bitorder="little")
    words = np.zeros((len(bits) + 3) // 4 * 4, np.uint8)
    words[: len(bits)] = bits
    return words.view(np.uint32)
