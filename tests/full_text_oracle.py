"""Host restatement of the full-text analyzer and the BM25 arithmetic of include/vrag_amd.h (csrc/fulltext.hip), from the
committed character table verbatim-rag_amd/csrc/unicode_word.inc.  numpy float32 operations are single IEEE roundings, so
the scores below are the device's bits."""
from __future__ import annotations

import bisect
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "verbatim-rag_amd", "csrc", "unicode_word.inc")


def _load_table():
    text = open(TABLE, encoding="utf-8").read()
    version = re.search(r'#define VRAG_UNIDATA_VERSION "([^"]+)"', text).group(1)
    alnum_part, lower_part = text.split("kAlnumRanges", 1)[1].split("kLowerRuns", 1)
    alnum = [(int(a, 16), int(b, 16)) for a, b in re.findall(r"\{0x([0-9A-F]+), 0x([0-9A-F]+)\}", alnum_part)]
    lower = [(int(a, 16), int(b, 16), int(s), int(d)) for a, b, s, d in
             re.findall(r"\{0x([0-9A-F]+), 0x([0-9A-F]+), (\d+), (-?\d+)\}", lower_part)]
    return version, alnum, lower


UNIDATA_VERSION, ALNUM, LOWER = _load_table()
_ALNUM_LO = [a for a, _b in ALNUM]
_LOWER_LO = [r[0] for r in LOWER]


def is_alnum(cp: int) -> bool:
    i = bisect.bisect_right(_ALNUM_LO, cp) - 1
    return i >= 0 and cp <= ALNUM[i][1]


def to_lower(cp: int) -> int:
    i = bisect.bisect_right(_LOWER_LO, cp) - 1
    if i < 0:
        return cp
    lo, hi, stride, delta = LOWER[i]
    return cp + delta if cp <= hi and (cp - lo) % stride == 0 else cp


FNV_BASIS, FNV_PRIME, M64 = 14695981039346656037, 1099511628211, (1 << 64) - 1


def fnv1a64(data: bytes) -> int:
    h = FNV_BASIS
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & M64
    return h


def tokens(text: str) -> List[str]:
    """Maximal runs of alphanumeric code points, each code point lowercased through the table."""
    out, cur = [], []
    for ch in text:
        cp = ord(ch)
        if is_alnum(cp):
            cur.append(chr(to_lower(cp)))
        elif cur:
            out.append("".join(cur))
            cur = []
    if cur:
        out.append("".join(cur))
    return out


def term_keys(text: str) -> List[int]:
    return [fnv1a64(t.encode("utf-8", "surrogatepass")) for t in tokens(text)]


class Bm25Oracle:
    """Postings of a corpus given as the term keys of every row; scores of the live rows as the device computes them."""

    def __init__(self, row_keys: Sequence[Sequence[int]], k1: float = 1.2, b: float = 0.75):
        self.k1, self.b = np.float32(k1), np.float32(b)
        n = len(row_keys)
        self.n = n
        self.dl = np.array([len(r) for r in row_keys], np.int64)
        flat = np.fromiter((k for r in row_keys for k in r), dtype=np.uint64, count=int(self.dl.sum()))
        rows = np.repeat(np.arange(n, dtype=np.int64), self.dl)
        self._build(flat, rows)
        self.set_live(np.ones(n, dtype=bool))

    @classmethod
    def from_arrays(cls, flat_keys: np.ndarray, dl: np.ndarray, k1: float = 1.2, b: float = 0.75) -> "Bm25Oracle":
        self = cls.__new__(cls)
        self.k1, self.b = np.float32(k1), np.float32(b)
        self.n = len(dl)
        self.dl = np.asarray(dl, np.int64)
        self._build(np.asarray(flat_keys, np.uint64), np.repeat(np.arange(self.n, dtype=np.int64), self.dl))
        self.set_live(np.ones(self.n, dtype=bool))
        return self

    def _build(self, flat: np.ndarray, rows: np.ndarray) -> None:
        order = np.lexsort((rows, flat))
        k, r = flat[order], rows[order]
        head = np.ones(len(k), dtype=bool)
        head[1:] = (k[1:] != k[:-1]) | (r[1:] != r[:-1])
        pos = np.nonzero(head)[0]
        self.p_key, self.p_row = k[pos], r[pos]
        self.p_tf = np.diff(np.append(pos, len(k))).astype(np.int64)
        self.keys, self.start = np.unique(self.p_key, return_index=True)
        self.end = np.append(self.start[1:], len(self.p_key))

    def set_live(self, live: np.ndarray) -> None:
        self.live = np.asarray(live, dtype=bool)
        self.N = int(self.live.sum())
        sum_dl = int(self.dl[self.live].sum())
        avgdl = np.float32(sum_dl / self.N) if self.N else np.float32(0)
        if avgdl > 0:
            t = self.dl.astype(np.float32) / avgdl
            self.kd = self.k1 * ((np.float32(1) - self.b) + self.b * t)
        else:
            self.kd = np.full(self.n, self.k1, np.float32)

    def postings(self, key: int) -> Tuple[np.ndarray, np.ndarray]:
        i = np.searchsorted(self.keys, np.uint64(key))
        if i >= len(self.keys) or self.keys[i] != np.uint64(key):
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        return self.p_row[self.start[i]:self.end[i]], self.p_tf[self.start[i]:self.end[i]]

    def df(self, key: int) -> int:
        rows, _tf = self.postings(key)
        return int(self.live[rows].sum())

    def query_terms(self, qkeys: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Distinct keys ascending, their count in the query, fp32 weights count * idf64."""
        keys, counts = np.unique(np.asarray(list(qkeys), dtype=np.uint64), return_counts=True)
        df = np.array([self.df(int(k)) for k in keys], np.float64)
        idf = np.log(1.0 + (float(self.N) - df + 0.5) / (df + 0.5))
        return keys, counts, (counts.astype(np.float64) * idf).astype(np.float32)

    def scores(self, qkeys: Sequence[int]) -> np.ndarray:
        keys, _counts, w = self.query_terms(qkeys)
        acc = np.zeros(self.n, np.float32)
        k1p1 = self.k1 + np.float32(1)
        for key, wt in zip(keys.tolist(), w.tolist()):
            rows, tf = self.postings(key)
            if len(rows) == 0:
                continue
            tff = tf.astype(np.float32)
            c = np.float32(wt) * ((tff * k1p1) / (tff + self.kd[rows]))
            acc[rows] = acc[rows] + c
        return acc

    def search(self, qkeys: Sequence[int], k: int, allow: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(rows, scores) of the hits: score > 0, live, allowed; (score desc, row asc); at most k."""
        acc = self.scores(qkeys)
        ok = (acc > 0) & self.live
        if allow is not None:
            ok &= allow
        rows = np.nonzero(ok)[0]
        order = np.lexsort((rows, -acc[rows]))[:k]
        return rows[order], acc[rows[order]]


def random_unicode_text(rng: np.random.Generator, n_chars: int) -> str:
    """Letters of several scripts, digits, numerics, marks, punctuation, white space and astral code points."""
    pools = [
        "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789",
        " \t\n.,;:!?-_'\"()[]{}/\\@#$%^&*+=<>|~`",
        "ÀÁÂÄÅÆÇÈÉÊËÌÍÎÏÐÑÒÓÔÕÖØÙÚÛÜÝÞßàáâãäåæçèéêëìíîïñòóôõöøùúûüýþÿĀāĂăĐđĲĳŁłŒœŠšŸŽžƁƂƷǄǅǆǇǈǉ",
        "ΑΒΓΔΕΖΗΘΙΚΛΜΝΞΟΠΡΣΤΥΦΧΨΩαβγδεζηθικλμνξοπρσςτυφχψωΆΈΉΊΌΎΏάέήίόύώϐϑϒϕ",
        "АБВГДЕЁЖЗИЙКЛМНОПРСТУФХЦЧШЩЪЫЬЭЮЯабвгдеёжзийклмнопрстуфхцчшщъыьэюяѢѣ",
        "中文日本語한국어ひらがなカタカナ漢字。、「」",
        "½¼¾²³¹ⅠⅡⅢⅣⅰⅱⅲ①②③٠١٢٣०१२३",
        "́̈​ 　 ­﻿",
        "İıẞſǅǈǋǲΣϴ℃KÅⓐⒶ",
        "🙂🙃𝐀𝐁𝐚𝐛𐐀𐐨𞤀𞤢",
    ]
    chars = []
    for _ in range(n_chars):
        pool = pools[int(rng.integers(0, len(pools)))]
        chars.append(pool[int(rng.integers(0, len(pool)))])
    return "".join(chars)


EDGE_STRINGS = ["", " ", ".", " . ", "a", "a.", "a. ", " a.", "a.b", "a. b", "a .b", "a . b", "a.  . b", "?! ?", "x!\n\ny?\t z",
                "end.　next line! \xa0nbsp? ​zero-width. ﻿bom", "é. ü! 中文。不分 割. 是? 的",
                "tab.\tafter", "no stop\nnew line", "trailing stop.", "   ", "\n.\n", "a." + " " * 300 + "b.",
                "🙂. 🙃! x", ". . . .", "a.\x1cb!\x1fc?\x85d"]


def zipf_corpus(n_rows: int, vocab: int = 5000, mean_len: int = 24, seed: int = 0) -> Tuple[List[str], List[str], np.ndarray, np.ndarray]:
    """Rows of words drawn Zipf-like from a vocabulary of lower-, capitalised and upper-case forms of non-ASCII words
    (each form is one token).  Returns (texts, vocabulary, term keys of all rows' tokens back to back, tokens per row)."""
    rng = np.random.default_rng(seed)
    alpha = "abcdefghijklmnopqrstuvwxyzéüßøçñ"
    words = set()
    while len(words) < vocab:
        n = int(rng.integers(2, 9))
        words.add("".join(alpha[int(i)] for i in rng.integers(0, len(alpha), n)))
    words = sorted(words)
    words[0] = "common"                      # the Zipf head: in (nearly) every row
    ranks = np.arange(1, vocab + 1, dtype=np.float64)
    p = 1.0 / ranks ** 1.1
    p /= p.sum()
    lens = rng.integers(max(1, mean_len // 2), mean_len * 3 // 2 + 1, n_rows)
    ids = rng.choice(vocab, size=int(lens.sum()), p=p)
    cased = [w.capitalize() for w in words]
    upper = [w.upper() for w in words]
    variant = rng.integers(0, 6, size=len(ids))
    seps = [" ", ", ", ". ", "\n", " - ", "; "]
    sep_ids = rng.integers(0, len(seps), size=len(ids))
    form_keys = np.array([[term_keys(f)[0] for f in forms] for forms in (words, cased, upper)], np.uint64)
    flat_keys = form_keys[np.where(variant == 1, 1, np.where(variant == 2, 2, 0)), ids]
    texts, at = [], 0
    for ln in lens.tolist():
        parts = []
        for j in range(at, at + ln):
            w = ids[j]
            v = variant[j]
            parts.append((cased if v == 1 else upper if v == 2 else words)[w])
            parts.append(seps[sep_ids[j]])
        texts.append("".join(parts))
        at += ln
    return texts, words, flat_keys, lens
