"""Typed metadata columns: one metadata key of every stored row as the arrays the row-filter kernel reads
(include/vrag_amd.h, vrag_row_filter_append).  Host side only -- `shards.RowFilter` holds the device copies.

Per row: `kinds` (uint8: 0 missing / other, 1 number, 2 string, 3 bool) and `payload` (uint64: the f64 bits of a number, the
dictionary code of a string, 0 / 1 of a bool, 0 otherwise).  Kinds and values are `store_filter._typed`'s: bool before int,
numbers as `float(value)`.  Strings are coded in first-seen order; a filter's string comparison is applied once per distinct
string (`string_table`), with Python's own operators, so string ordering is Python's by construction.
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, Tuple

import numpy as np

from .store_filter import STRING_COMPARE, _typed

KIND_OTHER, KIND_NUMBER, KIND_STRING, KIND_BOOL = 0, 1, 2, 3      # VRAG_FILTER_KIND_*


class MetaColumn:
    """One key's column, built by one Python pass over the rows and extended by the rows of every later insert -- O(new rows),
    never a rebuild.  `exact` turns False when a value cannot be represented faithfully: a NaN (tuple equality on NaN depends on
    object identity in the closures of `parse_filter`) or an int too large for a float (`_typed` raises for it); the store then
    answers filters on this key on the host.  `encodable` turns False when a stored string has no UTF-8 form (a lone
    surrogate): the dictionary then stays on the host, and so do the tables of this column's string comparisons -- the rest
    of a filter that names the key still runs on the device."""

    def __init__(self, key: str):
        self.key = key
        self.exact = True
        self.encodable = True
        self.strings: List[str] = []                 # code -> string
        self._codes: Dict[str, int] = {}
        self._kinds = np.empty(0, np.uint8)
        self._payload = np.empty(0, np.uint64)
        self._n = 0
        self._tables: Dict[Tuple[str, str], List[bool]] = {}   # (op, text) -> answer per code, extended as the dictionary grows

    def __len__(self) -> int:
        return self._n

    @property
    def kinds(self) -> np.ndarray:
        return self._kinds[: self._n]

    @property
    def payload(self) -> np.ndarray:
        return self._payload[: self._n]

    def extend(self, rows: Iterable[Dict[str, Any]]) -> None:
        """Appends `md.get(key)` of every row."""
        key, codes, strings = self.key, self._codes, self.strings
        kinds: List[int] = []
        numbers: List[float] = []
        others: List[int] = []
        for md in rows:
            try:
                t = _typed(md.get(key))
            except OverflowError:
                t, self.exact = None, False
            kind, number, other = KIND_OTHER, 0.0, 0
            if t is not None:
                tag, value = t
                if tag == "n":
                    kind, number = KIND_NUMBER, value
                    if value != value:
                        self.exact = False
                elif tag == "s":
                    code = codes.get(value)
                    if code is None:
                        code = codes[value] = len(strings)
                        strings.append(value)
                        if self.encodable and not value.isascii():
                            try:
                                value.encode("utf-8")
                            except UnicodeEncodeError:
                                self.encodable = False
                    kind, other = KIND_STRING, code
                else:
                    kind, other = KIND_BOOL, int(value)
            kinds.append(kind)
            numbers.append(number)
            others.append(other)
        m = len(kinds)
        if self._n + m > len(self._kinds):
            cap = max(self._n + m, int(len(self._kinds) * 1.5) + 16)
            for name, dtype in (("_kinds", np.uint8), ("_payload", np.uint64)):
                grown = np.empty(cap, dtype)
                grown[: self._n] = getattr(self, name)[: self._n]
                setattr(self, name, grown)
        k = np.asarray(kinds, dtype=np.uint8)
        self._kinds[self._n: self._n + m] = k
        self._payload[self._n: self._n + m] = np.where(k == KIND_NUMBER, np.asarray(numbers, dtype=np.float64).view(np.uint64),
                                                       np.asarray(others, dtype=np.uint64))
        self._n += m

    def compact(self, keep: np.ndarray) -> None:
        """Drops the rows whose `keep` is False, order kept.  The dictionary stays: codes keep their meaning (and the device copy
        its strings), a string no row holds any more simply matches no row."""
        at = np.nonzero(np.asarray(keep, dtype=bool)[: self._n])[0]
        self._kinds, self._payload = self._kinds[: self._n][at].copy(), self._payload[: self._n][at].copy()
        self._n = len(at)

    def string_bytes(self, first: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """The dictionary from code `first` on as the device holds it (vrag_row_filter_append_strings): (uint8 UTF-8 bytes,
        int64 offsets `[codes + 1]` from 0), code `first + i` = bytes[off[i]:off[i + 1]].  Only for an `encodable` column."""
        encoded = [s.encode("utf-8") for s in self.strings[first:]]
        off = np.zeros(len(encoded) + 1, np.int64)
        np.cumsum(np.fromiter(map(len, encoded), np.int64, len(encoded)), out=off[1:])
        return np.frombuffer(b"".join(encoded), np.uint8), off

    def string_table(self, op: str, text: str) -> np.ndarray:
        """`stored <op> text` for every string of the dictionary, as bits: uint32 words, bit `code % 32` of word `code // 32`
        (`len(self.strings)` codes).  The comparison is the operator `parse_filter`'s closure applies."""
        if len(self._tables) >= 256 and (op, text) not in self._tables:
            self._tables.clear()
        answers = self._tables.setdefault((op, text), [])
        if len(answers) < len(self.strings):
            cmp = STRING_COMPARE[op]
            answers.extend(bool(cmp(s, text)) for s in self.strings[len(answers):])
        bits = np.packbits(np.asarray(answers, dtype=bool), bitorder="little")
        words = np.zeros((len(bits) + 3) // 4 * 4, np.uint8)
        words[: len(bits)] = bits
        return words.view(np.uint32)
