"""Typed metadata columns: one metadata key of every stored row as the arrays the row-filter kernel reads
(include/vrag_amd.h, vrag_row_filter_append).  Host side only -- `shards.RowFilter` holds the device copies.

Per row: `kinds` (uint8: 0 missing / other, 1 number, 2 string, 3 bool) and `payload` (uint64: the f64 bits of a number, the
dictionary code of a string, 0 / 1 of a bool, 0 otherwise).  Kinds and values are `store_filter._typed`'s: bool before int,
numbers as `float(value)`.  Strings are coded in first-seen order; a filter's string comparison is applied once per distinct
string (`string_table`), with Python's own operators, so string ordering is Python's by construction.

The list part (`json_contains`; include/vrag_amd.h, vrag_row_filter_append_lists): the rows whose value is a list (or a tuple) as
CSR -- row r's elements are `elem_off[r] .. elem_off[r + 1]` of `elem_kinds` / `elem_payload`, each element encoded exactly as a
scalar value is, strings through the same dictionary.  Every other row has an empty range, and a list row's scalar kind stays
`KIND_OTHER`.
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
    of a filter that names the key still runs on the device.  `list_exact` is `exact` for the ELEMENTS of the list part (a NaN or an
    out-of-range int inside a list): it sends only list filters on this key to the host -- a scalar comparison never looks inside
    a list, so `exact` stays as it is.  An element string without a UTF-8 form turns `encodable` False: the dictionary is one."""

    def __init__(self, key: str):
        self.key = key
        self.exact = True
        self.encodable = True
        self.strings: List[str] = []                 # code -> string
        self._codes: Dict[str, int] = {}
        self._kinds = np.empty(0, np.uint8)
        self._payload = np.empty(0, np.uint64)
        self._n = 0
        self.list_exact = True
        self._elem_off = np.zeros(1, np.int64)       # [_n + 1] filled
        self._elem_kinds = np.empty(0, np.uint8)
        self._elem_payload = np.empty(0, np.uint64)
        self._n_elems = 0
        self._tables: Dict[Tuple[str, str], List[bool]] = {}   # (op, text) -> answer per code, extended as the dictionary grows

    def __len__(self) -> int:
        return self._n

    @property
    def kinds(self) -> np.ndarray:
        return self._kinds[: self._n]

    @property
    def payload(self) -> np.ndarray:
        return self._payload[: self._n]

    @property
    def elem_off(self) -> np.ndarray:
        """int64 `[len(self) + 1]`, from 0, non-decreasing: row r's elements are `elem_off[r] .. elem_off[r + 1]`."""
        return self._elem_off[: self._n + 1]

    @property
    def elem_kinds(self) -> np.ndarray:
        return self._elem_kinds[: self._n_elems]

    @property
    def elem_payload(self) -> np.ndarray:
        return self._elem_payload[: self._n_elems]

    def extend(self, rows: Iterable[Dict[str, Any]]) -> None:
        """Appends `md.get(key)` of every row: its scalar kind and payload and, for a list, its elements."""
        key, codes, strings = self.key, self._codes, self.strings

        def code_of(text: str) -> int:
            """The dictionary code of a string that has none yet."""
            code = codes[text] = len(strings)
            strings.append(text)
            if self.encodable and not text.isascii():
                try:
                    text.encode("utf-8")
                except UnicodeEncodeError:
                    self.encodable = False
            return code

        kinds: List[int] = []
        numbers: List[float] = []
        others: List[int] = []
        list_at: List[int] = []                        # the rows that hold a list, and how many elements each
        list_len: List[int] = []
        elem_kinds: List[int] = []
        elem_others: List[int] = []                    # code / bool / 0 per element
        number_at: List[int] = []                      # the elements that are numbers, and their values
        number_is: List[float] = []
        for md in rows:                                # row order, elements included: the dictionary's codes are first-seen order
            have = md.get(key)
            try:
                t = _typed(have)
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
                    kind, other = KIND_STRING, code_of(value) if code is None else code
                else:
                    kind, other = KIND_BOOL, int(value)
            elif isinstance(have, (list, tuple)):
                list_at.append(len(kinds))
                list_len.append(len(have))
                for value in have:                     # the same encoding, per element
                    if type(value) is str:
                        code = codes.get(value)
                        elem_kinds.append(KIND_STRING)
                        elem_others.append(code_of(value) if code is None else code)
                        continue
                    try:
                        t = _typed(value)
                    except OverflowError:
                        t, self.list_exact = None, False
                    if t is None:
                        elem_kinds.append(KIND_OTHER)
                        elem_others.append(0)
                    elif t[0] == "n":
                        number_at.append(len(elem_kinds))
                        number_is.append(t[1])
                        elem_kinds.append(KIND_NUMBER)
                        elem_others.append(0)
                        if t[1] != t[1]:
                            self.list_exact = False
                    elif t[0] == "s":                  # a subclass of str
                        code = codes.get(t[1])
                        elem_kinds.append(KIND_STRING)
                        elem_others.append(code_of(t[1]) if code is None else code)
                    else:
                        elem_kinds.append(KIND_BOOL)
                        elem_others.append(int(t[1]))
            kinds.append(kind)
            numbers.append(number)
            others.append(other)
        m, e = len(kinds), len(elem_kinds)
        lens = np.zeros(m, np.int64)
        lens[list_at] = list_len

        def room(names, filled, more):
            if filled + more > len(getattr(self, names[0])):
                cap = max(filled + more, int(len(getattr(self, names[0])) * 1.5) + 16)
                for name in names:
                    grown = np.empty(cap, getattr(self, name).dtype)
                    grown[:filled] = getattr(self, name)[:filled]
                    setattr(self, name, grown)

        room(("_kinds", "_payload"), self._n, m)
        k = np.asarray(kinds, dtype=np.uint8)
        self._kinds[self._n: self._n + m] = k
        self._payload[self._n: self._n + m] = np.where(k == KIND_NUMBER, np.asarray(numbers, dtype=np.float64).view(np.uint64),
                                                       np.asarray(others, dtype=np.uint64))
        room(("_elem_kinds", "_elem_payload"), self._n_elems, e)
        self._elem_kinds[self._n_elems: self._n_elems + e] = np.asarray(elem_kinds, dtype=np.uint8)
        payload = np.asarray(elem_others, dtype=np.uint64)
        payload[number_at] = np.asarray(number_is, dtype=np.float64).view(np.uint64)
        self._elem_payload[self._n_elems: self._n_elems + e] = payload
        room(("_elem_off",), self._n + 1, m)
        np.cumsum(lens, out=self._elem_off[self._n + 1: self._n + 1 + m])
        self._elem_off[self._n + 1: self._n + 1 + m] += self._n_elems
        self._n += m
        self._n_elems += e

    def compact(self, keep: np.ndarray) -> None:
        """Drops the rows whose `keep` is False, order kept.  The dictionary stays: codes keep their meaning (and the device copy
        its strings), a string no row holds any more simply matches no row."""
        at = np.nonzero(np.asarray(keep, dtype=bool)[: self._n])[0]
        self._kinds, self._payload = self._kinds[: self._n][at].copy(), self._payload[: self._n][at].copy()
        # the list part: the kept rows' element ranges, offsets re-based
        old = self.elem_off
        lens = old[at + 1] - old[at]
        off = np.zeros(len(at) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        take = np.repeat(old[at] - off[:-1], lens) + np.arange(int(off[-1]), dtype=np.int64)
        self._elem_kinds, self._elem_payload = self.elem_kinds[take], self.elem_payload[take]
        self._elem_off, self._n_elems = off, int(off[-1])
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
