"""Group codes of a metadata key: what a grouping search (`search_params={"group_by_field": ...}`) groups by.  Host side only --
`shards.GroupColumn` holds the device copy (include/vrag_amd.h, vrag_group_column_append).

A row's group is the `store_filter._typed` value of `metadata[key]`, read off the key's `store_columns.MetaColumn`: the pair
(kind, payload) with -0.0 folded into 0.0 -- so `2020` and `2020.0` are one group (both are the number 2020.0), `"5"` and `5` are
two, `True` is not `1`.  Rows without the key, or with None, a list or a dict (kind "other"), all share code 0, "no value".
Every other distinct value gets the next code in first-seen order, so the codes are dense: 1 .. number of values.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from .store_columns import KIND_NUMBER, KIND_OTHER, MetaColumn

NO_VALUE = 0                      # the code of the "no value" group
_MINUS_ZERO = np.uint64(0x8000000000000000)
_PAIR = np.dtype([("kind", np.uint8), ("payload", np.uint64)])


class GroupCodes:
    """int32 code per row of one `MetaColumn`, built by one pass over the column at the first grouped query on its key and
    extended by the column's new rows afterwards (`sync`: O(new rows)).  Dropped, not compacted, when the store compacts."""

    def __init__(self, column: MetaColumn):
        self.column = column
        self._code_of: Dict[Tuple[int, int], int] = {}     # (kind, payload) -> code, first-seen order from 1
        self._codes = np.empty(0, np.int32)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    @property
    def codes(self) -> np.ndarray:
        return self._codes[: self._n]

    @property
    def n_codes(self) -> int:
        """Largest code + 1 (the "no value" code included, whether a row holds it or not)."""
        return len(self._code_of) + 1

    def sync(self) -> np.ndarray:
        """Codes for the rows the column has gained since the last call; returns all codes."""
        column, done = self.column, self._n
        m = len(column) - done
        if m <= 0:
            return self.codes
        pairs = np.empty(m, _PAIR)
        kinds = column.kinds[done:]
        payload = column.payload[done:].copy()
        payload[(kinds == KIND_NUMBER) & (payload == _MINUS_ZERO)] = 0      # -0.0 == 0.0
        payload[kinds == KIND_OTHER] = 0
        pairs["kind"], pairs["payload"] = kinds, payload
        distinct, first, inverse = np.unique(pairs, return_index=True, return_inverse=True)
        code = np.empty(len(distinct), np.int32)
        for u in np.argsort(first, kind="stable").tolist():                   # first-seen order among the new rows
            kind, value = int(distinct["kind"][u]), int(distinct["payload"][u])
            code[u] = NO_VALUE if kind == KIND_OTHER else self._code_of.setdefault((kind, value), len(self._code_of) + 1)
        if done + m > len(self._codes):
            grown = np.empty(max(done + m, int(len(self._codes) * 1.5) + 16), np.int32)
            grown[:done] = self._codes[:done]
            self._codes = grown
        self._codes[done: done + m] = code[inverse.reshape(-1)]
        self._n = done + m
        return self.codes
