"""What `GpuVectorStore` derives from its rows' metadata: value indexes (`==` / `in` lookups), typed columns with their device
copies (`filter_eval="device"`) and group codes with theirs (grouping search).  One object, `StoreMetadata`, with one rule per
event: an insert extends what exists, a compaction compacts the columns and drops the rest, `close()` drops the device copies.
The metadata list itself is the store's row payload; it comes in as an argument.
"""
from __future__ import annotations

import logging
from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np

from .store_columns import MetaColumn
from .store_filter import _typed, compile_filter
from .store_groups import GroupCodes

logger = logging.getLogger(__package__ + ".vector_stores")     # the store's logger: these are the store's log lines


class StoreMetadata:
    """Takes no lock: every method runs under the store's `_mu`.  Calls no collective: a sharded store's ranks hold different
    metadata rows and each derives its own state.  `new_row_filter` / `new_group_column` make the device handles
    (`shards.RowFilter` / `shards.GroupColumn` on the store's device) when the first filter / grouped query needs one."""

    def __init__(self, new_row_filter: Callable[[], Any], new_group_column: Callable[[], Any]):
        self._new_row_filter, self._new_group_column = new_row_filter, new_group_column
        self.value_indexes: Dict[str, Dict[Any, List[np.ndarray]]] = {}   # key -> typed value -> row segments
        # filter_eval="device": typed columns of the keys filters (or grouped queries) have named, host side; the handle that holds
        # their device copies with each key's column number there; the filters already reported as host-routed
        self.columns: Dict[str, MetaColumn] = {}
        self.row_filter = None
        self.row_filter_cols: Dict[str, int] = {}
        self._reported: set = set()
        # grouping search: per key the host group codes (over the key's column in `columns`) and their device copy
        self.group_codes: Dict[str, GroupCodes] = {}
        self.group_cols: Dict[str, Any] = {}

    def extend(self, new_meta: Sequence[Dict[str, Any]], base: int) -> None:
        """The rows `new_meta` were appended to the metadata list at position `base`."""
        # value indexes that exist are extended by the new rows' values (a segment per insert, merged on the next read):
        # rebuilding them is a Python pass over EVERY stored row, per key, after every insert
        for key, index in self.value_indexes.items():
            fresh: Dict[Any, List[int]] = {}
            for j, md in enumerate(new_meta):
                t = _typed(md.get(key))
                if t is not None:
                    fresh.setdefault(t, []).append(base + j)
            for t, rows in fresh.items():
                index.setdefault(t, []).append(np.asarray(rows, dtype=np.int64))
        for column in self.columns.values():      # typed columns likewise: O(new rows) per insert
            column.extend(new_meta)

    def value_index(self, key: str, meta: Sequence[Dict[str, Any]]) -> Dict[Any, np.ndarray]:
        """typed metadata[key] -> rows (positions in the metadata list), built once per key until the next compaction: a
        per-document filter then costs its matches, not a Python predicate call per stored row.  Rows without a
        comparable value are in no bucket."""
        index = self.value_indexes.get(key)
        if index is None:
            buckets: Dict[Any, List[int]] = {}
            for i, md in enumerate(meta):
                t = _typed(md.get(key))
                if t is not None:
                    buckets.setdefault(t, []).append(i)
            index = self.value_indexes[key] = {v: [np.asarray(rows, dtype=np.int64)] for v, rows in buckets.items()}
        out = {}
        for v, segs in index.items():       # buckets are lists of row segments (one per insert since the build): merge on read
            if len(segs) > 1:
                segs[:] = [np.concatenate(segs)]
            out[v] = segs[0]
        return out

    def column(self, key: str, meta: Sequence[Dict[str, Any]]) -> MetaColumn:
        """The typed column of `key`: built by one Python pass over `meta` the first time, extended by every insert afterwards."""
        column = self.columns.get(key)
        if column is None:
            column = self.columns[key] = MetaColumn(key)
            column.extend(meta)
        return column

    def _report_once(self, filter: str, message: str, detail: str) -> None:
        if filter not in self._reported:
            if len(self._reported) >= 1024:
                self._reported.clear()
            self._reported.add(filter)
            logger.info(message, filter, detail)

    def held(self, filter: str, meta: Sequence[Dict[str, Any]], filter_strings: str) -> Optional[np.ndarray]:
        """`filter` over the rows of `meta` on the GPU (`filter_eval="device"`): the filter as a postfix program, the columns it
        names brought up to date in HBM (only rows not uploaded yet travel), its string comparisons resolved against the
        columns' dictionaries, one kernel.  None = this filter is the host's: the program is beyond the device's limits or a
        named column is inexact (logged once per filter string)."""
        program = compile_filter(filter)
        why = program.over_limit()
        columns = []
        for key in program.keys if why is None else ():
            column = self.column(key, meta)
            at = program.keys.index(key)
            pushed = {op for op, i in program.ops if op in ("leaf", "list_any") and program.leaves[i].column == at}
            if "leaf" in pushed and not column.exact:
                why = f"metadata[{key!r}] holds a NaN or a number beyond float range"
                break
            if "list_any" in pushed and not column.list_exact:
                why = f"a list of metadata[{key!r}] holds a NaN or a number beyond float range"
                break
            columns.append((column, pushed))
        if why is not None:
            self._report_once(filter, "GpuVectorStore: filter %r is evaluated on the host: %s", why)
            return None
        if self.row_filter is None:
            self.row_filter = self._new_row_filter()
        device_cols = []
        for column, pushed in columns:
            col = self.row_filter_cols.get(column.key)
            if col is None:
                col = self.row_filter_cols[column.key] = self.row_filter.add_column()
            have = self.row_filter.rows(col)
            if "leaf" in pushed and have < len(column):
                self.row_filter.append(col, column.kinds[have:], column.payload[have:])
            if "list_any" in pushed:        # the list part travels with the first list filter on the key, then per insert
                have, elems = self.row_filter.list_rows(col)
                if have < len(column):
                    self.row_filter.append_lists(col, column.elem_off[have:] - elems, column.elem_kinds[elems:],
                                                 column.elem_payload[elems:])
            device_cols.append((col, column))
        if filter_strings == "host":
            return self.row_filter.eval_program(program, device_cols, len(meta))
        kept: List[str] = []
        held = self.row_filter.eval_program(program, device_cols, len(meta), strings="device", kept=kept)
        if kept:
            self._report_once(filter, "GpuVectorStore: filter %r keeps host tables for: %s", "; ".join(kept))
        return held

    def group_column(self, key: str, meta: Sequence[Dict[str, Any]], n: int):
        """The device group codes of `metadata[key]` for rows `[0, n)` (after a flush): the host codes are built over the key's
        typed column -- the one `filter_eval="device"` keeps, or a new one, extended by every insert either way -- by one pass at
        the first grouped query on the key and by the new rows afterwards; only codes not uploaded yet travel."""
        codes = self.group_codes.get(key)
        if codes is None:
            codes = self.group_codes[key] = GroupCodes(self.column(key, meta))
        host = codes.sync()
        if not codes.column.exact:
            raise ValueError(f"group_by_field: metadata[{key!r}] holds a NaN or a number beyond float range; its rows cannot be grouped")
        device = self.group_cols.get(key)
        if device is None:
            device = self.group_cols[key] = self._new_group_column()
        have = len(device)
        if have < n:
            device.append(host[have:n])
        return device

    def compact(self, keep: np.ndarray) -> None:
        """The rows whose `keep` is False leave: the typed columns and their device copies are compacted where they lie; group
        codes and value indexes are dropped and rebuilt from the surviving rows by the next query that needs them."""
        if self.row_filter is not None:
            self.row_filter.compact(keep)
        for column in self.columns.values():
            column.compact(keep)
        self.group_codes, self.group_cols = {}, {}
        self.value_indexes = {}

    def drop_device(self) -> None:
        """Drops the device copies; the host columns and group codes stay and are uploaded again on demand."""
        self.row_filter, self.row_filter_cols = None, {}
        self.group_cols = {}
