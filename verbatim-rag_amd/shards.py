"""The device indexes of the vector store as Python objects: ctypes wrappers around the library's handles
(include/vrag_amd.h, vrag_dense_index_* / vrag_ivf_index_* / vrag_sparse_index_* / vrag_text_index_*) and the host-side
packing their calls need (CSR, UTF-8 batches, row bitmaps).  The store-side module that touches `ctypes`; vector_stores.py
holds the store that routes searches to these objects.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

_FP = C.POINTER(C.c_float)
_LP = C.POINTER(C.c_int64)
_IP = C.POINTER(C.c_int32)


def _fp(a: np.ndarray):       # like every `data_as` pointer, the result keeps its array alive
    return a.ctypes.data_as(_FP)


def _lp(a: np.ndarray):
    return a.ctypes.data_as(_LP)


def _ip(a: np.ndarray):
    return a.ctypes.data_as(_IP)


def _vp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _topk_out(nq: int, k: int, fill: bool = False):
    """The `[nq, k]` outputs of a search and their ctypes pointers: (float32 scores, int64 ids, scores ptr, ids ptr).
    Uninitialised where the library writes every slot; `fill=True` starts from "no hit" (-inf / -1) for the calls that may
    write fewer (`TextIndex`)."""
    if fill:
        scores, ids = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)
    else:
        scores, ids = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
    return scores, ids, _fp(scores), _lp(ids)


class _Handle:
    """Owner of one library handle: `_open` creates it, `close` destroys it once, and an object whose constructor failed
    (before or inside `_open`) is collected quietly."""

    _destroy = ""       # name of the library function that frees `_h`
    _lib = None
    _h = None

    def _open(self, create: str, *args) -> None:
        """`create(*args, &handle)`; a failed call leaves the handle null."""
        self._lib = _lib.load()
        self._h = C.c_void_p()
        _lib.check(create, getattr(self._lib, create)(*args, C.byref(self._h)))

    def close(self):
        if self._h:
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _allow_words(allow_words, n_allow: int) -> np.ndarray:
    """The bitmap of a filtered search as contiguous uint32 words; ValueError when it is shorter than `n_allow` rows (the
    library would read past it)."""
    words = np.ascontiguousarray(allow_words, dtype=np.uint32).reshape(-1)
    if n_allow < 0 or len(words) * 32 < n_allow:
        raise ValueError(f"allow_words holds {len(words) * 32} bits, n_allow = {n_allow}")
    return words


def _search_call(lib, fn: str, head: tuple, nq: int, k: int, allow, stream) -> Tuple[np.ndarray, np.ndarray]:
    """`fn(*head, nq, k, scores, ids, stream)`, or with `allow = (allow_words, n_allow)` the `_filtered` entry point, which
    takes the bitmap and its row count before the outputs."""
    if allow is not None:
        fn += "_filtered"
        allow = (_vp(_allow_words(*allow)), int(allow[1]))
    scores, ids, sp, ip = _topk_out(nq, k)
    _lib.check(fn, getattr(lib, fn)(*head, nq, k, *(allow or ()), sp, ip, stream))
    return scores, ids


def _compact_call(lib, fn: str, handle, keep: np.ndarray) -> int:
    """`fn(handle, keep bitmap, len(keep), &new_size)` -> new size."""
    keep = np.asarray(keep, dtype=bool).reshape(-1)
    words, new_size = _bitmap(keep), C.c_int64()
    _lib.check(fn, getattr(lib, fn)(handle, _vp(words) if len(words) else None, len(keep), C.byref(new_size)))
    return new_size.value


class DenseShard(_Handle):
    """One GPU's slice of the dense corpus (rows appended in order; ids are local row numbers)."""

    _destroy = "vrag_dense_index_destroy"

    def __init__(self, dim: int, capacity: int, dtype: str = "bf16", device: int = 0, prefilter: bool = True):
        """dtype "bf16" | "f32".  fp32 rows keep a bf16 prefilter image beside them unless `prefilter=False` (+50 % memory):
        a search ranks the image for 64 candidates per query and re-scores those exactly -- same bits as the full fp32 scan
        (include/vrag_amd.h, dtype 2), half the time for one query and a quarter for a batch of 256."""
        _lib.require_gpu()
        self.dim, self.capacity = dim, capacity
        self.ivf: Optional["IvfOverlay"] = None    # an IVF_FLAT overlay over these rows (owned: closed before the shard)
        code = 0 if dtype == "bf16" else (2 if prefilter and dim % 4 == 0 else 1)
        self._open("vrag_dense_index_create", dim, capacity, code, device)

    def add(self, rows: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        _lib.check("vrag_dense_index_add", self._lib.vrag_dense_index_add(self._h, _fp(rows), rows.shape[0]))

    def add_device(self, ptr: int, n: int, stream=None) -> None:
        """Rows already in HBM (`ptr`: device address of fp32 `[n, dim]` on the shard's device): no host round trip."""
        _lib.check("vrag_dense_index_add_device", self._lib.vrag_dense_index_add_device(self._h, C.c_void_p(int(ptr)), int(n), stream))

    def __len__(self) -> int:
        return int(self._lib.vrag_dense_index_size(self._h))

    def _queries(self, queries: np.ndarray) -> np.ndarray:
        return np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)

    def _search(self, queries, k: int, allow, stream):
        q = self._queries(queries)
        return _search_call(self._lib, "vrag_dense_index_search", (self._h, _fp(q)), q.shape[0], k, allow, stream)

    def search(self, queries: np.ndarray, k: int, stream=None) -> Tuple[np.ndarray, np.ndarray]:
        return self._search(queries, k, None, stream)

    def search_filtered(self, queries: np.ndarray, k: int, allow_words: np.ndarray, n_allow: int,
                        stream=None) -> Tuple[np.ndarray, np.ndarray]:
        """`search` over the rows `r < min(n_allow, len(self))` whose bit is set in `allow_words` (uint32, bit `r % 32` of
        word `r // 32`, as `_bitmap` packs them): exact chains over the passing rows only (`vrag_dense_index_search_filtered`)."""
        return self._search(queries, k, (allow_words, n_allow), stream)

    def search_grouped(self, queries: np.ndarray, n_groups: int, group_size: int, column: "GroupColumn",
                       allow_words: Optional[np.ndarray] = None, n_allow: int = 0,
                       stream=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Grouping search (`vrag_dense_index_search_grouped`): per query the best `n_groups` groups of `column` among the rows
        `r < min(len(self), len(column))` -- with `allow_words` those below `n_allow` whose bit is set -- each with its best
        `group_size` rows.  Returns (scores float32 `[Q, n_groups, group_size]`, ids int64 likewise, groups int32
        `[Q, n_groups]`); missing entries are -inf / -1 / -1."""
        q = self._queries(queries)
        nq = q.shape[0]
        allow = (None, 0) if allow_words is None else (_vp(_allow_words(allow_words, n_allow)), int(n_allow))
        scores = np.empty((nq, n_groups, group_size), np.float32)
        ids = np.empty((nq, n_groups, group_size), np.int64)
        groups = np.empty((nq, n_groups), np.int32)
        _lib.check("vrag_dense_index_search_grouped", self._lib.vrag_dense_index_search_grouped(
            self._h, _fp(q), nq, int(n_groups), int(group_size), column._h, *allow, _fp(scores), _lp(ids), _ip(groups), stream))
        return scores, ids, groups

    def search_device(self, queries: np.ndarray, k: int, out_scores: int, out_ids: int, row_map: Optional[int] = None,
                      n_map: int = 0, id_base: int = 0, stream=None) -> None:
        """The same search with the `[Q, k]` lists left in HBM at the device addresses `out_scores` / `out_ids`
        (global ids through the device table `row_map`, or `id_base + row`); kernels are only enqueued on `stream`."""
        q = self._queries(queries)
        _lib.check("vrag_dense_index_search_device", self._lib.vrag_dense_index_search_device(
            self._h, _fp(q), q.shape[0], k, C.c_void_p(row_map) if row_map else None, n_map, id_base,
            C.c_void_p(out_scores), C.c_void_p(out_ids), stream))

    def run_resident(self, nq: int, k: int, stream=None) -> None:
        _lib.check("vrag_dense_index_run_resident", self._lib.vrag_dense_index_run_resident(self._h, nq, k, stream))

    def compact(self, keep: np.ndarray) -> int:
        """Drops the rows whose `keep` (bool per row, `len(self)` of them) is False, in place in HBM, order kept
        (`vrag_dense_index_compact`); returns the new size.  An IVF overlay is renumbered with `IvfOverlay.remap(keep)` afterwards."""
        return _compact_call(self._lib, "vrag_dense_index_compact", self._h, keep)

    def read(self, first_row: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Rows `[first_row, first_row + n)` as float32 `[n, dim]` (bf16 rows widened); `n=None`: up to the end."""
        n = len(self) - first_row if n is None else int(n)
        out = np.empty((max(n, 0), self.dim), np.float32)
        _lib.check("vrag_dense_index_read", self._lib.vrag_dense_index_read(self._h, int(first_row), n, _fp(out)))
        return out

    def close(self):
        ivf, self.ivf = getattr(self, "ivf", None), None
        if ivf is not None:
            ivf.close()
        super().close()


class GroupColumn(_Handle):
    """One int32 group code (>= 0) per row of a `DenseShard`, in HBM (`vrag_group_column`): what `DenseShard.search_grouped`
    groups by.  Appended to in row order; owns the scratch of the searches made with it."""

    _destroy = "vrag_group_column_destroy"

    def __init__(self, device: int = 0):
        _lib.require_gpu()
        self._open("vrag_group_column_create", int(device))

    def append(self, codes: np.ndarray) -> None:
        codes = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
        _lib.check("vrag_group_column_append", self._lib.vrag_group_column_append(self._h, _ip(codes) if len(codes) else None, len(codes)))

    def __len__(self) -> int:
        return int(self._lib.vrag_group_column_size(self._h))


class Sq8Shard(_Handle):
    """One GPU's slice of the dense corpus as SQ8 rows (`vrag_sq8_index`, include/vrag_amd.h "SQ8 dense rows"): int8 codes
    and one fp32 scale per row, int8 queries, integer-exact scores.  The call shapes are `DenseShard`'s."""

    _destroy = "vrag_sq8_index_destroy"
    ivf = None    # an instance may own an IVF_SQ8 overlay over its rows (`IvfOverlay`: closed before the shard)

    def __init__(self, dim: int, capacity: int, device: int = 0):
        _lib.require_gpu()
        self.dim, self.capacity = dim, capacity
        self.ivf: Optional["IvfOverlay"] = None
        self._open("vrag_sq8_index_create", dim, capacity, device)

    def add(self, rows: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        _lib.check("vrag_sq8_index_add", self._lib.vrag_sq8_index_add(self._h, _fp(rows), rows.shape[0]))

    def add_device(self, ptr: int, n: int, stream=None) -> None:
        """Rows already in HBM (`ptr`: device address of fp32 `[n, dim]` on the shard's device), quantised there."""
        _lib.check("vrag_sq8_index_add_device", self._lib.vrag_sq8_index_add_device(self._h, C.c_void_p(int(ptr)), int(n), stream))

    def __len__(self) -> int:
        return int(self._lib.vrag_sq8_index_size(self._h))

    def read(self, first_row: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(codes int8 `[n, dim]`, scales float32 `[n]`) of rows `[first_row, first_row + n)`; `n=None`: up to the end."""
        n = len(self) - first_row if n is None else int(n)
        codes, scales = np.empty((max(n, 0), self.dim), np.int8), np.empty(max(n, 0), np.float32)
        _lib.check("vrag_sq8_index_read", self._lib.vrag_sq8_index_read(self._h, int(first_row), n, _vp(codes), _vp(scales)))
        return codes, scales

    def compact(self, keep: np.ndarray) -> int:
        """`DenseShard.compact` for SQ8 rows: codes and scales move in place (`vrag_sq8_index_compact`); returns the new size."""
        return _compact_call(self._lib, "vrag_sq8_index_compact", self._h, keep)

    def set_route(self, route: int) -> None:
        """0 = automatic, 1 = scan kernel, 2 = tile kernel: the same bits either way (a unit-test and tuning knob)."""
        _lib.check("vrag_sq8_index_set_route", self._lib.vrag_sq8_index_set_route(self._h, int(route)))

    def _search(self, queries, k: int, allow, stream):
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        return _search_call(self._lib, "vrag_sq8_index_search", (self._h, _fp(q)), q.shape[0], k, allow, stream)

    def search(self, queries: np.ndarray, k: int, stream=None) -> Tuple[np.ndarray, np.ndarray]:
        return self._search(queries, k, None, stream)

    def search_filtered(self, queries: np.ndarray, k: int, allow_words: np.ndarray, n_allow: int,
                        stream=None) -> Tuple[np.ndarray, np.ndarray]:
        """`search` over the rows `r < min(n_allow, len(self))` whose bit is set in `allow_words` (see
        `DenseShard.search_filtered`): the search kernels skip the other rows (`vrag_sq8_index_search_filtered`)."""
        return self._search(queries, k, (allow_words, n_allow), stream)

    def close(self):
        ivf, self.ivf = getattr(self, "ivf", None), None
        if ivf is not None:
            ivf.close()
        super().close()


class PqShard(_Handle):
    """One GPU's slice of the dense corpus as PQ rows (`vrag_pq_index`, include/vrag_amd.h "PQ dense rows"): `m` code bytes per
    row, scored through a per-query look-up table.  The call shapes are `DenseShard`'s, plus the codebooks: a new shard has none
    and refuses rows and searches until `train` or `set_codebooks` has run; they are frozen once it holds rows."""

    _destroy = "vrag_pq_index_destroy"
    ivf = None    # no overlay over PQ rows (the attribute the store's search path reads on every dense shard)

    def __init__(self, dim: int, m: int, capacity: int, device: int = 0):
        _lib.require_gpu()
        self.dim, self.m, self.capacity = dim, int(m), capacity
        self._open("vrag_pq_index_create", dim, self.m, capacity, device)

    def _rows(self, rows: np.ndarray) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        return rows

    def train(self, rows: np.ndarray, iters: int = 10) -> None:
        """Lloyd's k-means per sub-space over the sample `rows` (deterministic: no random numbers, `vrag_pq_index_train`)."""
        rows = self._rows(rows)
        _lib.check("vrag_pq_index_train", self._lib.vrag_pq_index_train(self._h, _fp(rows), rows.shape[0], int(iters)))

    def set_codebooks(self, codebooks: np.ndarray) -> None:
        cb = np.ascontiguousarray(codebooks, dtype=np.float32)
        if cb.shape != (self.m, 256, self.dim // self.m):
            raise ValueError(f"codebooks must be [{self.m}, 256, {self.dim // self.m}]")
        _lib.check("vrag_pq_index_set_codebooks", self._lib.vrag_pq_index_set_codebooks(self._h, _fp(cb)))

    def codebooks(self) -> np.ndarray:
        """float32 `[m, 256, dim // m]`, the bytes in place."""
        cb = np.empty((self.m, 256, self.dim // self.m), np.float32)
        _lib.check("vrag_pq_index_read_codebooks", self._lib.vrag_pq_index_read_codebooks(self._h, _fp(cb)))
        return cb

    def add(self, rows: np.ndarray) -> None:
        rows = self._rows(rows)
        _lib.check("vrag_pq_index_add", self._lib.vrag_pq_index_add(self._h, _fp(rows), rows.shape[0]))

    def add_device(self, ptr: int, n: int, stream=None) -> None:
        """Rows already in HBM (`ptr`: device address of fp32 `[n, dim]` on the shard's device), encoded there."""
        _lib.check("vrag_pq_index_add_device", self._lib.vrag_pq_index_add_device(self._h, C.c_void_p(int(ptr)), int(n), stream))

    def __len__(self) -> int:
        return int(self._lib.vrag_pq_index_size(self._h))

    def read(self, first_row: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Codes uint8 `[n, m]` of rows `[first_row, first_row + n)`; `n=None`: up to the end."""
        n = len(self) - first_row if n is None else int(n)
        codes = np.empty((max(n, 0), self.m), np.uint8)
        _lib.check("vrag_pq_index_read", self._lib.vrag_pq_index_read(self._h, int(first_row), n, _vp(codes)))
        return codes

    def compact(self, keep: np.ndarray) -> int:
        """`DenseShard.compact` for PQ rows: the codes move in place (`vrag_pq_index_compact`); returns the new size."""
        return _compact_call(self._lib, "vrag_pq_index_compact", self._h, keep)

    def _search(self, queries, k: int, allow, stream):
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        return _search_call(self._lib, "vrag_pq_index_search", (self._h, _fp(q)), q.shape[0], k, allow, stream)

    def search(self, queries: np.ndarray, k: int, stream=None) -> Tuple[np.ndarray, np.ndarray]:
        return self._search(queries, k, None, stream)

    def search_filtered(self, queries: np.ndarray, k: int, allow_words: np.ndarray, n_allow: int,
                        stream=None) -> Tuple[np.ndarray, np.ndarray]:
        """`search` over the rows `r < min(n_allow, len(self))` whose bit is set in `allow_words` (see
        `DenseShard.search_filtered`): the scan skips the other rows (`vrag_pq_index_search_filtered`)."""
        return self._search(queries, k, (allow_words, n_allow), stream)


class IvfOverlay(_Handle):
    """IVF lists over a shard's resident rows (`vrag_ivf_index`): centroids, list offsets and row numbers only -- IVF_FLAT over
    a `DenseShard`, IVF_SQ8 over an `Sq8Shard` (`vrag_ivf_index_create_sq8`: the rows are scored by the SQ8 rule).
    The shard must outlive it (the shard's `ivf` owns it and closes it first)."""

    _destroy = "vrag_ivf_index_destroy"

    def __init__(self, shard: "DenseShard | Sq8Shard", nlist: int):
        self.dim, self.nlist = shard.dim, int(nlist)
        self._open("vrag_ivf_index_create_sq8" if isinstance(shard, Sq8Shard) else "vrag_ivf_index_create", shard._h, self.nlist)

    def set_centroids(self, centroids: np.ndarray) -> None:
        c = np.ascontiguousarray(centroids, dtype=np.float32)
        if c.shape != (self.nlist, self.dim):
            raise ValueError(f"centroids must be [{self.nlist}, {self.dim}]")
        _lib.check("vrag_ivf_index_set_centroids", self._lib.vrag_ivf_index_set_centroids(self._h, _fp(c)))

    def train(self, iters: int = 10, max_train_rows: int = 1 << 62) -> None:
        _lib.check("vrag_ivf_index_train", self._lib.vrag_ivf_index_train(self._h, int(iters), int(max_train_rows)))

    def sync(self) -> None:
        _lib.check("vrag_ivf_index_sync", self._lib.vrag_ivf_index_sync(self._h))

    def stats(self) -> Dict[str, int]:
        nlist, n, largest = C.c_int32(), C.c_int64(), C.c_int64()
        _lib.check("vrag_ivf_index_stats", self._lib.vrag_ivf_index_stats(self._h, C.byref(nlist), C.byref(n), C.byref(largest)))
        return {"nlist": nlist.value, "rows": n.value, "largest_list": largest.value}

    def read(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(centroids `[nlist, dim]`, list_off `[nlist + 1]`, list_rows `[rows]`) after a `sync`."""
        cent = np.empty((self.nlist, self.dim), np.float32)
        off = np.empty(self.nlist + 1, np.uint32)
        rows = np.empty(self.stats()["rows"], np.uint32)
        _lib.check("vrag_ivf_index_read", self._lib.vrag_ivf_index_read(self._h, _fp(cent), _vp(off), _vp(rows) if len(rows) else None))
        return cent, off, rows

    def remap(self, keep: np.ndarray) -> None:
        """After `compact(keep)` of the shard (`DenseShard` or `Sq8Shard`), with the same `keep`: the lists' rows are renumbered, dropped rows
        leave their lists, the centroids stay (`vrag_ivf_index_remap`)."""
        keep = np.asarray(keep, dtype=bool).reshape(-1)
        words = _bitmap(keep)
        _lib.check("vrag_ivf_index_remap", self._lib.vrag_ivf_index_remap(self._h, _vp(words) if len(words) else None, len(keep)))

    def search(self, queries: np.ndarray, k: int, nprobe: int, stream=None, scanned: bool = False):
        """(scores `[Q, k]`, ids `[Q, k]`) -- exact scores of the best rows of the `nprobe` nearest lists; with
        `scanned=True` also the rows each query's lists hold."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        scores, ids, sp, ip = _topk_out(q.shape[0], k)
        seen = np.empty(q.shape[0], np.int64) if scanned else None
        _lib.check("vrag_ivf_index_search", self._lib.vrag_ivf_index_search(
            self._h, _fp(q), q.shape[0], k, int(nprobe), sp, ip, _lp(seen) if scanned else None, stream))
        return (scores, ids, seen) if scanned else (scores, ids)


class RowFilter(_Handle):
    """Typed metadata columns in HBM and the kernel that evaluates a filter program over them (`vrag_row_filter_*`,
    csrc/rowfilter.hip): 9 bytes per row and column.  Columns are numbered in creation order and only ever appended to.
    A column may also hold the dictionary of its strings (`append_strings`); the match kernel (csrc/strmatch.hip) then makes
    the answer table of a string comparison or a `LIKE` from it (`match`, `eval_program(strings="device")`).  And the list part
    of its rows (`append_lists`: 8 bytes per row + 9 per element), which the "list_any" op of a program reads (`json_contains`,
    csrc/listfilter.hip); `compact` drops the list parts, the caller appends them again."""

    _destroy = "vrag_row_filter_destroy"

    def __init__(self, device: int = 0):
        _lib.require_gpu()
        self._open("vrag_row_filter_create", int(device))

    def add_column(self) -> int:
        col = C.c_int32()
        _lib.check("vrag_row_filter_add_column", self._lib.vrag_row_filter_add_column(self._h, C.byref(col)))
        return col.value

    def append(self, col: int, kinds: np.ndarray, payload: np.ndarray) -> None:
        kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
        payload = np.ascontiguousarray(payload, dtype=np.uint64)
        if kinds.ndim != 1 or kinds.shape != payload.shape:
            raise ValueError(f"kinds {kinds.shape} and payload {payload.shape} must be one-dimensional and equally long")
        _lib.check("vrag_row_filter_append", self._lib.vrag_row_filter_append(self._h, int(col), _vp(kinds), _vp(payload), len(kinds)))

    def rows(self, col: int) -> int:
        n = C.c_int64()
        _lib.check("vrag_row_filter_rows", self._lib.vrag_row_filter_rows(self._h, int(col), C.byref(n)))
        return n.value

    def append_lists(self, col: int, elem_off: np.ndarray, elem_kinds: np.ndarray, elem_payload: np.ndarray) -> None:
        """Appends `len(elem_off) - 1` rows to the column's list part: row i holds elements elem_off[i]:elem_off[i + 1] of
        `elem_kinds` / `elem_payload`, elem_off[0] = 0; the device continues its offsets from the elements it holds
        (`store_columns.MetaColumn.elem_off` of the new rows, less its first entry)."""
        elem_off = np.ascontiguousarray(elem_off, dtype=np.int64)
        elem_kinds = np.ascontiguousarray(elem_kinds, dtype=np.uint8)
        elem_payload = np.ascontiguousarray(elem_payload, dtype=np.uint64)
        if elem_off.ndim != 1 or len(elem_off) < 1 or elem_kinds.ndim != 1 or elem_kinds.shape != elem_payload.shape or \
                int(elem_off[-1]) > len(elem_kinds):
            raise ValueError(f"elem_off {elem_off.shape} must hold one offset more than rows and end inside the equally long "
                             f"elem_kinds {elem_kinds.shape} and elem_payload {elem_payload.shape}")
        _lib.check("vrag_row_filter_append_lists", self._lib.vrag_row_filter_append_lists(
            self._h, int(col), _vp(elem_off), _vp(elem_kinds) if len(elem_kinds) else None,
            _vp(elem_payload) if len(elem_payload) else None, len(elem_off) - 1))

    def list_rows(self, col: int) -> Tuple[int, int]:
        """(rows, elements) of the column's list part on the device."""
        n, e = C.c_int64(), C.c_int64()
        _lib.check("vrag_row_filter_list_rows", self._lib.vrag_row_filter_list_rows(self._h, int(col), C.byref(n), C.byref(e)))
        return n.value, e.value

    def compact(self, keep: np.ndarray) -> None:
        """Drops the rows whose `keep` is False from every column, in place, order kept (`vrag_row_filter_compact`); a column
        that holds fewer rows than `keep` covers is compacted under its prefix.  The dictionaries stay.  When a row is dropped
        the list parts are dropped whole (`list_rows` = (0, 0)): append them again from the compacted host columns."""
        keep = np.asarray(keep, dtype=bool).reshape(-1)
        words = _bitmap(keep)
        _lib.check("vrag_row_filter_compact", self._lib.vrag_row_filter_compact(self._h, _vp(words) if len(words) else None, len(keep)))

    def append_strings(self, col: int, data: np.ndarray, off: np.ndarray) -> None:
        """Appends strings to the column's dictionary: string i = the UTF-8 bytes data[off[i]:off[i + 1]], off[0] = 0; codes
        continue from those held (`store_columns.MetaColumn.string_bytes`)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1 or data.ndim != 1 or (len(off) > 1 and int(off[-1]) > len(data)):
            raise ValueError(f"off {off.shape} must hold one offset more than strings and end inside the {len(data)} bytes")
        _lib.check("vrag_row_filter_append_strings", self._lib.vrag_row_filter_append_strings(
            self._h, int(col), _vp(data) if len(data) else None, _vp(off), len(off) - 1))

    def strings(self, col: int) -> Tuple[int, int]:
        """(codes, bytes) of the column's dictionary on the device."""
        n, b = C.c_int64(), C.c_int64()
        _lib.check("vrag_row_filter_strings", self._lib.vrag_row_filter_strings(self._h, int(col), C.byref(n), C.byref(b)))
        return n.value, b.value

    def match(self, col: int, op: str, text: str, n_codes: Optional[int] = None, out: Optional[np.ndarray] = None,
              column=None, stream=None) -> np.ndarray:
        """`stored <op> text` for codes [0, n_codes) of the column's device dictionary (default: all of it) as the words of
        `MetaColumn.string_table`; op one of == != < <= > >= like.  The kernel's limits are the library's
        (`match_on_device`): a text beyond them raises VragError, unless `column` (the `MetaColumn` of the same dictionary) is
        given -- then the host table answers, as it does for such a leaf in `eval_program`."""
        n = self.strings(col)[0] if n_codes is None else int(n_codes)
        n_words = (max(0, n) + 31) // 32
        if out is None:
            out = np.zeros(n_words, np.uint32)
        elif out.dtype != np.uint32 or not out.flags.c_contiguous or len(out) < n_words:
            raise ValueError(f"out must be a contiguous uint32 array of at least {n_words} words")
        if column is not None and match_on_device(op, text) is not None:
            if n < 0 or n > len(column.strings):
                raise ValueError(f"n_codes = {n} but the column holds {len(column.strings)} strings")
            answers = np.unpackbits(column.string_table(op, text).view(np.uint8), bitorder="little")[:n]
            out[:n_words] = _bitmap(answers)[:n_words]                   # the prefix's words, tail bits zero
            return out
        raw = text.encode("utf-8", "surrogatepass")          # what cannot be UTF-8 is the library's to refuse
        _lib.check("vrag_row_filter_match", self._lib.vrag_row_filter_match(
            self._h, int(col), _lib.FILTER_MATCH_OPS[op], raw, len(raw), n, _vp(out), stream))
        return out

    def eval(self, leaves: Sequence["_lib.FilterLeaf"], ops: np.ndarray, tables: np.ndarray, n_rows: int,
             out: Optional[np.ndarray] = None, stream=None, matches: Sequence["_lib.FilterMatch"] = (), texts: bytes = b"") -> np.ndarray:
        """The program's answer for rows [0, n_rows) as uint32 words (bit r % 32 of word r // 32, tail bits zero).  `out`: a
        uint32 array of at least ceil(n_rows / 32) words to write into (words behind those are left alone).  `matches`: table
        leaves whose tables the match kernel writes on the device before the program runs, their operand texts in `texts`
        (vrag_row_filter_eval_matched).  A program with a "list_any" op goes to vrag_row_filter_eval_lists, every other one to
        the entry point it always went to."""
        arr = (_lib.FilterLeaf * max(1, len(leaves)))(*leaves)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        tables = np.ascontiguousarray(tables, dtype=np.uint32)
        n_words = (max(0, int(n_rows)) + 31) // 32
        if out is None:
            out = np.zeros(n_words, np.uint32)
        elif out.dtype != np.uint32 or not out.flags.c_contiguous or len(out) < n_words:
            raise ValueError(f"out must be a contiguous uint32 array of at least {n_words} words")
        if len(ops) and bool(((ops & 0xFF) == _lib.FILTER_OPS["list_any"]).any()):
            _lib.check("vrag_row_filter_eval_lists", self._lib.vrag_row_filter_eval_lists(
                self._h, arr, len(leaves), _vp(ops), len(ops), _vp(tables) if len(tables) else None, len(tables),
                (_lib.FilterMatch * max(1, len(matches)))(*matches), len(matches), texts, len(texts), int(n_rows), _vp(out), stream))
            return out
        if len(matches):
            _lib.check("vrag_row_filter_eval_matched", self._lib.vrag_row_filter_eval_matched(
                self._h, arr, len(leaves), _vp(ops), len(ops), _vp(tables) if len(tables) else None, len(tables),
                (_lib.FilterMatch * len(matches))(*matches), len(matches), texts, len(texts), int(n_rows), _vp(out), stream))
            return out
        _lib.check("vrag_row_filter_eval", self._lib.vrag_row_filter_eval(
            self._h, arr, len(leaves), _vp(ops), len(ops), _vp(tables) if len(tables) else None, len(tables), int(n_rows),
            _vp(out), stream))
        return out

    def eval_program(self, program, columns: Sequence[Tuple[int, "object"]], n_rows: int, strings: str = "host",
                     kept: Optional[List[str]] = None) -> np.ndarray:
        """`bool[n_rows]` of a `store_filter.FilterProgram`; `columns[i]` = (this filter's column number, the
        `store_columns.MetaColumn` whose dictionary resolves the string leaves) of `program.keys[i]`.
        `strings`: who makes the tables of the string leaves -- "host" (default) `MetaColumn.string_table`, once per distinct
        string in Python; "device" the match kernel, over the columns' dictionaries in HBM (brought up to date here: only codes
        not uploaded yet travel).  A leaf the kernel cannot take -- its text beyond a limit or not encodable, its column
        holding a string without a UTF-8 form -- gets a host table inside the same call; `kept` (a list) receives one sentence
        per such leaf."""
        if strings not in ("host", "device"):
            raise ValueError(f"strings must be 'host' or 'device' (got {strings!r})")
        if strings == "host":
            leaves, ops, tables = program_arrays(program, columns)
            words = self.eval(leaves, ops, tables, n_rows)
            return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_rows].astype(bool)
        for col, meta in {c: (c, m) for c, m in columns}.values():
            have = self.strings(col)[0]
            if meta.encodable and have < len(meta.strings):
                self.append_strings(col, *meta.string_bytes(have))
        leaves, ops, tables, matches, texts = program_arrays(program, columns, device_strings=True, kept=kept)
        words = self.eval(leaves, ops, tables, n_rows, matches=matches, texts=texts)
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_rows].astype(bool)


def match_on_device(op: str, text: str) -> Optional[str]:
    """Why the match kernel cannot take (`op`, `text`) -- one sentence -- or None when it can (VRAG_FILTER_MATCH_MAX_*)."""
    from .store_filter import like_segments

    try:
        raw = text.encode("utf-8")
    except UnicodeEncodeError:
        return f"the text {text[:40]!r} has no UTF-8 form"
    if len(raw) > _lib.FILTER_MATCH_MAX_PATTERN:
        return f"the text {text[:40]!r}... has {len(raw)} bytes (the match kernel takes {_lib.FILTER_MATCH_MAX_PATTERN})"
    if op == "like" and like_segments(text) > _lib.FILTER_MATCH_MAX_SEGMENTS:
        return f"the pattern {text[:40]!r}... has {like_segments(text)} segments between its % (the match kernel takes " \
               f"{_lib.FILTER_MATCH_MAX_SEGMENTS})"
    return None


def program_arrays(program, columns: Sequence[Tuple[int, "object"]], device_strings: bool = False, kept: Optional[List[str]] = None):
    """A `FilterProgram` as the arguments of `RowFilter.eval`: (`_lib.FilterLeaf` list, ops uint32, string tables uint32).
    A string leaf's table is its comparison applied to every string of its column's dictionary as it stands now.
    `device_strings=True` adds (`_lib.FilterMatch` list, texts bytes): a string leaf the match kernel can take gets a table
    range of zeros and a match entry that fills it on the device; the others keep host tables, one sentence each into `kept`."""
    leaves, parts, off = [], [], 0
    matches, texts = [], b""
    for lf in program.leaves:
        col, meta = columns[lf.column]
        out = _lib.FilterLeaf(bound=float(lf.bound), table_off=0, table_codes=0, column=int(col),
                              num_op=_lib.FILTER_NUM_OPS[lf.num_op], str_mode=_lib.FILTER_STR_MODES.get(lf.str_op, 2),
                              bool_bits=int(lf.bools[0]) | (int(lf.bools[1]) << 1), other_bit=int(lf.other))
        if out.str_mode == 2:
            why = None
            if device_strings:
                why = match_on_device(lf.str_op, lf.text) if meta.encodable else \
                    f"metadata[{meta.key!r}] holds a string without a UTF-8 form"
                if why is not None and kept is not None:
                    kept.append(f"{lf.str_op} {lf.text[:40]!r} on metadata[{meta.key!r}]: {why}")
            if device_strings and why is None:
                raw = lf.text.encode("utf-8")
                matches.append(_lib.FilterMatch(text_off=len(texts), text_len=len(raw), leaf=len(leaves), op=_lib.FILTER_MATCH_OPS[lf.str_op]))
                texts += raw
                table = np.zeros((len(meta.strings) + 31) // 32, np.uint32)
            else:
                table = meta.string_table(lf.str_op, lf.text)
            out.table_off, out.table_codes = off, len(meta.strings)
            parts.append(table)
            off += len(table)
        leaves.append(out)
    ops = np.asarray([_lib.FILTER_OPS[op] | (i << 8) for op, i in program.ops], dtype=np.uint32)
    tables = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return (leaves, ops, tables, matches, texts) if device_strings else (leaves, ops, tables)


def dicts_to_csr(rows: Sequence[Dict[int, float]]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`{term: weight}` rows -> CSR (int64 indptr, int32 terms ascending within a row, float32 weights).  One pass of
    C-level iteration plus a lexsort: a 1 M-document ingest or a 1 000-query batch does not loop in Python per entry."""
    from itertools import chain

    n = len(rows)
    lens = np.fromiter((len(r) for r in rows), np.int64, n)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    total = int(indptr[-1])
    terms = np.fromiter(chain.from_iterable(rows), np.int64, total)                       # iterating a dict yields its keys
    weights = np.fromiter(chain.from_iterable(r.values() for r in rows), np.float64, total)
    i32 = np.iinfo(np.int32)
    if total and (terms.min() < i32.min or terms.max() > i32.max):
        # checked on the int64 keys: a term that does not fit int32 would wrap in the cast below and pass the later range checks
        # (terms that fit but lie outside the vocabulary are rejected there, by the caller or the C layer)
        bad = int(np.searchsorted(indptr, np.nonzero((terms < i32.min) | (terms > i32.max))[0][0], side="right") - 1)
        raise ValueError(f"sparse vector {bad} has a term outside the int32 range")
    order = np.lexsort((terms, np.repeat(np.arange(n, dtype=np.int64), lens)))
    return indptr, terms[order].astype(np.int32), weights[order].astype(np.float32)


def _csr_args(indptr, indices, values):
    """A CSR triple as the library takes it -- (indptr ptr, indices ptr, values ptr) -- and its row count."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float32)
    return (_lp(indptr), _ip(indices), _fp(values)), len(indptr) - 1


class SparseShard(_Handle):
    """One GPU's slice of the SPLADE corpus (immutable SELL-64 image built from CSR)."""

    _destroy = "vrag_sparse_index_destroy"

    def __init__(self, vocab: int, indptr: np.ndarray, indices: np.ndarray, values: np.ndarray, device: int = 0):
        _lib.require_gpu()
        self.vocab = vocab
        csr, self.n_docs = _csr_args(indptr, indices, values)
        self._open("vrag_sparse_index_create", vocab, self.n_docs, *csr, device)

    def stats(self) -> Dict[str, int]:
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check("vrag_sparse_index_stats", self._lib.vrag_sparse_index_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"n_docs": a.value, "nnz": b.value, "padded_nnz": c.value}

    def _search(self, csr, k: int, allow, stream):
        q, nq = _csr_args(*csr)
        return _search_call(self._lib, "vrag_sparse_index_search", (self._h, *q), nq, k, allow, stream)

    def search_csr(self, q_indptr, q_indices, q_values, k: int, stream=None) -> Tuple[np.ndarray, np.ndarray]:
        return self._search((q_indptr, q_indices, q_values), k, None, stream)

    def search(self, queries: Sequence[Dict[int, float]], k: int, stream=None):
        return self.search_csr(*dicts_to_csr(queries), k, stream)

    def search_filtered(self, queries: Sequence[Dict[int, float]], k: int, allow_words: np.ndarray, n_allow: int, stream=None):
        """`search` over the documents `d < min(n_allow, n_docs)` whose bit is set in `allow_words` (see
        `DenseShard.search_filtered`; `vrag_sparse_index_search_filtered`)."""
        return self._search(dicts_to_csr(queries), k, (allow_words, n_allow), stream)

    def search_device(self, queries: Sequence[Dict[int, float]], k: int, out_scores: int, out_ids: int,
                      row_map: Optional[int] = None, n_map: int = 0, id_base: int = 0, stream=None) -> None:
        """`search` with the lists left in HBM (see DenseShard.search_device)."""
        q, nq = _csr_args(*dicts_to_csr(queries))
        _lib.check("vrag_sparse_index_search_device", self._lib.vrag_sparse_index_search_device(
            self._h, *q, nq, k, C.c_void_p(row_map) if row_map else None, n_map, id_base, C.c_void_p(out_scores),
            C.c_void_p(out_ids), stream))

    def run_resident(self, nq: int, k: int, stream=None) -> None:
        _lib.check("vrag_sparse_index_run_resident", self._lib.vrag_sparse_index_run_resident(self._h, nq, k, stream))


def _utf8_batch(texts: Sequence[str]) -> Tuple[bytes, np.ndarray]:
    """Texts back to back as UTF-8 and their `[n + 1]` byte offsets."""
    raw = [t.encode("utf-8", "surrogatepass") for t in texts]
    off = np.zeros(len(raw) + 1, np.int64)
    if raw:
        np.cumsum([len(r) for r in raw], out=off[1:])
    return b"".join(raw), off


def _bitmap(mask: np.ndarray) -> np.ndarray:
    """bool per row -> uint32 words, bit r % 32 of word r // 32 (include/vrag_amd.h, vrag_text_index_set_live)."""
    bits = np.packbits(np.asarray(mask, dtype=bool), bitorder="little")
    words = np.zeros((len(bits) + 3) // 4 * 4, np.uint8)
    words[: len(bits)] = bits
    return words.view(np.uint32)


class TextIndex(_Handle):
    """BM25 index of raw texts in HBM (`vrag_text_index_*`, csrc/fulltext.hip): the device tokenises, builds the postings,
    keeps the live-row statistics and scores; the host computes idf in float64 (include/vrag_amd.h states the arithmetic)."""

    _destroy = "vrag_text_index_destroy"

    def __init__(self, k1: float = 1.2, b: float = 0.75, device: int = 0):
        # a search is two library calls (query analysis: df and N; scoring: K_d): one hold of this lock keeps an `add` or a
        # `set_live` from another thread out from between them, so both read one snapshot of the statistics
        self._mu = threading.Lock()
        self.k1, self.b = float(k1), float(b)
        self._open("vrag_text_index_create", self.k1, self.b, device)

    def add(self, texts: Sequence[str], fold: bool) -> None:
        blob, off = _utf8_batch(texts)
        with self._mu:
            _lib.check("vrag_text_index_add", self._lib.vrag_text_index_add(self._h, blob, _lp(off), len(texts), int(bool(fold))))

    def set_live(self, alive: np.ndarray) -> None:
        words = _bitmap(alive)
        with self._mu:
            _lib.check("vrag_text_index_set_live", self._lib.vrag_text_index_set_live(self._h, words.ctypes.data, len(alive)))

    def stats(self) -> Dict[str, int]:
        v = [C.c_int64() for _ in range(5)]
        _lib.check("vrag_text_index_stats", self._lib.vrag_text_index_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("rows", "live", "sum_dl", "segments", "postings"), (x.value for x in v)))

    def set_corpus_stats(self, n_live_total: int, sum_dl_total: int) -> None:
        """This index is one shard of a row-sharded corpus: `K_d` and the `N` of `query_terms` come from the corpus-wide
        totals (the sums of every shard's `stats()["live"]` / `["sum_dl"]`) until they are set again; (0, 0) = its own."""
        with self._mu:
            _lib.check("vrag_text_index_set_corpus_stats", self._lib.vrag_text_index_set_corpus_stats(
                self._h, int(n_live_total), int(sum_dl_total)))

    def query_terms(self, queries: Sequence[str]):
        """(indptr [Q+1], keys uint64, counts int32, df int64, N): the distinct terms of every query, ascending keys -- every
        term of the query texts, with df = 0 for those the index does not hold."""
        blob, off = _utf8_batch(queries)
        cap = max(1, len(blob))
        indptr = np.zeros(len(queries) + 1, np.int64)
        keys, counts, df = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.int64)
        n_live = C.c_int64()
        _lib.check("vrag_text_index_query_terms", self._lib.vrag_text_index_query_terms(
            self._h, blob, _lp(off), len(queries), cap, _lp(indptr), keys.ctypes.data, _ip(counts), _lp(df), C.byref(n_live)))
        m = int(indptr[-1])
        return indptr, keys[:m], counts[:m], df[:m], n_live.value

    @staticmethod
    def weights(counts: np.ndarray, df: np.ndarray, n_live: int) -> np.ndarray:
        """w_t = fp32(count * idf), idf = ln(1 + (N - df + 0.5) / (df + 0.5)) in float64."""
        df64 = df.astype(np.float64)
        idf = np.log(1.0 + (float(n_live) - df64 + 0.5) / (df64 + 0.5))
        return (counts.astype(np.float64) * idf).astype(np.float32)

    def search(self, queries: Sequence[str], k: int, allow: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """`[Q, k]` scores and rows (-1 = no hit) of a batch of query texts: one device pass for the batch.  `allow`: bool per
        row; rows beyond its length (added after it was built) are not returned."""
        if len(queries) == 0:
            return _topk_out(0, k, fill=True)[:2]
        return self._search(queries, k, allow, None, None)

    def search_sharded(self, queries: Sequence[str], k: int, allow: Optional[np.ndarray], n_live_total: int, sum_df, device_out=None):
        """A shard's part of a search over a row-sharded corpus.  The term list depends on the query texts alone, so the df
        vectors of all shards line up: `sum_df(df) -> corpus-wide df` (one collective per batch) sits between the query
        analysis and the scoring, and the weights come from the summed `N` and df in float64 exactly as `weights` states.
        Returns host `[Q, k]` (scores, LOCAL rows); with `device_out = (scores ptr, ids ptr, row_map ptr or None, n_map,
        stream)` (k <= 64) the lists are left in HBM with global rows instead (`vrag_text_index_search_device`) and None is
        returned."""
        return self._search(queries, k, allow, (sum_df, n_live_total), device_out)

    def _search(self, queries, k: int, allow, corpus, device_out):
        """Query analysis, weights (`corpus = (sum_df, n_live_total)`: from the corpus-wide df and N) and scoring under one
        hold of the lock; `head` = the arguments the host and the device form of the scoring call share."""
        Q = len(queries)
        words = _bitmap(allow) if allow is not None else None
        with self._mu:
            indptr, keys, counts, df, n_live = self.query_terms(queries)
            if corpus is not None:
                df, n_live = np.asarray(corpus[0](df), dtype=np.int64), corpus[1]
            w = np.ascontiguousarray(self.weights(counts, df, n_live))
            keys = np.ascontiguousarray(keys)
            head = (self._h, _lp(indptr), keys.ctypes.data, _fp(w), Q, k, words.ctypes.data if words is not None else None,
                    len(allow) if allow is not None else 0)
            if device_out is not None:
                out_s, out_i, row_map, n_map, stream = device_out
                _lib.check("vrag_text_index_search_device", self._lib.vrag_text_index_search_device(
                    *head, C.c_void_p(row_map) if row_map else None, n_map, 0, C.c_void_p(out_s), C.c_void_p(out_i), stream))
                return None
            scores, ids, sp, ip = _topk_out(Q, k, fill=True)
            _lib.check("vrag_text_index_search", self._lib.vrag_text_index_search(*head, sp, ip))
            return scores, ids


def tokenize_keys(texts: Sequence[str], device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The analyzer alone (`vrag_text_tokenize`): token counts per text and every token's term key, in text order."""
    lib = _lib.load()
    blob, off = _utf8_batch(texts)
    cap = max(1, len(blob))
    counts = np.zeros(max(1, len(texts)), np.int32)
    keys = np.zeros(cap, np.uint64)
    n = C.c_int64()
    _lib.check("vrag_text_tokenize", lib.vrag_text_tokenize(blob, _lp(off), len(texts), device, cap, _ip(counts), keys.ctypes.data, C.byref(n)))
    return counts[: len(texts)], keys[: n.value]
