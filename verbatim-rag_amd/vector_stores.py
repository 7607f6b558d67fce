"""GPU vector store behind the reference's `VectorStore` interface.

Kept from the reference (same names, argument meaning, error behaviour):
  * `SearchResult` / `VectorStore`            verbatim_rag/vector_stores/base.py:10-74
  * `BaseMilvusStore.add_vectors/.query` semantics (dense = COSINE, sparse = IP, hybrid = top-2k per
    method then weighted RRF, dense fallback on failure)      vector_stores/milvus_base.py:90-127,189-313,366-459
  * weighted RRF + hit conversion              vector_stores/hybrid_search.py:15-175 (float64 Python semantics)
The Milvus client is replaced by exact brute-force top-k on the GPU (include/vrag_amd.h,
vrag_dense_index_* / vrag_sparse_index_*).  Multi-GPU: rows shard across ranks and per-shard top-k lists are
all-gathered and merged in distributed.py (ShardedTopK).
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import logging
import re
import threading
from abc import ABC, abstractmethod
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
# The layers under the store, re-exported here under the names callers and tests have always used.  The store resolves
# DenseShard / SparseShard / IvfOverlay / TextIndex through THIS module's globals at call time (tests replace them here);
# RowFilter / GroupColumn likewise, through the two factories it hands its `StoreMetadata`.
from .shards import (_FP, _IP, _LP, DenseShard, GroupColumn, IvfOverlay, PqShard, RowFilter, SparseShard, Sq8Shard, TextIndex, _allow_words, _bitmap,  # noqa: F401
                     _utf8_batch, dicts_to_csr, tokenize_keys)
from .store_filter import _FILTER_TOKEN, _typed, compile_filter, parse_filter  # noqa: F401
from .store_io import (_NO_METADATA, _get_strings, _put_strings, _replace_into, _write_text, get_pq_codebooks,  # noqa: F401
                       put_pq_codebooks, read_saved)
from .store_metadata import StoreMetadata

logger = logging.getLogger(__name__)


@dataclass
class SearchResult:
    """base.py:10-39."""

    id: str
    score: float
    metadata: Dict[str, Any]
    text: str
    enhanced_text: str = ""

    def __gt__(self, other):
        return self.score > other.score

    def __lt__(self, other):
        return self.score < other.score

    def __eq__(self, other):
        return self.score == other.score

    def __hash__(self):
        return hash((self.id, self.score, self.text, self.enhanced_text))


class VectorStore(ABC):
    """base.py:42-74."""

    @abstractmethod
    def add_vectors(self, ids, dense_vectors, sparse_vectors, texts, enhanced_texts, metadatas):
        pass

    @abstractmethod
    def query(self, dense_query=None, sparse_query=None, text_query=None, top_k: int = 5,
              search_type: str = "hybrid", filter: Optional[str] = None) -> List[SearchResult]:
        pass

    @abstractmethod
    def delete(self, ids: List[str]):
        pass


# ---------------------------------------------------------------------------- rank fusion
# The reference fuses per-method hit lists with weighted reciprocal-rank fusion (vector_stores/hybrid_search.py:15-175).
# Here ONE array routine (`rrf_merge_rows`) does the arithmetic for a whole batch of queries on row numbers; the
# per-query, dict-shaped entry points the reference's callers know are thin adapters over it.  The arithmetic contract
# (pinned by tests/golden/host_fixtures.json, generated from the imported reference): float64,
# `score(id) = sum over methods in insertion order of share(method) / (rrf_k + rank + 1)` with 0-based ranks, ids ordered
# by score descending with ties in first-seen order, reported `distance = 1 - score`.
FUSION_METHODS = ("dense", "sparse", "full_text")


def sanitize_hybrid_weights(hybrid_weights: Dict[str, float]) -> Dict[str, float]:
    """Keeps the entries that name a fusion method with a positive numeric weight, as floats (hybrid_search.py:15-45).
    Raises ValueError for an empty mapping or when nothing survives; dropped entries are logged."""
    if not hybrid_weights:
        raise ValueError("hybrid_weights must be a non-empty dict")
    kept: Dict[str, float] = {}
    for name, w in hybrid_weights.items():
        usable = name in FUSION_METHODS and isinstance(w, (int, float)) and w > 0
        if usable:
            kept[name] = float(w)
        else:
            logger.warning("hybrid_weights: dropping %r: %r (unknown method or non-positive weight)", name, w)
    if not kept:
        raise ValueError("No valid hybrid_weights after validation")
    return kept


def normalize_weights(results_by_method: Dict[str, Any], weights: Dict[str, float]) -> Dict[str, float]:
    """Share of each method that actually produced a list (hybrid_search.py:48-70): its weight over the sum of the
    present methods' weights; equal shares when that sum is zero."""
    present = list(results_by_method)
    mass = [weights.get(m, 0.0) for m in present]
    total = sum(mass)
    if total == 0:
        logger.warning("hybrid search: no weight on any of %s, fusing with equal shares", present)
        return dict.fromkeys(present, 1.0 / len(present))
    return {m: w / total for m, w in zip(present, mass)}


def rrf_merge_rows(rows_by_method: Dict[str, np.ndarray], top_k: int, weights: Dict[str, float],
                   rrf_k: int = 60) -> Tuple[np.ndarray, np.ndarray]:
    """Weighted RRF for a whole batch of queries on row numbers.  `rows_by_method[m]` is `[Q, L_m]` ranked rows, methods
    in insertion order; a negative entry is a rank without a candidate (no hit, or a hit the caller must skip: it still
    occupies its rank).  Returns `rows [Q, top_k]` (-1 padded) and `distance [Q, top_k]` (float64, `1 - score`).

    All lists are laid side by side as one `[Q, L]` candidate matrix and the (query, row) pairs are grouped by ONE stable
    sort of the flattened matrix -- O(Q L log(Q L)) time, O(Q L) memory, whatever the list length.  A group's score
    is accumulated method by method in insertion order (`np.add.at` applies repeated indices one after the other), so
    every float64 sum has the operands and the order of the reference's sequential accumulation; the final order is
    score descending with ties in first-seen order (a lexsort on the group's first position)."""
    methods = list(rows_by_method)
    if not methods:
        raise ValueError("rrf_merge_rows needs at least one method")
    share = normalize_weights(dict.fromkeys(methods), weights)
    lists = [np.asarray(rows_by_method[m], dtype=np.int64) for m in methods]
    Q = lists[0].shape[0]
    cand = np.concatenate(lists, axis=1)                                          # [Q, L]
    L = cand.shape[1]
    rows_out = np.full((Q, top_k), -1, np.int64)
    dist = np.zeros((Q, top_k), np.float64)
    flat = cand.reshape(-1)
    live = np.nonzero(flat >= 0)[0]                                               # flat positions, ascending = (query, position)
    if live.size == 0:
        return rows_out, dist
    qi = live // L
    span = int(flat.max()) + 1
    key = qi * span + flat[live]                                                  # one integer per (query, row) pair
    order = np.argsort(key, kind="stable")                                        # equal pairs stay in position order
    sk = key[order]
    head = np.concatenate([[True], sk[1:] != sk[:-1]])
    gid_sorted = np.cumsum(head) - 1
    n_groups = int(gid_sorted[-1]) + 1
    gid = np.empty(live.size, np.int64)
    gid[order] = gid_sorted
    first_pos = live[order][head]                                                 # flat position of a group's first occurrence
    score = np.zeros(n_groups, np.float64)
    pos_in_q = live - qi * L
    lo = 0
    for m, rows in zip(methods, lists):
        n = rows.shape[1]
        sel = (pos_in_q >= lo) & (pos_in_q < lo + n)
        gain = share.get(m, 0.0) * (1.0 / (rrf_k + np.arange(n, dtype=np.float64) + 1))
        np.add.at(score, gid[sel], gain[pos_in_q[sel] - lo])
        lo += n
    gq = first_pos // L
    final = np.lexsort((first_pos, -score, gq))                                   # query, then score desc, then first seen
    gq_f = gq[final]
    start = np.searchsorted(gq_f, np.arange(Q), side="left")
    rank_in_q = np.arange(n_groups) - start[gq_f]
    keep = rank_in_q < top_k
    rows_out[gq_f[keep], rank_in_q[keep]] = flat[first_pos[final][keep]]
    dist[gq_f[keep], rank_in_q[keep]] = 1.0 - score[final][keep]
    return rows_out, dist


def rrf_fuse_rows_device(rows_by_method: Dict[str, np.ndarray], top_k: int, weights: Dict[str, float],
                         rrf_k: int = 60, device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """`rrf_merge_rows` on the GPU (`vrag_rrf_fuse`, csrc/fuse.hip): same arguments, same `[Q, top_k]` rows (-1 padded) and
    float64 distances, bit for bit.  The gain of every position -- `share * (1.0 / (rrf_k + rank + 1))`, the expression
    `rrf_merge_rows` evaluates -- is computed here, so the kernel only adds float64 values in the reference's order
    (ascending position = methods in insertion order, ranks ascending) and the division and the weights never reach it.
    Lists of up to 4096 entries per query in all, row numbers below 2^32 (include/vrag_amd.h)."""
    methods = list(rows_by_method)
    if not methods:
        raise ValueError("rrf_fuse_rows_device needs at least one method")
    share = normalize_weights(dict.fromkeys(methods), weights)
    lists = [np.asarray(rows_by_method[m], dtype=np.int64) for m in methods]
    Q = lists[0].shape[0]
    cand = np.ascontiguousarray(np.concatenate(lists, axis=1))                   # [Q, L]
    L = cand.shape[1]
    rows_out = np.full((Q, top_k), -1, np.int64)
    dist = np.zeros((Q, top_k), np.float64)
    if cand.size == 0 or top_k <= 0 or not (cand >= 0).any():
        return rows_out, dist
    gains = np.ascontiguousarray(np.concatenate(
        [share.get(m, 0.0) * (1.0 / (rrf_k + np.arange(r.shape[1], dtype=np.float64) + 1)) for m, r in zip(methods, lists)]))
    k = min(top_k, L)                                                             # the call's top_k <= l_total; the rest is padding
    got_rows = np.empty((Q, k), np.int64)
    got_dist = np.empty((Q, k), np.float64)
    _lib.check("vrag_rrf_fuse", _lib.load().vrag_rrf_fuse(
        cand.ctypes.data_as(C.c_void_p), gains.ctypes.data_as(C.c_void_p), Q, L, k, got_rows.ctypes.data_as(C.c_void_p),
        got_dist.ctypes.data_as(C.c_void_p), 0, int(device), None))
    rows_out[:, :k] = got_rows
    dist[:, :k] = got_dist
    return rows_out, dist


def merge_hybrid_results(results_by_method: Dict[str, List[dict]], top_k: int, weights: Dict[str, float],
                         rrf_k: int = 60, log_label: str = "") -> List[dict]:
    """The per-query, dict-shaped form (hybrid_search.py:73-129): hits are dicts with an "id"; hits whose id is falsy
    are skipped but keep their rank.  Ids are numbered in first-seen order and the batch routine does the rest; each
    merged entry is a copy of the first hit seen for its id with `distance = 1 - score`."""
    number: Dict[Any, int] = {}
    exemplar: List[dict] = []
    coded: Dict[str, np.ndarray] = {}
    for method, hits in results_by_method.items():
        row = np.full((1, len(hits)), -1, np.int64)
        for pos, hit in enumerate(hits):
            key = hit.get("id")
            if not key:
                continue
            if key not in number:
                number[key] = len(exemplar)
                exemplar.append(hit)
            row[0, pos] = number[key]
        coded[method] = row
    if log_label:
        logger.info("hybrid merge (%s): methods=%s rrf_k=%s top_k=%s", log_label, list(coded), rrf_k, top_k)
    rows, dist = rrf_merge_rows(coded, top_k, weights, rrf_k)
    merged = []
    for code, d in zip(rows[0], dist[0]):
        if code >= 0:
            hit = dict(exemplar[int(code)])
            hit["distance"] = float(d)
            merged.append(hit)
    return merged


def _metadata_of(entity: dict) -> Dict[str, Any]:
    raw = entity.get("metadata", {}) or {}
    if not isinstance(raw, str):
        return raw
    try:                                # a JSON column read back as text
        return json.loads(raw)
    except Exception:
        return {"raw": raw}


def convert_hits_to_results(hits: List[dict], dynamic_fields: Optional[List[str]] = None) -> List[SearchResult]:
    """Search hits (`{"id", "distance", "entity": {...}}`, the shape a Milvus client returns and the shape
    `merge_hybrid_results` passes through) -> `SearchResult`s; `dynamic_fields` present on the entity are copied into
    the metadata (hybrid_search.py:132-175)."""
    results = []
    for hit in hits:
        entity = hit.get("entity", {})
        metadata = _metadata_of(entity)
        metadata.update({f: entity[f] for f in (dynamic_fields or ()) if entity.get(f) is not None})
        results.append(SearchResult(id=hit.get("id"), score=hit.get("distance", 0.0), metadata=metadata,
                                    text=entity.get("text", ""), enhanced_text=entity.get("enhanced_text", "")))
    return results


IVF_INDEX_TYPES = ("IVF_FLAT", "IVF_SQ8")   # index types with lists: an `IvfOverlay` over the resident dense shard
IVF_MIN_ROWS = 4096       # below this a store with one of them searches FLAT
IVF_NLIST_MAX = 16384     # vrag_ivf_index_create
IVF_MIN_LIST_ROWS = 39    # rows per list a training needs, as faiss' k-means asks for (min_points_per_centroid)
IVF_K_MAX = 64            # vrag_ivf_index_search
PQ_MIN_ROWS = 256 * IVF_MIN_LIST_ROWS   # below this an index_type="PQ" store keeps exact fp32 rows: 256 centroids per sub-space to train
PQ_TRAIN_ROWS_MAX = 65536   # rows of the training sample, evenly strided over the host rows (a first choice: not swept)
PQ_TRAIN_ITERS = 10         # Lloyd rounds of that training (a first choice: not swept)
PQ_M_MAX, PQ_DSUB_MAX = 128, 64   # vrag_pq_index_create


def ivf_effective_nlist(n_rows: int, nlist: int) -> int:
    """Lists an IVF_FLAT / IVF_SQ8 store of `n_rows` rows is built with: 0 (= search FLAT) below `IVF_MIN_ROWS`, else the configured
    `nlist` capped by the library's limit and by `IVF_MIN_LIST_ROWS` rows per list."""
    if n_rows < IVF_MIN_ROWS:
        return 0
    return min(int(nlist), IVF_NLIST_MAX, n_rows // IVF_MIN_LIST_ROWS)


def parse_nprobe(search_params: Optional[Dict[str, Any]], default: int) -> int:
    """`nprobe` of a query's `search_params`: `{"nprobe": n}` as the reference's callers pass it (index.py:571) or Milvus'
    `{"params": {"nprobe": n}}`; the grouping keys are `parse_grouping`'s, other keys are ignored, no `nprobe` = `default`.  ValueError unless a positive integer."""
    value = None
    if search_params:
        inner = search_params.get("params")
        if "nprobe" in search_params:
            value = search_params["nprobe"]
        elif isinstance(inner, dict) and "nprobe" in inner:
            value = inner["nprobe"]
    if value is None:
        return default
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"nprobe must be a positive integer (got {value!r})")
    return int(value)


GROUP_TOP_K_MAX = 64      # vrag_dense_index_search_grouped: groups per query
GROUP_SIZE_MAX = 16       # ... and rows per group
_GROUP_KEYS = ("group_by_field", "group_size", "strict_group_size")
_GROUP_FIELD = re.compile(r"""^metadata\[\s*(["'])(.+)\1\s*\]$""")


@dataclass(frozen=True)
class Grouping:
    """A query's grouping request: the metadata key, rows per group, and Milvus' `strict_group_size` (accepted, no effect:
    an exact search always returns every row a group has, up to `group_size`)."""
    key: str
    group_size: int = 1
    strict: bool = False


def parse_grouping(search_params: Optional[Dict[str, Any]]) -> Optional[Grouping]:
    """The grouping request of a query's `search_params`: `group_by_field` (a metadata key, bare or spelled
    `metadata["key"]`), `group_size` (default 1, at most `GROUP_SIZE_MAX`) and `strict_group_size` (a bool), at top level or
    under `"params"` like `nprobe` (top level wins).  None when no `group_by_field` is given.  ValueError for a field that is
    no non-empty string, a `group_size` that is no integer in range, a `strict_group_size` that is no bool, and for
    `group_size` / `strict_group_size` without a `group_by_field`."""
    given: Dict[str, Any] = {}
    if search_params:
        inner = search_params.get("params")
        for name in _GROUP_KEYS:
            if name in search_params:
                given[name] = search_params[name]
            elif isinstance(inner, dict) and name in inner:
                given[name] = inner[name]
    if "group_by_field" not in given:
        if given:
            raise ValueError(f"{sorted(given)[0]} needs a group_by_field")
        return None
    field = given["group_by_field"]
    if not isinstance(field, str) or not field.strip():
        raise ValueError(f"group_by_field must be a metadata key (got {field!r})")
    field = field.strip()
    spelled = _GROUP_FIELD.match(field)
    if spelled:
        field = spelled.group(2)
    elif field.startswith("metadata["):
        raise ValueError(f"group_by_field must be a metadata key or metadata[\"key\"] (got {field!r})")
    size = given.get("group_size", 1)
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 1 <= size <= GROUP_SIZE_MAX:
        raise ValueError(f"group_size must be an integer in [1, {GROUP_SIZE_MAX}] (got {size!r})")
    strict = given.get("strict_group_size", False)
    if not isinstance(strict, (bool, np.bool_)):
        raise ValueError(f"strict_group_size must be a bool (got {strict!r})")
    return Grouping(field, int(size), bool(strict))


def check_index_config(index_type: str, nlist: int, nprobe: int, sharded: bool, m: Optional[int] = None, nbits: int = 8,
                       dense_dim: Optional[int] = None) -> None:
    """The constructor's refusals for `index_type` / `nlist` / `nprobe` and, for index_type="PQ", `m` / `nbits` (pure: no
    device needed)."""
    if index_type not in ("FLAT", *IVF_INDEX_TYPES, "PQ"):
        raise ValueError(f"index_type must be 'FLAT', 'IVF_FLAT', 'IVF_SQ8' or 'PQ' (got {index_type!r})")
    for name, v in (("nlist", nlist), ("nprobe", nprobe)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} must be a positive integer (got {v!r})")
    if index_type in IVF_INDEX_TYPES and sharded:
        raise ValueError(f"index_type={index_type!r} is single-GPU: sharded stores (distributed=True or a comm) keep FLAT")
    if index_type != "PQ":
        if m is not None:
            raise ValueError(f"m is the number of sub-vectors of index_type='PQ': not with index_type={index_type!r}")
        return
    if sharded:
        raise ValueError("index_type='PQ' is single-GPU: sharded stores (distributed=True or a comm) keep FLAT")
    if isinstance(nbits, bool) or not isinstance(nbits, (int, np.integer)) or nbits != 8:
        raise ValueError(f"index_type='PQ' stores 8-bit codes: nbits must be 8 (got {nbits!r})")
    if m is None:
        raise ValueError("index_type='PQ' needs m, the number of sub-vectors (code bytes per row)")
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= PQ_M_MAX:
        raise ValueError(f"m must be an integer in [1, {PQ_M_MAX}] (got {m!r})")
    if not isinstance(dense_dim, (int, np.integer)) or dense_dim < 1 or dense_dim % m != 0:
        raise ValueError(f"m must divide dense_dim (got m={m!r}, dense_dim={dense_dim!r})")
    if dense_dim // m > PQ_DSUB_MAX:
        raise ValueError(f"a PQ sub-vector holds at most {PQ_DSUB_MAX} components: dense_dim={dense_dim!r} / m={m!r} is more")


def check_auto_compact(auto_compact: Optional[float], sharded: bool) -> None:
    """The constructor's refusals for `auto_compact` (pure: no device needed)."""
    if auto_compact is None:
        return
    if isinstance(auto_compact, bool) or not isinstance(auto_compact, (int, float, np.floating)) or not 0 < auto_compact < 1:
        raise ValueError(f"auto_compact must be None or a fraction in (0, 1) (got {auto_compact!r})")
    if sharded:
        raise ValueError("auto_compact is single-GPU: sharded stores (distributed=True or a comm) are not compacted")


DENSE_DTYPES = ("f32", "bf16", "int8")


def check_dense_dtype(dense_dtype: str, index_type: str, sharded: bool) -> None:
    """The constructor's refusals for `dense_dtype` (pure: no device needed).  "int8" (SQ8 rows, `Sq8Shard`) has no
    device-resident search form, so it is single-GPU; its lists are index_type="IVF_SQ8", which in turn needs int8 rows."""
    if dense_dtype not in DENSE_DTYPES:
        raise ValueError(f"dense_dtype must be 'f32', 'bf16' or 'int8' (got {dense_dtype!r})")
    if dense_dtype == "int8" and sharded:
        raise ValueError("dense_dtype='int8' is single-GPU: sharded stores (distributed=True or a comm) keep 'f32' or 'bf16'")
    if dense_dtype == "int8" and index_type == "IVF_FLAT":
        raise ValueError("index_type='IVF_FLAT' needs 'f32' or 'bf16' rows: dense_dtype='int8' searches FLAT or index_type='IVF_SQ8'")
    if index_type == "IVF_SQ8" and dense_dtype != "int8":
        raise ValueError(f"index_type='IVF_SQ8' lays its lists over SQ8 rows: it needs dense_dtype='int8' (got dense_dtype={dense_dtype!r})")
    if index_type == "PQ" and dense_dtype != "f32":
        raise ValueError(f"index_type='PQ' encodes fp32 rows: it needs dense_dtype='f32' (got dense_dtype={dense_dtype!r})")


def check_choice(name: str, value, a: str, b: str) -> None:
    """The constructor's refusal for an option with two choices."""
    if value not in (a, b):
        raise ValueError(f"{name} must be {a!r} or {b!r} (got {value!r})")


_JSON_PLAIN = (str, int, float, bool, type(None))


def json_serialize_safe(obj: Any) -> Any:
    """The JSON column's view of caller metadata -- what a search returns and what filters compare against
    (the reference applies the same conversion before its insert, vector_stores/utils.py:10-29): datetimes as ISO
    strings, enum members as their values, mapping keys as strings, descending through dicts and lists only."""
    from datetime import datetime
    from enum import Enum

    def view(x):
        if isinstance(x, dict):
            return {str(key): view(val) for key, val in x.items()}
        if isinstance(x, list):
            return [view(item) for item in x]
        if isinstance(x, datetime):
            return x.isoformat()
        if isinstance(x, Enum):
            return getattr(x, "value", str(x))
        return x

    return view(obj)


def _metadata_rows(metadatas: Sequence[Optional[dict]]) -> List[Dict[str, Any]]:
    """`json_serialize_safe(dict(md))` for a batch of rows (milvus_base.py:108-109); flat dicts of plain JSON scalars
    under string keys -- what ingestion produces -- are copied without the recursive walk."""
    plain = _JSON_PLAIN
    out = []
    for md in metadatas:
        if not md:
            out.append(_NO_METADATA)         # stored metadata is never modified in place (results hand out copies)
        elif all(type(k) is str and type(v) in plain for k, v in md.items()):
            out.append(dict(md))
        else:
            out.append(json_serialize_safe(dict(md)))
    return out


class _Column:
    """Append-only numpy column with amortised growth: `data` is the `[n]` or `[n, width]` view of the filled part.
    A view handed out earlier stays valid (it keeps its buffer) and covers the rows that existed then."""

    def __init__(self, dtype, width: Optional[int] = None, first: Optional[Sequence] = None):
        self._width = width
        self._buf = np.empty((0,) if width is None else (0, width), dtype)
        self._n = 0
        if first is not None:
            self.extend(np.asarray(first, dtype))

    def __len__(self) -> int:
        return self._n

    @property
    def data(self) -> np.ndarray:
        return self._buf[: self._n]

    def extend(self, rows: np.ndarray, adopt: bool = False) -> None:
        """`adopt=True`: `rows` is a fresh array nobody else holds -- an empty column takes it as its buffer (no copy)."""
        m = len(rows)
        if adopt and self._n == 0 and rows.dtype == self._buf.dtype and rows.flags.c_contiguous and rows.flags.owndata:
            self._buf, self._n = rows, m
            return
        if self._n + m > len(self._buf):
            cap = max(self._n + m, int(len(self._buf) * 1.5) + 16)
            grown = np.empty((cap,) + self._buf.shape[1:], self._buf.dtype)
            grown[: self._n] = self._buf[: self._n]
            self._buf = grown
        self._buf[self._n: self._n + m] = rows
        self._n += m


def _take(col: list, at: np.ndarray) -> list:
    """`[col[i] for i in at]` for 10^7 rows: one object-array gather instead of a Python loop."""
    box = np.empty(len(col), dtype=object)
    box[:] = col
    return box[at].tolist()


def csr_take_rows(indptr: np.ndarray, indices: np.ndarray, values: np.ndarray, rows: np.ndarray):
    """CSR of the selected rows (in the given order), without a Python loop per row."""
    rows = np.asarray(rows, dtype=np.int64)
    lens = indptr[rows + 1] - indptr[rows]
    out_ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=out_ptr[1:])
    take = np.repeat(indptr[rows] - out_ptr[:-1], lens) + np.arange(int(out_ptr[-1]), dtype=np.int64)
    return out_ptr, indices[take], values[take]


def _as_csr(sparse_vectors, n_expected: int, vocab: int):
    """Sparse rows in any accepted form -> canonical CSR (int64 indptr, int32 terms strictly ascending within a row,
    float32 weights).  Accepted: the reference's `List[Dict[int, float]]` (embedding_providers.py:33-49), and for bulk
    ingest a `(indptr, indices, values)` triple or a scipy CSR matrix (rows with unsorted terms are sorted; a term
    repeated inside a row is rejected -- a dict cannot hold one)."""
    if hasattr(sparse_vectors, "indptr") and hasattr(sparse_vectors, "indices") and hasattr(sparse_vectors, "data"):
        sparse_vectors = (sparse_vectors.indptr, sparse_vectors.indices, sparse_vectors.data)
    if isinstance(sparse_vectors, tuple) and len(sparse_vectors) == 3 and isinstance(sparse_vectors[0], np.ndarray):
        indptr = np.ascontiguousarray(sparse_vectors[0], dtype=np.int64)
        indices = np.asarray(sparse_vectors[1])
        values = np.ascontiguousarray(sparse_vectors[2], dtype=np.float32)
        if len(indptr) != n_expected + 1:
            raise ValueError(f"add_vectors: {len(indptr) - 1} sparse_vectors for {n_expected} ids")
        if indptr[0] != 0 or (np.diff(indptr) < 0).any() or indptr[-1] != len(indices) or len(indices) != len(values):
            raise ValueError("add_vectors: malformed CSR sparse_vectors")
        if len(indices) and (indices.min() < 0 or indices.max() >= vocab):
            bad = int(np.searchsorted(indptr, np.nonzero((indices < 0) | (indices >= vocab))[0][0], side="right") - 1)
            raise ValueError(f"add_vectors: sparse vector {bad} has a term outside [0, {vocab})")
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        if len(indices) > 1:
            # terms must ascend strictly inside a row: look only at the places where they do not (row starts, mostly)
            drops = np.nonzero(indices[1:] <= indices[:-1])[0] + 1
            if len(drops) and not np.isin(drops, indptr).all():
                row_of = np.repeat(np.arange(n_expected, dtype=np.int64), np.diff(indptr))
                order = np.lexsort((indices, row_of))
                indices, values = indices[order], values[order]
                drops = np.nonzero(indices[1:] <= indices[:-1])[0] + 1
                if not np.isin(drops, indptr).all():
                    raise ValueError("add_vectors: a sparse vector repeats a term")
        return indptr, indices, values
    if len(sparse_vectors) != n_expected:
        raise ValueError(f"add_vectors: {len(sparse_vectors)} sparse_vectors for {n_expected} ids")
    indptr, indices, values = dicts_to_csr(sparse_vectors)
    if len(indices) and (indices.min() < 0 or indices.max() >= vocab):
        bad = int(np.searchsorted(indptr, np.nonzero((indices < 0) | (indices >= vocab))[0][0], side="right") - 1)
        raise ValueError(f"add_vectors: sparse vector {bad} has a term outside [0, {vocab})")
    return indptr, indices, values


def _merge_parts(scores: np.ndarray, rows: np.ndarray, k: int, device: int) -> Tuple[np.ndarray, np.ndarray]:
    """Lists of the segments of one shard `[P, Q, k]` (global rows) -> `[Q, k]`, on the GPU (`vrag_topk_merge`)."""
    from .distributed import merge_topk_device

    return merge_topk_device(scores, rows, k, device)



def _one_epoch(method):
    """A `GpuVectorStore` search method answered from ONE epoch of the store (class docstring, "Compaction"): answered again from
    scratch when a compaction ran meanwhile.  The epoch is read under the lock, which a running compaction holds from its first
    change to its last; an exception counts as a moved epoch when the epoch has moved (a stale row number can point past the
    shortened columns)."""

    @functools.wraps(method)
    def answered(self, *args, **kwargs):
        while True:
            with self._mu:
                epoch = self._epoch
            try:
                out = method(self, *args, **kwargs)
            except Exception:
                if self._epoch == epoch:
                    raise
                continue
            if self._epoch == epoch:
                return out

    return answered


# ---------------------------------------------------------------------------- the store
class GpuVectorStore(VectorStore):
    """Exact GPU search store with BaseMilvusStore's behaviour (milvus_base.py:90-127,189-459).

    dense = COSINE (rows and queries are L2-normalised here, so IP on the device equals cosine),
    sparse = IP over shared terms.  Rows live on the host until the first query after an insert
    ("flush"), then in HBM; a flush appends the new dense rows to the resident shard and builds a SELL-64 image of the
    new sparse rows only (a tail segment beside the main image; the two are folded into one image when the tail
    outgrows a quarter of it).  Dense rows are stored fp32 like the reference's FLOAT_VECTOR field
    (milvus_local.py:109-118): 4 * dim bytes per row in HBM (times `dense_headroom` of append room) and as much on the
    host; `dense_dtype="bf16"` halves the HBM bytes a query streams at the price of rounding the stored rows, which
    also gives up bit-exact ranking between rows whose fp32 scores nearly tie; `dense_dtype="int8"` stores SQ8 rows
    (`Sq8Shard`: int8 codes and one fp32 scale per row, dim + 4 bytes, half of bf16's stream) and quantises the queries by
    the same rule -- scores are the integer-exact ones of include/vrag_amd.h "SQ8 dense rows", approximate only in what a
    code says about its component; single-GPU, FLAT or `index_type="IVF_SQ8"`, the host keeps its fp32 rows.
    `filter` supports the comparison subset of Milvus expressions in `parse_filter`
    (the reference itself only builds `metadata["document_id"] == "..."`, index.py:735-739); anything else is
    rejected loudly.  Filters and deletes act before the search like Milvus' (a selective filter still returns its
    best rows): `_topk_rows` re-runs short queries on a cached shard of just the passing rows.
    Every method of a search returns up to `K_LIMIT` = 1024 rows (hybrid search asks for 2 * top_k, so top_k <= 512
    there); asking for more raises ValueError -- never a silently shorter list.

    Host layout (columnar, sized for 10^7 rows): ids in one list with a lazily built id -> row table for deletes; unit
    dense rows in one growing `[n, dim]` fp32 array; sparse rows as one growing CSR; liveness as a bool column.
    `add_vectors` also takes an `[n, dim]` ndarray and a CSR triple / scipy CSR matrix for bulk ingest.

    Multi-GPU: `distributed=True` (one process per GPU, torch.distributed initialised, every rank making
    the SAME calls with the SAME arguments) row-shards the store -- each insert batch is cut contiguously over the
    ranks; a rank keeps the vectors, texts and metadata of ITS rows only (`payload="replicated"` keeps texts and
    metadata on every rank instead), ids stay replicated.  A search runs on each rank's shard, ONE all-gather carries
    the per-shard `[Q, k]` lists and every rank merges them on its GPU (`distributed.ShardComm`; under RCCL the lists
    never leave HBM between the local search and the merge); the texts / metadata of the merged hits then meet in one
    object gather.  `query` / `query_batch` return the same results on every rank and the same results as a
    single-GPU store.  Full text on a sharded store: each rank indexes the texts of its rows; `(N, sum dl)` are summed over
    the ranks once after every insert / delete / load and the `df` vector of a query batch once per batch
    (`ShardComm.sum_int64`, exact integers), so every rank scores its rows with the corpus-wide statistics -- the bits of
    the single-GPU store -- and the lists merge like the other methods'.

    Compaction: `delete` only clears a row's liveness bit; `compact()` drops the dead rows from every host column and every
    device structure and renumbers the survivors `0 .. live - 1` in their old order -- the state `load(save())` would produce,
    except that the resident dense rows (fp32 / bf16 rows, the prefilter image, SQ8 codes and scales) are compacted where they
    lie in HBM (`DenseShard.compact`: no re-upload, no second copy) and an IVF overlay keeps its centroids
    (`IvfOverlay.remap`).  The sparse images and the full-text index are rebuilt from the compacted host copies by the next
    flush, as a fold rebuilds them.  Never implicit unless `auto_compact` is set.  Single-GPU.
    Searches run outside the lock and decode row numbers after the device returns, and a compaction changes what a row number
    means, so the store keeps an EPOCH: `compact()` advances it under the lock before it touches anything; `query` /
    `query_batch` read it under the lock when they start and again when they have their answer, and answer again from scratch
    when it has moved (an exception met on the way counts as a moved epoch when it has).  An answer is therefore entirely
    from before a compaction or entirely from after it.  The device handles serialise a search's kernels against the move itself.
    """

    enable_full_text = False  # per store: the constructor's `enable_full_text`

    SUBSET_CACHE = 4
    K_LIMIT = 1024          # vrag_*_index_search: lists of up to 64 per device pass, longer ones as exact pages of 64
    DEVICE_K = 64           # longest list the device-resident exchange carries (one device pass)
    SPARSE_TAIL_MIN = 65536  # rows a sparse tail segment may always hold before it is folded into the main image
    TEXT_TAIL_MIN = 65536    # the same for the full-text index's tail segment
    # rrf_route="device": smallest hybrid batch that is fused on the GPU; below it the call's launch and copies cost more than numpy
    # (2 x 20 lists on an MI355X host: 16 queries 0.044 ms host / 0.070 ms device, 64 queries 0.104 / 0.076 -- profiles/rrf_fuse_probe.txt).
    # Both sides give the same bits, so it changes no output.
    RRF_DEVICE_MIN_QUERIES = 64

    def _use_prefilter(self) -> bool:
        if self.dense_dtype != "f32" or self.dense_prefilter is False:
            return False
        if self.dense_prefilter is True:
            return True
        return self.dense_dim is not None and self.dense_dim % 64 == 0 and self.dense_dim <= 768

    def _new_dense_shard(self, capacity: int):
        """An empty dense shard of this store's `dense_dtype` with room for `capacity` rows."""
        if self.dense_dtype == "int8":
            return Sq8Shard(self.dense_dim, capacity, self.device)
        if self._pq_codebooks is not None:      # a trained PQ store: every shard it builds carries the frozen codebooks
            shard = PqShard(self.dense_dim, self.m, capacity, self.device)
            shard.set_codebooks(self._pq_codebooks)
            return shard
        return DenseShard(self.dense_dim, capacity, self.dense_dtype, self.device, prefilter=self._use_prefilter())

    def __init__(self, dense_dim: Optional[int] = 384, sparse_vocab: Optional[int] = 30522, enable_dense: bool = True,
                 enable_sparse: bool = True, dense_dtype: str = "f32", device: int = 0, distributed: bool = False,
                 group=None, comm=None, payload: str = "sharded", dense_headroom: float = 1.5,
                 dense_prefilter="auto", enable_full_text: bool = False, bm25_k1: float = 1.2, bm25_b: float = 0.75,
                 filter_route: str = "subset", rrf_route: str = "host", index_type: str = "FLAT", nlist: int = 8192,
                 nprobe: int = 16, filter_eval: str = "host", filter_strings: str = "host",
                 auto_compact: Optional[float] = None, m: Optional[int] = None, nbits: int = 8):
        """`enable_full_text`: BM25 keyword search over the raw texts (milvus_cloud.py: bm25_k1 = 1.2, bm25_b = 0.75),
        `search_type="full_text"` and the third leg of a weighted hybrid search; the texts are tokenised, indexed and
        scored on the device (`TextIndex`).  Off by default.  On a sharded store (`distributed=True` or a `comm`) the
        corpus-wide BM25 statistics are summed over the ranks, which needs an initialised `torch.distributed` and a `comm`
        with `sum_int64`: ValueError otherwise.
        `dense_dtype`: "f32" (default), "bf16" or "int8" (see the class docstring); "int8" with `distributed=True`, a `comm`
        or `index_type="IVF_FLAT"` raises ValueError (its lists are `index_type="IVF_SQ8"`).  Kept in a saved store's manifest.
        `dense_prefilter` (fp32 rows only): keep a bf16 image of the rows beside them so that every search streams
        half (small batches) or a fraction (large ones) of the bytes of the full fp32 scan and returns the same bits (`DenseShard`).  It costs
        +50 % of the dense rows' HBM.  "auto" (default) = on where the image route exists (dim % 64 == 0 and <= 768,
        csrc/topk.hip `prefilter_route_ok`), True / False force it; the choice is kept in a saved store's manifest.
        `filter_route`: how the dense and the sparse leg answer a query whose filter (or a delete) leaves them short --
        "subset" (default) builds and caches a second shard of just the passing rows from the host copies; "bitmap" runs
        the filtered search of the RESIDENT shard over a row bitmap (`DenseShard.search_filtered`; no second shard is ever
        built, and a delete costs the next query nothing but the bitmap).  Same results either way.  A store whose exchange
        runs on the GPU (`comm.on_gpu`) keeps "subset".  A run-time choice: not written by `save`, a keyword of `load`.
        `rrf_route`: where `query_batch` fuses the methods' lists of a hybrid batch -- "host" (default) in numpy
        (`rrf_merge_rows`), "device" on the GPU (`rrf_fuse_rows_device`; batches of at least `RRF_DEVICE_MIN_QUERIES`
        queries, smaller ones are cheaper in numpy).  Same bits either way; on a sharded store every
        rank fuses the same merged lists itself (no collective).  The per-query paths (`query`, a store with a falsy id)
        always fuse on the host.  A run-time choice like `filter_route`: not written by `save`, a keyword of `load`.
        `filter_eval`: where the row mask of a filter that is no single `==` / `in` comparison (a range, `!=`, `and` / `or` /
        `not`) is computed -- "host" (default) by one Python predicate call per stored row, "device" by the row-filter kernel
        (`RowFilter`, csrc/rowfilter.hip) over typed columns of the keys the filter names: a column is built by one Python pass on
        the first filter that names its key, extended by the rows of every later insert, and costs 9 bytes of HBM per row.  The
        same mask bit for bit.  A filter beyond the device program's limits (16 keys, 64 comparisons, 256 operations, nesting
        32 deep) or naming a key that holds a NaN is answered on the host (logged once per filter string).  A run-time choice like
        `filter_route`: not written by `save`, a keyword of `load`.  A `json_contains` / `_any` / `_all` filter reads the key's
        lists instead, kept in HBM as CSR (8 bytes per row + 9 per element, csrc/listfilter.hip): uploaded by the first list filter
        on the key, extended after every insert, dropped by `compact()` and uploaded again by the next list filter; a NaN
        inside a list of the key sends list filters on it to the host.
        `filter_strings` (only with `filter_eval="device"`): who applies a filter's string comparisons and `LIKE` patterns to the
        distinct strings of a key -- "host" (default) Python, once per distinct string for every new (operator, text); "device"
        the match kernel (csrc/strmatch.hip) over the key's string dictionary kept in HBM (its UTF-8 bytes plus 8 bytes per
        distinct string; only new strings travel after an insert).  The same mask bit for bit.  A comparison whose text is
        beyond the kernel's limits (256 bytes, 16 segments between a pattern's `%`) or whose key holds a string without a UTF-8
        form keeps its host table while the rest of the filter runs on the device (logged once per filter string).  A run-time
        choice like `filter_eval`.
        `index_type`: "FLAT" (default) = every dense query streams the whole shard, exact.  "IVF_FLAT" (the reference's Milvus
        stores, milvus_base.py:40-50) = the dense leg looks only at the rows of the `nprobe` lists nearest to the query out of
        `nlist` k-means lists laid over the resident shard (`IvfOverlay`; `ivf_effective_nlist` caps `nlist` for small stores
        and keeps stores under `IVF_MIN_ROWS` rows FLAT) -- approximate in WHICH rows it finds, exact in their scores and
        order.  "IVF_SQ8" (Milvus' name) = the same lists over the SQ8 rows of `dense_dtype="int8"`, which it requires (ValueError
        with any other `dense_dtype`): the rows of the probed lists are scored by the SQ8 rule, so what it reports about a row is
        what the FLAT int8 store reports, bit for bit; everything said of IVF_FLAT here holds for it.
        `search_params={"nprobe": n}` (or Milvus' `{"params": {"nprobe": n}}`) of `query` / `query_batch` overrides
        `nprobe` per call; n >= nlist returns the FLAT results.  Lists of more than 64 rows per method, filtered queries left
        short and sharded stores search FLAT.  Kept in a saved store's manifest (FLAT stores write nothing new).
        "PQ" with `m` (and `nbits=8`, the one width) = product-quantised rows (`PqShard`, include/vrag_amd.h "PQ dense rows"): `m`
        code bytes per row in HBM instead of 4 `dense_dim`, every query scored through a look-up table -- approximate in what a
        code says about its sub-vector, exact and bit-defined in everything else.  `m` must divide `dense_dim` (at most 64
        components per sub-vector, `m` <= 128); it needs `dense_dtype="f32"` and a single GPU (ValueError otherwise).  Below
        `PQ_MIN_ROWS` rows the store keeps the exact fp32 `DenseShard`; the flush that reaches it trains the codebooks on at most
        `PQ_TRAIN_ROWS_MAX` evenly strided host rows (`PQ_TRAIN_ITERS` Lloyd rounds, deterministic) and swaps a `PqShard` in.
        The codebooks are frozen from then on: later inserts, shards rebuilt for capacity and filter-subset shards use them, so
        both `filter_route`s return the same bits; `save` writes them and `load` never retrains.  `pq_stats()` tells which state
        the store is in.  Grouping searches are refused.
        `auto_compact`: None (default) = `compact()` runs only when it is called.  A fraction in (0, 1): `delete` calls it once
        the dead rows exceed that fraction of the stored rows.  Single-GPU like `compact()`; a run-time choice, a keyword of `load`."""
        check_auto_compact(auto_compact, distributed or comm is not None)
        check_index_config(index_type, nlist, nprobe, distributed or comm is not None, m, nbits, dense_dim)
        check_dense_dtype(dense_dtype, index_type, distributed or comm is not None)
        self._lib = _lib.load()
        _lib.require_gpu()
        check_choice("payload", payload, "sharded", "replicated")
        check_choice("filter_route", filter_route, "subset", "bitmap")
        check_choice("rrf_route", rrf_route, "host", "device")
        check_choice("filter_eval", filter_eval, "host", "device")
        check_choice("filter_strings", filter_strings, "host", "device")
        if not enable_dense and not enable_sparse and not enable_full_text:      # milvus_base.py:54-56
            raise ValueError("At least one of enable_dense, enable_sparse, or enable_full_text must be True")
        if enable_full_text and comm is None and distributed:
            import torch.distributed as dist

            if not (dist.is_available() and dist.is_initialized()):
                raise ValueError("enable_full_text on a sharded store needs an initialised torch.distributed process group "
                                 "(global df / N / avgdl are summed over the ranks)")
        if enable_full_text and comm is not None and (comm.world > 1 or getattr(comm, "on_gpu", False)) \
                and not callable(getattr(comm, "sum_int64", None)):
            raise ValueError("enable_full_text on a sharded store needs a comm with sum_int64 (global df / N / avgdl are summed "
                             "over the ranks)")
        self.enable_dense, self.enable_sparse = enable_dense, enable_sparse
        self.enable_full_text, self.bm25_k1, self.bm25_b = bool(enable_full_text), float(bm25_k1), float(bm25_b)
        self.dense_dim, self.sparse_vocab, self.dense_dtype, self.device = dense_dim, sparse_vocab, dense_dtype, device
        self.dense_headroom = max(1.0, float(dense_headroom))
        if dense_prefilter not in ("auto", True, False):
            raise ValueError(f"dense_prefilter must be 'auto', True or False (got {dense_prefilter!r})")
        self.dense_prefilter = dense_prefilter
        self._comm = comm
        self._owns_comm = False
        if comm is None and distributed:
            from .distributed import ShardComm

            self._comm = ShardComm(group, device)
            self._owns_comm = True
        self.rrf_route = rrf_route
        self.filter_route = filter_route
        self.filter_eval = filter_eval
        self.filter_strings = filter_strings
        self.index_type, self.nlist, self.nprobe = index_type, int(nlist), int(nprobe)
        self.auto_compact = None if auto_compact is None else float(auto_compact)
        self._epoch = 0              # advanced by every compaction, under the lock (class docstring)
        self._ivf_trained_rows = 0   # rows in the shard when its overlay was last trained (0 = no overlay)
        self.m, self.nbits = (int(m), 8) if index_type == "PQ" else (None, None)
        self._pq_codebooks: Optional[np.ndarray] = None   # float32 [m, 256, dense_dim // m] once trained (or loaded): frozen
        self._pq_trained_rows = 0    # rows of the sample they were trained on
        # the route searches take: the filtered search returns host lists, which the device-resident exchange does not carry.
        # Replicated configuration only, so every rank decides alike.
        self._filter_route = filter_route
        if filter_route == "bitmap" and self._comm is not None and getattr(self._comm, "on_gpu", False):
            self._filter_route = "subset"
            logger.info("GpuVectorStore: filter_route='bitmap' needs host result lists; the exchange runs on the GPU, keeping 'subset'")
        self._rank = self._comm.rank if self._comm is not None else 0
        self._world = self._comm.world if self._comm is not None else 1
        self._payload_sharded = self._world > 1 and payload == "sharded"
        # full text goes through the exchange (statistics sums + list merge) exactly where `_device_topk` does
        self._text_sharded = self.enable_full_text and self._comm is not None and (self._world > 1 or self._comm.on_gpu)
        self._text_totals: Optional[Tuple[int, int]] = None   # corpus-wide (N, sum dl), None = to be summed again
        # replicated on every rank, indexed by global row
        self._ids: List[str] = []
        self._alive = _Column(bool)
        self._id_rows: Optional[Dict[str, Any]] = None        # id -> row (or rows), built by the first delete
        # texts / metadata: indexed by global row, or by local row when the payload is sharded
        self._texts: List[str] = []
        self._enh: List[str] = []
        self._meta: List[Dict[str, Any]] = []
        # this rank's shard, indexed by local row; `_owned.data[j]` = global row of local row j (ascending)
        self._owned = _Column(np.int64)
        self._dense_rows = _Column(np.float32, dense_dim) if enable_dense else None
        self._sp_ptr = _Column(np.int64, first=[0])
        self._sp_idx = _Column(np.int32)
        self._sp_val = _Column(np.float32)
        self._dense: Optional[DenseShard] = None
        self._dense_cap = 0          # capacity of the resident dense shard
        self._dense_flushed = 0      # local rows already in it
        self._sparse_parts: List[Tuple[Any, int, int]] = []   # (SELL image, first local row, rows): main [+ tail]
        self._sparse_flushed = 0
        self._text: Optional[TextIndex] = None      # BM25 index of the raw texts (local rows), main [+ tail] segments
        self._text_flushed = 0
        self._text_main = 0          # rows in its main segment
        self._text_live_stale = False
        self._main_rows: np.ndarray = np.zeros(0, np.int64)   # _owned.data at the last flush
        self._owned_dev = None       # the same table in HBM (RCCL exchange): (torch tensor, rows)
        self._dirty = False
        # Callers arrive from asyncio.to_thread workers (index.py:552-655 under api/): inserts, deletes, the flush and the
        # cache fills are serialised by this lock; searches run outside it on the shard objects they captured, and a shard
        # that has been replaced or evicted is released by its last user (DenseShard / SparseShard.__del__), never closed
        # under a running search.  (Sharded stores are SPMD: one caller thread per rank.)
        self._mu = threading.RLock()
        self._masks: Dict[str, Optional[np.ndarray]] = {}
        # what is derived from the rows of `_meta`: value indexes, typed columns, group codes, and the device copies of the
        # last two, made through the names this module holds when one is needed (header comment).  The factories close over
        # `device`, not `self`: the store stays free of reference cycles and releases its HBM when its last user lets go
        # (so `self.device` is assigned once, above, and never rebound: the handles would not follow it)
        self._metadata = StoreMetadata(lambda: RowFilter(device), lambda: GroupColumn(device))
        self._all_ids_truthy = True
        # replicated like `_all_ids_truthy`: no two rows share an id (the ids seen so far, until two of them do).  Rows that
        # share an id are ONE candidate of a hybrid fusion (hybrid_search.py:73-129 keys by id); deletes leave it as it is.
        self._ids_unique = True
        self._id_seen: Optional[set] = set()
        self._documents: Dict[str, Dict[str, Any]] = {}      # document records (add_documents / get_document)
        self._subsets: Dict[Any, Tuple[Any, np.ndarray, Any]] = {}   # (kind, mask bytes) -> (subset shard, global row of each subset row, device copy)

    def __len__(self) -> int:
        return len(self._ids)

    def close(self) -> None:
        """Drops the resident shards and, when the store created its own `ShardComm`, the library's RCCL communicator -- call
        it on every rank before `torch.distributed.destroy_process_group()` (a communicator left to the garbage collector may
        be destroyed after torch's process group is gone).  The store is empty afterwards."""
        with self._mu:
            self._subsets.clear()
            self._dense = None              # released by their last user (DenseShard / SparseShard.__del__)
            self._sparse_parts = []
            self._text = None
            self._owned_dev = None
            self._metadata.drop_device()
            self._dense_flushed = self._sparse_flushed = self._text_flushed = self._text_main = 0
            self._dirty = True
            if self._comm is not None and self._owns_comm:
                self._comm.close()

    # -------------------------------------------------------------- ingest
    def add_vectors(self, ids, dense_vectors, sparse_vectors, texts, enhanced_texts, metadatas):
        if self.enable_dense and (dense_vectors is None or len(dense_vectors) == 0):
            raise ValueError("Dense vectors required but not provided")          # milvus_base.py:101-104
        if self.enable_sparse and (sparse_vectors is None or
                                   (len(sparse_vectors) == 0 if not hasattr(sparse_vectors, "indptr") else sparse_vectors.shape[0] == 0)):
            raise ValueError("Sparse vectors required but not provided")
        # Build and validate every new row BEFORE touching the store (the reference assembles the whole batch and
        # inserts it in one call, milvus_base.py:90-127): a malformed entry leaves the store exactly as it was.
        n = len(ids)
        for name, col in (("texts", texts), ("enhanced_texts", enhanced_texts), ("metadatas", metadatas)):
            if len(col) != n:
                raise ValueError(f"add_vectors: {len(col)} {name} for {n} ids")
        lo, hi = (0, n)
        if self._world > 1:
            from .distributed import shard_range

            lo, hi = shard_range(n, self._rank, self._world)
        new_dense = None
        if self.enable_dense:
            if len(dense_vectors) != n:
                raise ValueError(f"add_vectors: {len(dense_vectors)} dense_vectors for {n} ids")
            try:
                block = np.asarray(dense_vectors, dtype=np.float32)
            except ValueError:
                block = None                                   # ragged rows: name the first offender below
            if block is None or block.ndim != 2 or block.shape[1] != self.dense_dim:
                for i, v in enumerate(dense_vectors):
                    shape = np.asarray(v, dtype=np.float32).shape
                    if shape != (self.dense_dim,):
                        raise ValueError(f"add_vectors: dense vector {i} has shape {shape}, the store holds {self.dense_dim}-d rows")
                raise ValueError(f"add_vectors: dense_vectors must be [n, {self.dense_dim}]")
            new_dense = np.empty((hi - lo, self.dense_dim), np.float32)
            slab = 16384                                     # a cache-sized slab at a time into one reused scratch: no
            sq = np.empty((min(slab, max(1, hi - lo)), self.dense_dim), np.float32)   # [n, dim] temporaries at 10^6 rows
            for a in range(lo, hi, slab):
                mine = block[a:min(hi, a + slab)]
                np.multiply(mine, mine, out=sq[: len(mine)])
                norms = np.sqrt(sq[: len(mine)].sum(axis=1, dtype=np.float32))
                np.divide(mine, np.where(norms > 0, norms, np.float32(1.0))[:, None], out=new_dense[a - lo:a - lo + len(mine)])   # COSINE == IP on unit rows
        new_csr = None
        if self.enable_sparse:
            indptr, indices, values = _as_csr(sparse_vectors, n, self.sparse_vocab)
            new_csr = (indptr[lo:hi + 1] - indptr[lo], indices[indptr[lo]:indptr[hi]], values[indptr[lo]:indptr[hi]])
        keep = slice(lo, hi) if self._payload_sharded else slice(0, n)
        new_meta = _metadata_rows(metadatas[keep])                                # milvus_base.py:108-109
        new_texts, new_enh = list(texts[keep]), list(enhanced_texts[keep])
        with self._mu:
            self._note_unique(ids)              # first: an id that cannot be hashed leaves the store as it was
            base = len(self._ids)
            self._ids.extend(ids)
            if self._id_rows is not None:
                for i, x in enumerate(ids):
                    self._note_id(x, base + i)
            if self._all_ids_truthy:
                self._all_ids_truthy = all(bool(x) for x in ids)
            self._texts.extend(new_texts)
            self._enh.extend(new_enh)
            self._meta.extend(new_meta)
            self._alive.extend(np.ones(n, dtype=bool))
            self._owned.extend(np.arange(base + lo, base + hi, dtype=np.int64))
            if new_dense is not None:
                self._dense_rows.extend(new_dense, adopt=True)
            if new_csr is not None:
                self._sp_ptr.extend(new_csr[0][1:] + self._sp_ptr.data[-1])
                self._sp_idx.extend(new_csr[1])
                self._sp_val.extend(new_csr[2])
            self._dirty = True
            self._drop_subsets()
            self._metadata.extend(new_meta, len(self._meta) - len(new_meta))

    def _note_unique(self, ids) -> None:
        """Keeps `_ids_unique` in step with the ids of new rows (under the lock, or before the store is shared)."""
        seen = self._id_seen
        if seen is None:
            return
        before = len(seen)
        seen.update(ids)
        if len(seen) != before + len(ids):
            self._ids_unique, self._id_seen = False, None

    def _note_id(self, key, row: int) -> None:
        have = self._id_rows.get(key)
        if have is None:
            self._id_rows[key] = row
        elif isinstance(have, list):
            have.append(row)
        else:
            self._id_rows[key] = [have, row]

    def delete(self, ids: List[str]):
        with self._mu:
            if self._id_rows is None:                       # one pass over the ids, then O(1) per deleted id
                self._id_rows = {}
                for row, key in enumerate(self._ids):
                    self._note_id(key, row)
            alive = self._alive.data
            for key in ids:
                rows = self._id_rows.get(key)
                if rows is not None:
                    alive[rows] = False
            self._text_live_stale = True
            self._text_totals = None
            self._drop_subsets()
            if self.auto_compact is not None and len(alive) and 1.0 - float(alive.mean()) > self.auto_compact:
                self.compact()

    def compact(self) -> int:
        """Drops every deleted row from the host columns and the device structures (class docstring, "Compaction"); returns the
        number of rows reclaimed.  The rows that stay keep their order and are renumbered `0 .. len(self) - 1`.  Returns 0 and
        touches nothing when no row is dead.  Rows inserted since the last flush are flushed first, so that the device holds
        exactly the rows the bitmap speaks of.  ValueError on a sharded store."""
        if self._comm is not None:
            raise ValueError("compact() is single-GPU: sharded stores (distributed=True or a comm) keep their deleted rows until a save / load")
        with self._mu:
            keep = self._alive.data.copy()
            n, live = len(keep), int(keep.sum())
            if live == n:
                return 0
            self._flush()
            self._epoch += 1                     # before anything moves: a search that sees any of it answers again
            at = np.nonzero(keep)[0]
            # device: the dense rows in place, the overlay renumbered, the filter columns in place; sparse images and the
            # full-text index are dropped and rebuilt by the next flush from the compacted host copies (a SELL image is
            # sorted by row length and the BM25 postings by term: removing rows is a rebuild either way)
            if self._dense is not None:
                self._dense.compact(keep)
                overlay = getattr(self._dense, "ivf", None)
                if overlay is not None:
                    overlay.remap(keep)
                self._dense_flushed = live
            self._metadata.compact(keep)
            self._sparse_parts, self._sparse_flushed = [], 0
            self._text, self._text_flushed, self._text_main = None, 0, 0
            self._text_live_stale, self._text_totals = True, None
            # host columns
            self._ids, self._texts, self._enh, self._meta = (_take(col, at) for col in (self._ids, self._texts, self._enh, self._meta))
            self._alive = _Column(bool, first=np.ones(live, dtype=bool))
            self._owned = _Column(np.int64, first=np.arange(live, dtype=np.int64))
            self._main_rows = self._owned.data
            if self._dense_rows is not None:
                rows = _Column(np.float32, self.dense_dim)
                rows.extend(self._dense_rows.data[at], adopt=True)
                self._dense_rows = rows
            if self.enable_sparse:
                ptr, idx, val = csr_take_rows(self._sp_ptr.data, self._sp_idx.data, self._sp_val.data, at)
                self._sp_ptr, self._sp_idx, self._sp_val = _Column(np.int64, first=ptr), _Column(np.int32, first=idx), _Column(np.float32, first=val)
            # what a load would derive from the surviving rows
            self._id_rows = None
            self._all_ids_truthy = all(bool(x) for x in self._ids)
            self._ids_unique, self._id_seen = True, set()
            self._note_unique(self._ids)
            self._drop_subsets()
            self._dirty = self.enable_sparse or self.enable_full_text
            return n - live

    def _sparse_slice(self, a: int, b: int):
        """CSR of local rows [a, b)."""
        ptr = self._sp_ptr.data
        return ptr[a:b + 1] - ptr[a], self._sp_idx.data[ptr[a]:ptr[b]], self._sp_val.data[ptr[a]:ptr[b]]

    def _flush(self):
        with self._mu:
            if not self._dirty:
                return
            n = len(self._owned)
            # published before the device append: a search that is running on the resident shard decodes its hits with
            # the mapping it reads AFTER the kernel returns, so every row the kernel can have seen is in it
            self._main_rows = self._owned.data
            if self.enable_dense and n > self._dense_flushed:
                rows = self._dense_rows.data
                if self.index_type == "PQ" and self._pq_codebooks is None and n >= PQ_MIN_ROWS:
                    self._pq_train(rows)
                    self._dense = None                  # the exact shard goes: the PQ shard is built from the host rows below
                if self._dense is None or n > self._dense_cap:
                    # (re)build with head-room so later inserts append instead of re-uploading every row
                    self._dense = None                  # released now unless a search on another thread still holds it
                    self._dense_cap = max(1024, int(n * self.dense_headroom))
                    dense = self._new_dense_shard(self._dense_cap)
                    dense.add(rows)
                    self._dense = dense
                else:
                    self._dense.add(rows[self._dense_flushed:])
                self._dense_flushed = n
                if self._has_lists:
                    self._ivf_refresh(n)
            if self.enable_sparse and n > self._sparse_flushed:
                main = self._sparse_parts[0] if self._sparse_parts else None
                main_n = main[2] if main else 0
                if main is None or n - main_n > max(self.SPARSE_TAIL_MIN, main_n // 4):
                    self._sparse_parts = []             # one image of everything
                    self._sparse_parts = [(SparseShard(self.sparse_vocab, *self._sparse_slice(0, n), device=self.device), 0, n)]
                else:                                   # the main image stays; the rows behind it form the tail segment
                    tail = SparseShard(self.sparse_vocab, *self._sparse_slice(main_n, n), device=self.device)
                    self._sparse_parts = [main, (tail, main_n, n - main_n)]
                self._sparse_flushed = n
            if self._text_sharded:
                self._text_totals = None                # every rank, whatever its share of the new rows
                if self._text is None:                  # a rank without rows still answers the query analysis
                    self._text = TextIndex(self.bm25_k1, self.bm25_b, self.device)
            if self.enable_full_text and n > self._text_flushed:
                if self._text is None:
                    self._text = TextIndex(self.bm25_k1, self.bm25_b, self.device)
                fold = self._text_main == 0 or n - self._text_main > max(self.TEXT_TAIL_MIN, self._text_main // 4)
                if self._payload_sharded or self._world == 1:      # the text list is indexed by local row
                    fresh = self._texts[self._text_flushed:n]
                else:                                              # replicated payload: by global row
                    fresh = [self._texts[g] for g in self._owned.data[self._text_flushed:n].tolist()]
                self._text.add(fresh, fold=fold)
                if fold:
                    self._text_main = n
                self._text_flushed = n
                self._text_live_stale = True
            if self._comm is not None and self._comm.on_gpu and n:
                import torch

                self._owned_dev = (torch.from_numpy(np.ascontiguousarray(self._main_rows)).to(torch.device("cuda", self.device)), n)
            self._dirty = False

    def _pq_train(self, rows: np.ndarray) -> None:
        """The codebooks of an index_type="PQ" store, once (called by `_flush`, under the lock, by the flush that reaches
        `PQ_MIN_ROWS`): trained on at most `PQ_TRAIN_ROWS_MAX` evenly strided host rows by a `PqShard` made for it, read back and
        frozen -- every shard the store builds from here on gets them through `set_codebooks` (`_new_dense_shard`)."""
        n = len(rows)
        take = min(n, PQ_TRAIN_ROWS_MAX)
        sample = rows if take == n else rows[(np.arange(take, dtype=np.int64) * n) // take]
        trainer = PqShard(self.dense_dim, self.m, 1, self.device)
        trainer.train(sample, PQ_TRAIN_ITERS)
        self._pq_codebooks = np.ascontiguousarray(trainer.codebooks(), dtype=np.float32)
        self._pq_trained_rows = take
        trainer.close()
        self._drop_subsets()                            # subsets built from exact rows would answer with other bits

    def pq_stats(self) -> Optional[Dict[str, int]]:
        """`{"m", "rows", "trained_rows"}` of an index_type="PQ" store whose dense field is a `PqShard` after a flush; None while
        the store searches exact rows (another index_type, or fewer than `PQ_MIN_ROWS` rows so far)."""
        with self._mu:
            self._flush()
            if self._pq_codebooks is None or self._dense is None:
                return None
            return {"m": self.m, "rows": len(self._dense), "trained_rows": self._pq_trained_rows}

    @property
    def _has_lists(self) -> bool:
        """An IVF store (IVF_FLAT over fp32 / bf16 rows, IVF_SQ8 over int8 rows): its dense shard gets an overlay."""
        return self.index_type in IVF_INDEX_TYPES

    def _ivf_refresh(self, n: int) -> None:
        """Keeps the IVF overlay of the resident dense shard in step with its `n` rows (called by `_flush`, under the
        lock): trains (10 Lloyd rounds over 64 rows per list) on the first flush that reaches `IVF_MIN_ROWS`, when the shard
        has doubled since, and when the shard was rebuilt for capacity; every flush assigns the new rows to their lists."""
        shard = self._dense
        nlist_eff = ivf_effective_nlist(n, self.nlist)
        if nlist_eff == 0:
            return
        current = getattr(shard, "ivf", None)
        if current is None or n >= 2 * self._ivf_trained_rows:
            overlay = IvfOverlay(shard, nlist_eff)
            overlay.train(10, 64 * nlist_eff)
            overlay.sync()
            shard.ivf = overlay          # the overlay it replaces is released by its last user, like a replaced shard
            self._ivf_trained_rows = n
        else:
            current.sync()

    def ivf_stats(self) -> Optional[Dict[str, int]]:
        """`{"nlist", "rows", "largest_list", "trained_rows"}` of the dense shard's IVF_FLAT / IVF_SQ8 overlay after a flush; None
        while the store searches FLAT (index_type="FLAT", or fewer than `IVF_MIN_ROWS` rows)."""
        with self._mu:
            self._flush()
            overlay = getattr(self._dense, "ivf", None)
            if overlay is None:
                return None
            return dict(overlay.stats(), trained_rows=self._ivf_trained_rows)

    def _nprobe_of(self, search_params: Optional[Dict[str, Any]]) -> Optional[int]:
        """The dense leg's `nprobe` for one call; None on a FLAT store (`search_params` has nothing to say there)."""
        return parse_nprobe(search_params, self.nprobe) if self._has_lists else None

    def _main_parts(self, kind: str):
        """(segments of the resident shard as (shard, first local row), device row table, rows in the whole store)
        after a flush, captured under the lock."""
        with self._mu:
            self._flush()
            if kind == "dense":
                parts = [(self._dense, 0)] if self._dense is not None else []
            else:
                parts = [(sh, base) for sh, base, _n in self._sparse_parts]
            return parts, self._owned_dev, len(self._ids)

    # -------------------------------------------------------------- row payloads (texts, metadata)
    def _payload_slot(self, row: int) -> int:
        """Index of global row `row` in the text / metadata lists, -1 when another rank holds it."""
        if not self._payload_sharded:
            return row
        owned = self._owned.data
        j = int(np.searchsorted(owned, row))
        return j if j < len(owned) and owned[j] == row else -1

    def _payloads(self, rows) -> Dict[int, Tuple[str, str, Dict[str, Any]]]:
        """global row -> (text, enhanced text, metadata copy) for the given rows; sharded payloads meet in ONE object
        gather (every rank asks for the same rows and contributes the ones it holds)."""
        want = sorted({int(r) for r in rows if r >= 0})
        out = {}
        for r in want:
            j = self._payload_slot(r)
            if j >= 0:
                out[r] = (self._texts[j], self._enh[j], dict(self._meta[j]))
        if self._payload_sharded:
            merged: Dict[int, Tuple[str, str, Dict[str, Any]]] = {}
            for part in self._comm.gather_objects(out):
                merged.update(part)
            return merged
        return out

    # -------------------------------------------------------------- search
    def _mask(self, filter: Optional[str]) -> Optional[np.ndarray]:
        """Rows a query may return (alive and passing `filter`), or None for all; cached per filter string until the
        next insert / delete (one Python predicate call per row otherwise, on every query)."""
        key = filter or ""
        with self._mu:
            return self._mask_locked(key, filter)

    def _mask_locked(self, key: str, filter: Optional[str]) -> Optional[np.ndarray]:
        if key not in self._masks:
            alive = self._alive.data.copy()
            if filter:
                pred = parse_filter(filter)
                lookup = getattr(pred, "lookup", None)
                held = np.zeros(len(self._meta), dtype=bool)     # over the rows whose metadata this rank holds
                if lookup is not None:      # one `==` / `in` comparison (the reference's document_id filter, index.py:735-739)
                    index = self._metadata.value_index(lookup[0], self._meta)
                    for v in lookup[1]:
                        rows = index.get(v)
                        if rows is not None:
                            held[rows] = True
                else:
                    held = self._metadata.held(filter, self._meta, self.filter_strings) if self.filter_eval == "device" else None
                    if held is None:
                        held = np.asarray([bool(pred(md)) for md in self._meta], dtype=bool)
                if self._payload_sharded:
                    passing = np.zeros(len(alive), dtype=bool)
                    passing[self._owned.data[: len(held)][held]] = True
                    passing = self._comm.union_mask(passing)
                else:
                    passing = held
                alive = alive & passing
            if len(self._masks) >= 64:
                self._masks.clear()
            self._masks[key] = None if alive.all() else alive
        return self._masks[key]

    def _hit(self, row: int, score: float) -> dict:
        """A search hit in the shape `merge_hybrid_results` works on; the entity (text, metadata copy) is attached
        by `_results` only to the hits that survive the merge."""
        return {"id": self._ids[row], "distance": float(score), "_row": row}

    def _results(self, hits: List[dict]) -> List[SearchResult]:
        pay = self._payloads([h["_row"] for h in hits])
        return [SearchResult(id=h["id"], score=h["distance"], metadata=pay[h["_row"]][2], text=pay[h["_row"]][0],
                             enhanced_text=pay[h["_row"]][1]) for h in hits]

    def _search(self, kind: str, query, limit: int, mask: Optional[np.ndarray], nprobe: Optional[int] = None) -> List[dict]:
        return self._search_batch(kind, [query], limit, mask, nprobe)[0]

    def _unit_queries(self, queries: Sequence[Any]) -> np.ndarray:
        """COSINE: unit queries against the unit rows (fp32 norm, one row at a time or all at once: same bits)."""
        rows_q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32).reshape(len(queries), self.dense_dim))
        norms = np.sqrt((rows_q * rows_q).sum(axis=1, dtype=np.float32))
        return rows_q / np.where(norms > 0, norms, np.float32(1.0))[:, None]

    def _segment_lists(self, parts, mapping: Optional[np.ndarray], Q: int, k: int, search_one):
        """The segment loop of every host route -> this rank's (`scores [Q, k]`, GLOBAL `rows [Q, k]`, -1 = no hit).
        `search_one(shard, base)` returns a segment's (scores, LOCAL rows); `mapping[j]` = global row of local row j (None =
        the resident table).  Lists of several segments are merged on the GPU; no segment gives empty lists."""
        found_lists = []
        for shard, base in parts:
            sc, local = search_one(shard, base)
            # the resident table is read AFTER the kernel returned: every row the kernel can have seen is in it (`_flush`)
            rows_of = mapping if mapping is not None else self._main_rows
            at = local + base
            found = (local >= 0) & (at < len(rows_of))
            g = np.where(found, rows_of[np.where(found, at, 0)], -1) if len(rows_of) else np.full_like(local, -1)
            found_lists.append((sc, g))
        if not found_lists:
            return np.full((Q, k), -np.inf, np.float32), np.full((Q, k), -1, np.int64)
        if len(found_lists) == 1:
            return found_lists[0]
        return _merge_parts(np.stack([np.where(g >= 0, sc, -np.inf).astype(np.float32) for sc, g in found_lists]),
                            np.stack([g for _sc, g in found_lists]), k, self.device)

    def _exchange_host(self, scores: np.ndarray, rows: np.ndarray, k: int):
        """This rank's host lists -> the lists merged over all ranks; a store without an exchange keeps its own."""
        # The bitmap route (`_filtered_topk`) never gets here with `comm.on_gpu`: it produces host lists, which the
        # device-resident exchange does not carry, so the constructor keeps such a store on filter_route="subset".
        comm = self._comm
        if comm is not None and (self._world > 1 or comm.on_gpu):
            return comm.allgather_merge(scores, rows, k)
        return scores, rows

    def _resident_slots(self, Q: int, k: int):
        """(current stream of the store's device, the exchange's HBM payload for `[Q, k]` lists, its ids ptr, its scores ptr)."""
        import torch

        stream = C.c_void_p(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        payload, ids_ptr, scores_ptr = self._comm.exchange_buffers(Q, k)
        return stream, payload, ids_ptr, scores_ptr

    def _device_topk(self, kind: str, parts, shard_rows: Optional[np.ndarray], queries: Sequence[Any], k: int,
                     rows_dev=None, nprobe: Optional[int] = None):
        """Top-k of `queries` over one (possibly sharded) set of rows -> (`scores [Q, k]`, GLOBAL `rows [Q, k]`, -1 = no
        hit).  `parts` are this rank's segments as (shard, first local row) (empty when it holds none of the rows) and
        `shard_rows[j]` the global row of local row j (None = the resident main shard, whose append-only mapping is read
        after the search; `rows_dev` = the same table in HBM); with more than one rank the per-shard lists meet in one
        all-gather and are merged on the GPU.  `nprobe` (IVF_FLAT / IVF_SQ8 stores, the dense leg's first pass): a shard with an overlay
        answers lists of up to `IVF_K_MAX` rows from its `nprobe` nearest lists instead of streaming every row."""
        Q = len(queries)
        comm = self._comm
        q_in = self._unit_queries(queries) if kind == "dense" and parts else queries
        if comm is not None and comm.on_gpu and k <= self.DEVICE_K and (rows_dev is not None or not parts):
            return self._device_topk_resident(parts, rows_dev, q_in, Q, k)

        def search_one(shard, _base):
            ivf = getattr(shard, "ivf", None) if nprobe is not None and k <= IVF_K_MAX else None
            if ivf is not None:
                return ivf.search(q_in, k, nprobe)
            return shard.search(q_in, k)               # dicts_to_csr converts sparse keys / weights to int32 / float32

        return self._exchange_host(*self._segment_lists(parts, shard_rows, Q, k, search_one), k)

    def _device_topk_resident(self, parts, rows_dev, q_in, Q: int, k: int):
        """The RCCL form of `_device_topk`: every segment writes its `[Q, k]` lists (global rows through the device
        table) into HBM, segments are merged on the device, the payload goes through ONE all-gather and the cross-rank
        merge; only the merged result is copied to the host."""
        stream, payload, ids_ptr, scores_ptr = self._resident_slots(Q, k)
        n = Q * k
        if not parts:
            _lib.check("vrag_topk_fill_empty", self._lib.vrag_topk_fill_empty(C.c_void_p(scores_ptr), C.c_void_p(ids_ptr), n, self.device, stream))
        else:
            import torch

            table, n_map = rows_dev
            if len(parts) == 1:
                slots = [(scores_ptr, ids_ptr)]
            else:
                seg_s = torch.empty((len(parts), n), dtype=torch.float32, device=payload.device)
                seg_i = torch.empty((len(parts), n), dtype=torch.int64, device=payload.device)
                slots = [(seg_s[p].data_ptr(), seg_i[p].data_ptr()) for p in range(len(parts))]
            for (shard, base), (sp, ip) in zip(parts, slots):
                shard.search_device(q_in, k, sp, ip, row_map=table.data_ptr() + 8 * base, n_map=n_map - base, stream=stream)
            if len(parts) > 1:
                _lib.check("vrag_topk_merge", self._lib.vrag_topk_merge(
                    C.c_void_p(seg_s.data_ptr()), C.c_void_p(seg_i.data_ptr()), len(parts), Q, k, k, 0, 0,
                    C.c_void_p(scores_ptr), C.c_void_p(ids_ptr), 1, self.device, stream))
        return self._comm.allgather_merge_device(payload, Q, k, k)

    def _subset(self, kind: str, mask: np.ndarray):
        """A shard holding only this rank's rows that pass `mask` (Milvus filters before it searches,
        milvus_base.py:240-262, so a selective filter must still return its best rows however far down the unfiltered
        ranking they are).  Built from the host copies, cached per (kind, mask) until the next insert / delete; returns
        (segments, global row of each subset row, device copy of that table) -- rows ascending, so the kernels'
        `(score desc, id asc)` order carries over."""
        key = (kind, mask.tobytes())
        with self._mu:
            hit = self._subsets.get(key)
            if hit is None:
                owned = self._owned.data
                known = owned < len(mask)                     # rows inserted after the caller built its mask are not in it
                local = np.nonzero(known & mask[np.where(known, owned, 0)])[0] if len(owned) else np.zeros(0, np.int64)
                shard = None
                if len(local) and kind == "dense":
                    shard = self._new_dense_shard(len(local))
                    shard.add(self._dense_rows.data[local])
                elif len(local):
                    shard = SparseShard(self.sparse_vocab, *csr_take_rows(self._sp_ptr.data, self._sp_idx.data, self._sp_val.data, local),
                                        device=self.device)
                rows = owned[local] if len(owned) else local
                dev = None
                if shard is not None and self._comm is not None and self._comm.on_gpu:
                    import torch

                    dev = (torch.from_numpy(np.ascontiguousarray(rows)).to(torch.device("cuda", self.device)), len(rows))
                while len(self._subsets) >= self.SUBSET_CACHE:
                    self._subsets.pop(next(iter(self._subsets)))          # freed when its last user lets go
                hit = self._subsets[key] = ([(shard, 0)] if shard is not None else [], rows, dev)
            return hit

    def _filtered_topk(self, kind: str, parts, queries: Sequence[Any], k: int, mask: np.ndarray):
        """`_device_topk` among the rows that pass `mask` (global rows), on the RESIDENT segments (`filter_route="bitmap"`):
        per segment the mask is taken at the segment's rows and packed again from its first local row (segments start at
        arbitrary rows, so this is no word offset); rows beyond the mask do not pass.  The segments' `[Q, k]` lists are
        merged like the unfiltered ones and, on a sharded store, meet in the host exchange."""
        q_in = self._unit_queries(queries) if kind == "dense" and parts else queries
        mapping = self._main_rows

        def search_one(shard, base):
            seg_rows = mapping[base:base + (len(shard) if kind == "dense" else shard.n_docs)]
            known = seg_rows < len(mask)
            allow = known & mask[np.where(known, seg_rows, 0)]
            return shard.search_filtered(q_in, k, _bitmap(allow), len(allow))

        return self._exchange_host(*self._segment_lists(parts, mapping, len(queries), k, search_one), k)

    def _drop_subsets(self):
        with self._mu:
            self._subsets.clear()
            self._masks.clear()

    def _check_limit(self, limit: int) -> None:
        if limit > self.K_LIMIT:
            raise ValueError(f"GpuVectorStore: a search may ask for at most {self.K_LIMIT} rows per method "
                             f"(got {limit}; hybrid search asks for 2 * top_k)")

    @staticmethod
    def _fit_mask(mask: Optional[np.ndarray], n: int) -> Optional[np.ndarray]:
        """`mask` over exactly `n` rows: rows that were inserted after the caller built it do not pass."""
        if mask is None or len(mask) == n:
            return mask
        return np.concatenate([mask, np.zeros(n - len(mask), dtype=bool)]) if len(mask) < n else mask[:n]

    @staticmethod
    def _no_hits(Q: int, limit: int) -> Tuple[np.ndarray, np.ndarray]:
        return np.full((Q, limit), -1, np.int64), np.zeros((Q, limit), np.float32)

    @staticmethod
    def _put_hits(rows_out: np.ndarray, score_out: np.ndarray, at, scores: np.ndarray, rows: np.ndarray,
                  n: Optional[int] = None) -> None:
        """Merged lists into the results at `at`: rows outside `[0, n)` (`n` None: negative rows) become -1, their scores 0."""
        found = rows >= 0 if n is None else (rows >= 0) & (rows < n)
        rows_out[at] = np.where(found, rows, -1)
        score_out[at] = np.where(found, scores, np.float32(0.0))

    def _topk_rows(self, kind: str, queries: Sequence[Any], limit: int, mask: Optional[np.ndarray],
                   _retry: int = 0, nprobe: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Best `limit` rows per query among the rows that pass `mask`: `rows [Q, limit]` (-1 = no hit, tail only) and
        their fp32 scores.  One device pass for the whole batch over the full shard; queries that come up short because
        filtered / deleted rows took their slots (and every query when the filter passes under 1/8 of the rows) get a
        second pass over the masked subset shard -- or, with `filter_route="bitmap"`, the filtered search of the resident
        shard (`_filtered_topk`; no subset shard is built in that mode).  `nprobe` (dense leg of an IVF_FLAT / IVF_SQ8 store): the full pass looks at the rows of that many
        lists only (`_device_topk`); the second pass stays exact.  Every branch below depends only on replicated state and on merged
        results, so the ranks of a sharded store take the same path and meet in the same collectives."""
        self._check_limit(limit)
        parts, rows_dev, n = self._main_parts(kind)
        mask = self._fit_mask(mask, n)
        Q = len(queries)
        rows_out, score_out = self._no_hits(Q, limit)
        k = limit
        n_pass = n if mask is None else int(mask.sum())
        if n == 0 or Q == 0 or n_pass == 0:
            return rows_out, score_out
        want = min(k, n_pass)
        short = np.ones(Q, dtype=bool)
        if mask is None or n_pass * 8 >= n:
            scores, rows = self._device_topk(kind, parts, None, queries, k, rows_dev, nprobe if kind == "dense" else None)
            if (rows >= n).any() and _retry < 3:      # rows inserted while this search ran took slots: search again
                return self._topk_rows(kind, queries, limit, mask, _retry + 1, nprobe)
            rows = np.where(rows < n, rows, -1)
            found = rows >= 0
            valid = found if mask is None else found & mask[np.where(found, rows, 0)]
            count = valid.sum(axis=1)
            # a sparse query can have fewer than `want` rows sharing a term: then the full pass, which returned fewer
            # than k candidates, has already seen every match
            done = (count >= want) | (found.sum(axis=1) < k) if mask is not None else np.ones(Q, dtype=bool)
            if mask is not None and kind == "dense" and nprobe is not None:
                done = count >= want                  # a short IVF list has not seen every row: the exact pass answers
            order = np.argsort(~valid, axis=1, kind="stable")                   # passing hits first, ranking kept
            rows_c = np.take_along_axis(rows, order, axis=1)
            scores_c = np.take_along_axis(scores, order, axis=1)
            rows_c[np.arange(k)[None, :] >= count[:, None]] = -1
            self._put_hits(rows_out, score_out, done, scores_c[done], rows_c[done])
            short = ~done
        if short.any():
            which = np.nonzero(short)[0]
            if self._filter_route == "bitmap":
                scores, rows = self._filtered_topk(kind, parts, [queries[i] for i in which], want, mask)
            else:
                sub_parts, shard_rows, sub_dev = self._subset(kind, mask)
                scores, rows = self._device_topk(kind, sub_parts, shard_rows, [queries[i] for i in which], want, sub_dev)
            self._put_hits(rows_out, score_out, (which, slice(0, want)), scores, rows, n)
        return rows_out, score_out

    def _text_topk(self, queries: Sequence[str], limit: int, mask: Optional[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        """BM25 top-`limit` of a batch of query texts among the rows that pass `mask` -- `rows [Q, limit]` (-1 = no hit)
        and fp32 scores, as `_topk_rows`.  One device pass for the batch; the filter is a row bitmap the scoring kernel
        reads (no subset index), the statistics are those of the live rows."""
        self._check_limit(limit)
        if self._text_sharded:
            return self._text_topk_sharded(queries, limit, mask)
        with self._mu:
            text, n, _owned = self._text_snapshot()
        Q = len(queries)
        rows_out, score_out = self._no_hits(Q, limit)
        if text is None or n == 0 or Q == 0:
            return rows_out, score_out
        # rows inserted after the caller built its mask lie beyond it: the library does not return them (nor any row an
        # insert from another thread adds while this search runs, whatever `n` was)
        if mask is not None and not mask.any():
            return rows_out, score_out
        scores, rows = text.search([q or "" for q in queries], limit, mask)
        self._put_hits(rows_out, score_out, slice(None), scores, rows)
        return rows_out, score_out

    def _text_snapshot(self):
        """Opens both full-text routes, under the lock: flush, then (index, local rows it holds, their global rows); the
        index's live rows, and with them its statistics, follow the deletes here."""
        self._flush()
        text, n_local = self._text, self._text_flushed
        owned = self._owned.data[:n_local]
        if text is not None and self._text_live_stale:
            if n_local:
                text.set_live(self._alive.data[owned])
            self._text_live_stale = False
        return text, n_local, owned

    def _text_topk_sharded(self, queries: Sequence[str], limit: int, mask: Optional[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        """`_text_topk` on a row-sharded store.  Every rank scores its own rows with the corpus-wide statistics: `(N, sum dl)`
        summed over the ranks once after a change (cached), the `df` vector of the batch summed once per batch; the local
        lists go through the exchange of `_device_topk` (host lists, or HBM-resident under RCCL for k <= DEVICE_K).  Every
        branch depends on replicated state only (row count, query count, the OR-reduced mask, the summed N), so the ranks
        meet in the same collectives; a rank without rows enters them with zeros and empty lists.  Like every search of a
        sharded store, this route must be driven from ONE thread per rank: the statistics sum runs under the store's lock and
        the df sum under the index's, so two threads querying on one rank could order their collectives differently from the
        peer rank."""
        comm = self._comm
        with self._mu:
            text, n_local, owned = self._text_snapshot()
            n = len(self._ids)
            if text is not None and self._text_totals is None:
                own = text.stats()
                tot = comm.sum_int64([own["live"], own["sum_dl"]])
                text.set_corpus_stats(int(tot[0]), int(tot[1]))
                self._text_totals = (int(tot[0]), int(tot[1]))
            totals, owned_dev = self._text_totals, self._owned_dev
        Q = len(queries)
        rows_out, score_out = self._no_hits(Q, limit)
        if text is None or n == 0 or Q == 0 or totals[0] == 0:
            return rows_out, score_out
        mask = self._fit_mask(mask, n)
        if mask is not None and not mask.any():
            return rows_out, score_out
        allow = mask[owned] if mask is not None else None       # the global-row mask at this rank's rows
        texts = [q or "" for q in queries]
        k = limit
        if comm.on_gpu and k <= self.DEVICE_K:
            stream, payload, ids_ptr, scores_ptr = self._resident_slots(Q, k)
            table, n_map = owned_dev if (owned_dev is not None and n_local) else (None, 0)
            text.search_sharded(texts, k, allow, totals[0], comm.sum_int64,
                                device_out=(scores_ptr, ids_ptr, table.data_ptr() if table is not None else None, min(n_map, n_local), stream))
            scores, rows = comm.allgather_merge_device(payload, Q, k, k)
        else:
            scores, local = text.search_sharded(texts, k, allow, totals[0], comm.sum_int64)
            found = (local >= 0) & (local < n_local)
            rows = np.where(found, owned[np.where(found, local, 0)], -1) if n_local else np.full_like(local, -1)
            scores, rows = self._exchange_host(np.where(rows >= 0, scores, -np.inf).astype(np.float32), rows, k)
        self._put_hits(rows_out, score_out, slice(None), scores, rows, n)
        return rows_out, score_out

    def _search_batch(self, kind: str, queries: Sequence[Any], limit: int, mask: Optional[np.ndarray],
                      nprobe: Optional[int] = None) -> List[List[dict]]:
        rows, scores = (self._text_topk(queries, limit, mask) if kind == "full_text"
                        else self._topk_rows(kind, queries, limit, mask, nprobe=nprobe))
        return [[self._hit(int(r), float(v)) for r, v in zip(rows[i], scores[i]) if r >= 0] for i in range(len(queries))]

    def _results_batch(self, rows: np.ndarray, distances: np.ndarray) -> List[List[SearchResult]]:
        """`[Q, k]` merged rows / scores -> result lists; the payloads of the whole batch are fetched at once."""
        pay = self._payloads(rows.reshape(-1))
        ids = self._ids
        return [[SearchResult(id=ids[r], score=float(d), metadata=dict(pay[r][2]), text=pay[r][0], enhanced_text=pay[r][1])
                 for r, d in zip(rows[i].tolist(), distances[i].tolist()) if r >= 0] for i in range(rows.shape[0])]

    def _hybrid_batch(self, queries: Dict[str, Sequence[Any]], top_k, mask, weights, rrf_k,
                      nprobe: Optional[int] = None) -> List[List[SearchResult]]:
        """Every method of `queries` (method -> the batch's queries, in fusion order) for all queries, 2 * top_k rows each,
        then weighted RRF: one array merge for the whole batch, or query by query when an id is falsy (such hits keep
        their rank but are skipped) or rows share an id (they are one candidate, as in `query`).  A failing full-text leg is left out with a warning, as in `_hybrid_search_with_weights`;
        with one method left, its first top_k are the answer."""
        limit = top_k * 2
        lists: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
        for m, q in queries.items():
            if m != "full_text":
                lists[m] = self._topk_rows(m, q, limit, mask, nprobe=nprobe)
                continue
            try:                                                   # as the per-query path (milvus_base.py:420-431)
                lists[m] = self._text_topk(q, limit, mask)
            except Exception as e:
                if self._world > 1:
                    raise                                  # ranks must not diverge into different collectives
                logger.warning("Full text search failed: %s, excluding from hybrid", e)
        Q = len(next(iter(queries.values())))
        if not lists:
            logger.warning("Hybrid search: no valid methods executed after validation")
            return [[] for _ in range(Q)]
        if len(lists) == 1:                                        # one method: its first top_k
            rows, scores = next(iter(lists.values()))
            return self._results_batch(rows[:, :top_k], scores[:, :top_k])
        if self._all_ids_truthy and self._ids_unique:
            ranked = {m: r for m, (r, _s) in lists.items()}
            if self.rrf_route == "device" and Q >= self.RRF_DEVICE_MIN_QUERIES:
                rows, dist = rrf_fuse_rows_device(ranked, top_k, weights, rrf_k, self.device)
            else:
                rows, dist = rrf_merge_rows(ranked, top_k, weights, rrf_k)
            return self._results_batch(rows, dist)
        out = []
        for i in range(Q):
            rbm = {m: [self._hit(int(r), float(v)) for r, v in zip(rows[i], sc[i]) if r >= 0] for m, (rows, sc) in lists.items()}
            out.append(self._results(merge_hybrid_results(rbm, top_k, weights, rrf_k)))
        return out

    @_one_epoch
    def query_batch(self, dense_queries: Optional[Sequence[Any]] = None, sparse_queries: Optional[Sequence[Any]] = None,
                    text_queries: Optional[Sequence[Optional[str]]] = None, top_k: int = 5, search_type: str = "hybrid",
                    filter: Optional[str] = None, search_params: Optional[Dict[str, Any]] = None,
                    hybrid_weights: Optional[Dict[str, float]] = None, rrf_k: int = 60) -> List[List[SearchResult]]:
        """Cross-query form of `query`: element i equals `query(dense_queries[i], sparse_queries[i], ...)`,
        with the dense and the sparse searches of all queries done as one batched device pass each (the batched
        kernels order hits by `(score desc, id asc)` like the single-query ones).  Queries that take one of `query`'s
        side branches (no vectors, a missing half in hybrid mode) are answered by `query` itself.  On a bf16 shard a
        batch of >= 3 dense queries runs on the matrix cores with every fp32 query carried as a (bf16, bf16 remainder)
        pair (16 significant bits; include/vrag_amd.h, vrag_dense_index_search): scores then agree with the single-query
        fp32 path to fp32 summation noise; an f32 shard (the default) uses fp32 queries at every batch size.
        `top_k` (2 * top_k in hybrid mode) may not exceed `K_LIMIT` = 1024: ValueError otherwise."""
        n = max(len(x) for x in (dense_queries, sparse_queries, text_queries) if x is not None)
        dq = list(dense_queries) if dense_queries is not None else [None] * n
        sq = list(sparse_queries) if sparse_queries is not None else [None] * n
        tq = list(text_queries) if text_queries is not None else [None] * n
        if not (len(dq) == len(sq) == len(tq) == n):
            raise ValueError("query_batch: dense_queries / sparse_queries / text_queries differ in length")

        grouping = parse_grouping(search_params)
        if grouping is not None:
            self._check_grouped_call(search_type, hybrid_weights, top_k, all(_is_given(q) for q in dq),
                                     any(not _is_given(d) and not _is_given(s) for d, s in zip(dq, sq)))
            return self._grouped_batch(dq, top_k, filter, grouping)

        def single(i):
            return self.query(dense_query=dq[i], sparse_query=sq[i], text_query=tq[i], top_k=top_k, search_type=search_type,
                              filter=filter, search_params=search_params, hybrid_weights=hybrid_weights, rrf_k=rrf_k)

        def is_set(q):   # `query` tests vectors by truthiness (milvus_base.py:232,243,254)
            return q is not None and len(q) > 0

        if hybrid_weights is not None:
            weights = sanitize_hybrid_weights(hybrid_weights)
            if "full_text" in weights and not self.enable_full_text:
                weights = {k: v for k, v in weights.items() if k != "full_text"}
            d_some, s_some, t_some = [q is not None for q in dq], [q is not None for q in sq], [q is not None for q in tq]
            uniform = all(all(x) or not any(x) for x in (d_some, s_some, t_some))
            use = {"dense": ("dense" in weights and all(d_some), dq), "sparse": ("sparse" in weights and all(s_some), sq),
                   "full_text": ("full_text" in weights and all(t_some), tq)}
            queries = {m: q for m, (on, q) in use.items() if on}
            if not weights or not uniform or not queries:
                return [single(i) for i in range(n)]          # mixed / degenerate batches: the per-query code decides
            mask = self._mask(filter)
            return self._hybrid_batch(queries, top_k, mask, weights, rrf_k, self._nprobe_of(search_params))
        if search_type == "full_text" and self.enable_full_text and all(q for q in tq):
            mask = self._mask(filter)
            return self._results_batch(*self._text_topk(tq, top_k, mask))
        if search_type == "dense" and all(is_set(q) for q in dq):
            mask = self._mask(filter)
            return self._results_batch(*self._topk_rows("dense", dq, top_k, mask, nprobe=self._nprobe_of(search_params)))
        if search_type == "sparse" and all(is_set(q) for q in sq):
            mask = self._mask(filter)
            return self._results_batch(*self._topk_rows("sparse", sq, top_k, mask))
        if search_type == "hybrid" and all(is_set(q) for q in dq) and all(is_set(q) for q in sq):
            mask = self._mask(filter)
            nprobe = self._nprobe_of(search_params)        # a bad nprobe is the caller's ValueError, not a failed batch
            try:
                return self._hybrid_batch({"dense": dq, "sparse": sq}, top_k, mask, {"dense": 0.5, "sparse": 0.5}, rrf_k, nprobe)
            except Exception as e:
                if self._world > 1:
                    raise                                  # ranks must not diverge into different collectives
                logger.warning("Batched hybrid search failed: %s, answering per query", e)
        return [single(i) for i in range(n)]

    @_one_epoch
    def query(self, dense_query=None, sparse_query=None, text_query=None, top_k: int = 5, search_type: str = "hybrid",
              filter: Optional[str] = None, search_params: Optional[Dict[str, Any]] = None,
              hybrid_weights: Optional[Dict[str, float]] = None, rrf_k: int = 60) -> List[SearchResult]:
        """milvus_base.py:189-313.  `top_k` (2 * top_k in hybrid mode) may not exceed `K_LIMIT` = 1024.
        `search_params={"group_by_field": key, "group_size": g}` (`parse_grouping`) makes a dense query a grouping search: the
        best `top_k` groups of `metadata[key]`, each with its best `g` rows, as one flat list group by group (`_grouped_batch`)."""
        grouping = parse_grouping(search_params)
        if grouping is not None:
            self._check_grouped_call(search_type, hybrid_weights, top_k, _is_given(dense_query),
                                     not _is_given(dense_query) and not _is_given(sparse_query))
            return self._grouped_batch([dense_query], top_k, filter, grouping)[0]
        if hybrid_weights is not None:
            return self._hybrid_search_with_weights(dense_query, sparse_query, text_query, top_k, filter, hybrid_weights, rrf_k,
                                                    self._nprobe_of(search_params))
        if search_type == "full_text" and text_query and self.enable_full_text:   # milvus_base.py:229-230
            return self._results(self._search("full_text", text_query, top_k, self._mask(filter)))
        if not _is_given(dense_query) and not _is_given(sparse_query):
            return self._filter_only_query(filter, top_k)
        mask = self._mask(filter)
        nprobe = self._nprobe_of(search_params)
        if search_type == "dense" and _is_given(dense_query):
            hits = self._search("dense", dense_query, top_k, mask, nprobe)
        elif search_type == "sparse" and _is_given(sparse_query):
            hits = self._search("sparse", sparse_query, top_k, mask)
        elif search_type == "hybrid" and _is_given(dense_query) and _is_given(sparse_query):
            try:
                rbm = {"dense": self._search("dense", dense_query, top_k * 2, mask, nprobe),
                       "sparse": self._search("sparse", sparse_query, top_k * 2, mask)}
                hits = merge_hybrid_results(rbm, top_k, {"dense": 0.5, "sparse": 0.5}, rrf_k=rrf_k)
            except Exception as e:  # milvus_base.py:296-306
                if self._world > 1:
                    raise
                logger.warning("Hybrid search failed: %s, falling back to dense search", e)
                hits = self._search("dense", dense_query, top_k, mask, nprobe)
        else:
            raise ValueError(f"Invalid search configuration: type={search_type}, "
                             f"dense={dense_query is not None}, sparse={sparse_query is not None}")
        return self._results(hits)

    # -------------------------------------------------------------- grouping search
    def _check_grouped_call(self, search_type: str, hybrid_weights, top_k: int, dense_given: bool, filter_only: bool) -> None:
        """The refusals of a grouped `query` / `query_batch`: everything but a dense query on a single-GPU FLAT store of fp32 or
        bf16 rows."""
        supported = ("grouping search (group_by_field) is supported for search_type='dense' on a single-GPU store with "
                     "index_type='FLAT' and dense_dtype 'f32' or 'bf16'")
        if hybrid_weights is not None:
            raise ValueError(f"{supported}: not with hybrid_weights")
        if filter_only:
            raise ValueError(f"{supported}: a filter-only call (no query vector) cannot be grouped")
        if search_type != "dense":
            raise ValueError(f"{supported}: not with search_type={search_type!r}")
        if not dense_given:
            raise ValueError(f"{supported}: it needs a dense query")
        if not self.enable_dense:
            raise ValueError(f"{supported}: this store has no dense field")
        if self._comm is not None:
            raise ValueError(f"{supported}: not on a sharded store (distributed=True or a comm)")
        if self._has_lists:
            raise ValueError(f"{supported}: not with index_type={self.index_type!r}")
        if self.dense_dtype == "int8":
            raise ValueError(f"{supported}: not with dense_dtype='int8'")
        if self.index_type == "PQ":
            raise ValueError(f"{supported}: not with index_type='PQ'")
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= top_k <= GROUP_TOP_K_MAX:
            raise ValueError(f"a grouping search returns 1 <= top_k <= {GROUP_TOP_K_MAX} groups (got {top_k!r})")

    def _grouped_batch(self, queries: Sequence[Any], top_k: int, filter: Optional[str], grouping: Grouping,
                       _retry: int = 0) -> List[List[SearchResult]]:
        """Grouping search for a batch of dense queries: per query the best `top_k` groups of `metadata[grouping.key]` among the
        rows that pass `filter` (deletes excluded), each with its best `grouping.group_size` rows, flattened group by group.
        One `DenseShard.search_grouped` call on the resident shard, whatever `filter_route` is: the mask travels as a bitmap."""
        mask = self._mask(filter)
        with self._mu:
            self._flush()
            shard, n = self._dense, len(self._ids)
            column = self._metadata.group_column(grouping.key, self._meta, n) if shard is not None and n else None
        Q, g = len(queries), grouping.group_size
        mask = self._fit_mask(mask, n)
        if column is None or Q == 0 or (mask is not None and not mask.any()):
            return [[] for _ in range(Q)]
        allow = () if mask is None else (_bitmap(mask), n)
        scores, local, _groups = shard.search_grouped(self._unit_queries(queries), top_k, g, column, *allow)
        rows_of = self._main_rows       # read AFTER the kernel returned: every row the kernel can have seen is in it (`_flush`)
        found = (local >= 0) & (local < len(rows_of))
        rows = np.where(found, rows_of[np.where(found, local, 0)], -1) if len(rows_of) else np.full_like(local, -1)
        if (rows >= n).any():           # rows inserted while this search ran took slots: search again
            if _retry < 3:
                return self._grouped_batch(queries, top_k, filter, grouping, _retry + 1)
            rows = np.where(rows < n, rows, -1)
        return self._results_batch(rows.reshape(Q, top_k * g), scores.reshape(Q, top_k * g))

    def _filter_only_query(self, filter: Optional[str], limit: int) -> List[SearchResult]:
        mask = self._mask(filter)
        rows = (np.arange(min(limit, len(self._ids))) if mask is None else np.nonzero(mask)[0][:limit]).astype(np.int64)
        return self._results_batch(rows[None, :], np.ones((1, len(rows))))[0]

    def _hybrid_search_with_weights(self, dense_query, sparse_query, text_query, top_k, filter, hybrid_weights, rrf_k,
                                    nprobe: Optional[int] = None):
        """milvus_base.py:366-459."""
        hybrid_weights = sanitize_hybrid_weights(hybrid_weights)
        if "full_text" in hybrid_weights and not self.enable_full_text:
            logger.warning("full_text not available on %s, removing from hybrid_weights", self.__class__.__name__)
            hybrid_weights = {k: v for k, v in hybrid_weights.items() if k != "full_text"}
        if not hybrid_weights:
            raise ValueError("No valid search methods in hybrid_weights")
        mask = self._mask(filter)
        rbm: Dict[str, List[dict]] = {}
        if "dense" in hybrid_weights and dense_query is not None:
            rbm["dense"] = self._search("dense", dense_query, top_k * 2, mask, nprobe)
        if "sparse" in hybrid_weights and sparse_query is not None:
            rbm["sparse"] = self._search("sparse", sparse_query, top_k * 2, mask)
        if "full_text" in hybrid_weights and text_query is not None:           # milvus_base.py:420-431
            try:
                rbm["full_text"] = self._search("full_text", text_query, top_k * 2, mask)
            except Exception as e:
                if self._world > 1:
                    raise
                logger.warning("Full text search failed: %s, excluding from hybrid", e)
        if len(rbm) == 0:
            logger.warning("Hybrid search: no valid methods executed after validation")
            return []
        if len(rbm) == 1:
            return self._results(list(rbm.values())[0][:top_k])
        return self._results(merge_hybrid_results(rbm, top_k, hybrid_weights, rrf_k))

    def add_documents(self, documents: List[Dict[str, Any]]):
        """Document records beside the chunk rows (milvus_base.py:129-165; probed with `hasattr` by
        VerbatimIndex._store_document_metadata, index.py:299-316): id, title, source, content_type, raw_content,
        metadata, plus the promoted filter fields when the metadata carries them."""
        with self._mu:
            for doc in documents or []:
                metadata = doc.get("metadata", {})
                row = {"id": doc.get("id", ""), "title": doc.get("title") or "", "source": doc.get("source") or "",
                       "content_type": json_serialize_safe(doc.get("doc_type") or doc.get("content_type") or ""),
                       "raw_content": doc.get("raw_content", ""),
                       "metadata": json_serialize_safe(metadata) if isinstance(metadata, dict) else metadata}
                if isinstance(metadata, dict):
                    for key in ("user_id", "dataset_id", "document_id"):
                        if key in metadata:
                            row[key] = metadata.get(key)
                self._documents[row["id"]] = row

    def get_document(self, document_id: str) -> Optional[Dict[str, Any]]:
        """milvus_base.py:173-187: the stored record (a copy) or None."""
        with self._mu:
            row = self._documents.get(document_id)
            return dict(row) if row is not None else None

    # -------------------------------------------------------------- persistence
    FORMAT = 3

    def save(self, path: str) -> None:
        """Writes the store to a directory (deleted rows are dropped): `store.json` (geometry, document records) and the
        id column by rank 0; per rank `vectors.rank{r}.npz` (its packed unit dense rows, sparse CSR and the row numbers
        they belong to) and the text / enhanced-text / metadata columns of those rows (string columns as NUL-joined text,
        `_put_strings`; metadata as one JSON array).  Every file is written beside its final name and renamed into
        place, and a sharded `save` ends in a barrier, so a `load` that follows on any rank reads complete files.  The reference persists through the Milvus-lite database file
        (milvus_local.py:39-56); this is the GPU store's own on-disk format.  Sharded stores: every rank calls `save`
        with the same path."""
        import os

        os.makedirs(path, exist_ok=True)
        with self._mu:
            alive = self._alive.data.copy()
            owned = self._owned.data
            new_row = np.cumsum(alive) - 1                                   # row number after dropping the deleted rows
            local = np.nonzero(alive[owned])[0] if len(owned) else np.zeros(0, np.int64)
            arrays: Dict[str, np.ndarray] = {"owned": new_row[owned[local]].astype(np.int64)}
            if self.enable_dense:
                arrays["dense"] = np.ascontiguousarray(self._dense_rows.data[local], dtype=np.float32)
            if self.enable_sparse:
                indptr, indices, values = csr_take_rows(self._sp_ptr.data, self._sp_idx.data, self._sp_val.data, local)
                arrays.update(sp_indptr=indptr, sp_indices=indices, sp_values=values)
            # texts / metadata lists are indexed by local row, or by global row when a sharded store replicates them
            slots = local if (self._payload_sharded or self._world == 1) else owned[local]
            whole = len(slots) == len(self._texts) and (len(slots) == 0 or (slots[0] == 0 and slots[-1] == len(slots) - 1))
            pick = (lambda col: col) if whole else (lambda col: _take(col, slots))
            texts, enh, metas = pick(self._texts), pick(self._enh), pick(self._meta)
            ids = self._ids if alive.all() else _take(self._ids, np.nonzero(alive)[0])
            if not any(metas):
                metas = {"empty_rows": len(metas)}                             # nothing to store per row
            head = {"format": self.FORMAT, "world": self._world, "dense_dim": self.dense_dim, "sparse_vocab": self.sparse_vocab,
                    "enable_dense": self.enable_dense, "enable_sparse": self.enable_sparse, "dense_dtype": self.dense_dtype,
                    "dense_prefilter": self.dense_prefilter, "enable_full_text": self.enable_full_text, "bm25_k1": self.bm25_k1,
                    "bm25_b": self.bm25_b, "rows": len(ids), "documents": list(self._documents.values())}
            if self.index_type != "FLAT":      # a FLAT store's manifest stays byte for byte what it was
                head.update(index_type=self.index_type, nlist=self.nlist, nprobe=self.nprobe)
            if self.index_type == "PQ":
                head.update(m=self.m, nbits=self.nbits)
                put_pq_codebooks(arrays, self._pq_codebooks, self._pq_trained_rows)
            r = self._rank

            def put_arrays(tmp):
                with open(tmp, "wb") as f:
                    np.savez(f, **arrays)

            _replace_into(path, f"vectors.rank{r}.npz", put_arrays)
            _put_strings(path, f"texts.rank{r}", texts)
            _put_strings(path, f"enhanced.rank{r}", enh)
            _replace_into(path, f"metadatas.rank{r}.json", lambda tmp: _write_text(tmp, json.dumps(metas, ensure_ascii=False)))
            if r == 0:
                _put_strings(path, "ids", ids)
                _replace_into(path, "store.json", lambda tmp: _write_text(tmp, json.dumps(head, ensure_ascii=False)))
        if self._world > 1:
            self._comm.barrier()

    @staticmethod
    def _read_saved(path: str):
        return read_saved(path)

    @classmethod
    def load(cls, path: str, device: int = 0, distributed: bool = False, group=None, comm=None,
             payload: str = "sharded", filter_route: str = "subset", rrf_route: str = "host",
             filter_eval: str = "host", filter_strings: str = "host", auto_compact: Optional[float] = None) -> "GpuVectorStore":
        """Reads a directory written by `save` -- by this or an earlier revision (formats 1 - 3), by any number of
        ranks: when the world size differs from the writer's, the saved shards are put back in row order and cut
        contiguously over the ranks that open the store.  `filter_route`, `rrf_route`, `filter_eval`, `filter_strings`, `auto_compact`: as the constructor's (not part of a saved store).
        An IVF_FLAT / IVF_SQ8 store comes back as what it was with its `nlist` / `nprobe`; its lists are trained again at the first flush
        (training is deterministic: the same rows give the same lists)."""
        head, ids, shards = cls._read_saved(path)
        st = cls(dense_dim=head["dense_dim"], sparse_vocab=head["sparse_vocab"], enable_dense=head["enable_dense"],
                 enable_sparse=head["enable_sparse"], dense_dtype=head["dense_dtype"], device=device,
                 distributed=distributed, group=group, comm=comm, payload=payload,
                 dense_prefilter=head.get("dense_prefilter", "auto"), enable_full_text=bool(head.get("enable_full_text", False)),
                 bm25_k1=head.get("bm25_k1", 1.2), bm25_b=head.get("bm25_b", 0.75), filter_route=filter_route,
                 rrf_route=rrf_route, index_type=head.get("index_type", "FLAT"), nlist=head.get("nlist", 8192),
                 nprobe=head.get("nprobe", 16), filter_eval=filter_eval, filter_strings=filter_strings, auto_compact=auto_compact,
                 m=head.get("m"), nbits=head.get("nbits", 8))
        if st.index_type == "PQ":                                 # trained codebooks come back as they were: never retrained
            st._pq_codebooks, st._pq_trained_rows = get_pq_codebooks(shards[0][1] if shards else {}, st.m, st.dense_dim)
        n = len(ids)
        for owned, *_ in shards:
            if len(owned) and (owned.min() < 0 or owned.max() >= n):
                raise ValueError(f"{path}: shard rows outside the {n} stored ids")
        if len(shards) == st._world:
            owned, z, texts, enh, metas = shards[st._rank]
            owned = np.asarray(owned, dtype=np.int64)
            dense = z["dense"] if st.enable_dense else None
            csr = (z["sp_indptr"], z["sp_indices"], z["sp_values"]) if st.enable_sparse else None
        else:                                                     # re-shard: everything back in row order, my contiguous cut
            from .distributed import shard_range

            all_owned = np.concatenate([np.asarray(o, dtype=np.int64) for o, *_ in shards]) if shards else np.zeros(0, np.int64)
            order = np.argsort(all_owned, kind="stable")
            lo, hi = shard_range(n, st._rank, st._world)
            pick = order[lo:hi]                                   # positions in the concatenation of the saved shards
            owned = all_owned[pick]
            texts_all = [t for _o, _z, tx, _e, _m in shards for t in tx]
            enh_all = [t for _o, _z, _tx, e, _m in shards for t in e]
            meta_all = [t for _o, _z, _tx, _e, m in shards for t in m]
            texts, enh, metas = [texts_all[i] for i in pick], [enh_all[i] for i in pick], [meta_all[i] for i in pick]
            dense = np.concatenate([z["dense"] for _o, z, *_ in shards])[pick] if st.enable_dense else None
            csr = None
            if st.enable_sparse:
                ptrs, idxs, vals, off = [np.zeros(1, np.int64)], [], [], 0
                for _o, z, *_ in shards:
                    ptrs.append(z["sp_indptr"][1:].astype(np.int64) + off)
                    idxs.append(z["sp_indices"])
                    vals.append(z["sp_values"])
                    off += int(z["sp_indptr"][-1])
                csr = csr_take_rows(np.concatenate(ptrs), np.concatenate(idxs), np.concatenate(vals), pick)
        m = len(owned)
        covered = np.concatenate([np.asarray(o, dtype=np.int64) for o, *_ in shards]) if shards else np.zeros(0, np.int64)
        if len(covered) != n or len(np.unique(covered)) != n:
            raise ValueError(f"{path}: the saved shards do not cover the {n} stored ids exactly once")
        st._ids = list(ids)
        st._all_ids_truthy = all(bool(x) for x in st._ids)
        st._note_unique(st._ids)
        st._documents = {d.get("id", ""): dict(d) for d in head.get("documents", [])}
        st._alive.extend(np.ones(n, dtype=bool))
        st._owned.extend(owned)
        if st._payload_sharded or st._world == 1:
            st._texts, st._enh, st._meta = list(texts), list(enh), list(metas)
        else:                                                     # replicated payload: every rank needs every row's
            st._texts, st._enh, st._meta = [""] * n, [""] * n, [{} for _ in range(n)]
            for o, _z, tx, e, mm in shards:
                for g, t1, t2, t3 in zip(np.asarray(o).tolist(), tx, e, mm):
                    st._texts[g], st._enh[g], st._meta[g] = t1, t2, dict(t3)
        if st.enable_dense:
            if dense.shape[0] != m:
                raise ValueError(f"{path}: {dense.shape[0]} dense rows for {m} shard rows")
            st._dense_rows.extend(np.asarray(dense, dtype=np.float32))
        if st.enable_sparse:
            ip, ix, vv = csr
            if len(ip) != m + 1:
                raise ValueError(f"{path}: sparse indptr has {len(ip)} entries for {m} shard rows")
            st._sp_ptr.extend(np.asarray(ip[1:], dtype=np.int64))
            st._sp_idx.extend(np.asarray(ix, dtype=np.int32))
            st._sp_val.extend(np.asarray(vv, dtype=np.float32))
        st._dirty = n > 0
        return st


def _is_given(q) -> bool:
    """Truthiness of a query vector the way the reference tests it (`if dense_query`, milvus_base.py:232-254), for
    lists, dicts and numpy rows alike."""
    return q is not None and len(q) > 0
