"""Model-based test of `GpuVectorStore`: a brute-force model of the whole store, a seeded generator of interleaved operations
(insert, delete, query, query_batch, save + load) and the exact comparison of every answer.  No test functions here: the CPU
run (tests/test_store_model_host.py, over the stand-in shards) and the GPU run (tests/test_store_model_gpu.py) share it.

The model is a plain list of rows.  Every query is answered from nothing over the rows that are alive and pass the filter --
`oracle.topk_ref` for the dense and the sparse leg, `sq8_ref` for int8 rows, a fresh `Bm25Oracle` for full text, and a float64
restatement of weighted RRF BY ID for the hybrid forms -- and nothing is kept between operations.  Filters are a fixed table
of (expression, Python predicate) pairs: the model never parses a filter string.

The data makes every comparison exact (`==` on ids and on score bits, no tolerance anywhere):
  * dense rows and queries have 48 entries of +-1/8 and 4 of +-2/8: squared sum exactly 1, every entry exact in bf16, every dot
    product a multiple of 1/64 that is exact in any summation order -- so the store's normalisation is the identity, every
    kernel gives the same score, and equal scores are frequent: the tie order is what is tested (`check_unit` asserts the
    property on every generated row);
  * sparse weights are k/64 in the document's own (unsorted) term order, some documents are empty;
  * texts are drawn Zipf-like from a small vocabulary, some are empty, every other one ends in a term all of them hold.
"""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np

import verbatim_rag_amd  # noqa: F401
from oracle import topk_ref as T
from verbatim_rag_amd import vector_stores as vs

import full_text_oracle as FT
import sq8_ref
from sharded_store_cases import CpuDense, CpuSparse

METHODS = ("dense", "sparse", "full_text")
VOCAB = 200
NONZERO = 52          # 48 entries of 1/8 and 4 of 2/8: 48/64 + 4 * 4/64 = 1


# ------------------------------------------------------------------------------------------------ configurations
@dataclass(frozen=True)
class Config:
    name: str
    dim: int = 64
    dense: bool = True
    sparse: bool = True
    text: bool = False
    dtype: str = "f32"
    prefilter: Any = "auto"
    routes: Tuple[Tuple[str, str], ...] = ()          # run-time options, passed to the constructor and to `load` again
    host_routes: Optional[Tuple[Tuple[str, str], ...]] = None   # what the stand-ins can run of them (None = the same)
    ivf: bool = False
    start: int = 300
    headroom: float = 1.1
    tail_min: int = 64
    falsy: bool = False
    host: bool = True                                 # the stand-ins can run it
    size_p: Tuple[float, ...] = (0.15, 0.2, 0.35, 0.3)   # weights of the insert sizes 1, 7, 64, 300
    route: str = ""                                   # the search route the configuration is meant to take
    q_p: Tuple[float, ...] = (1, 1, 1, 1, 1, 1, 1)    # weights of the batch sizes 1, 2, 3, 5, 17, 33, 70
    reuse_from: int = 0                               # first operation whose insert may repeat an id


_BITMAP_DEVICE = (("filter_route", "bitmap"), ("rrf_route", "device"), ("filter_eval", "device"), ("filter_strings", "device"))
_LARGE = dict(start=4200, tail_min=256, size_p=(0.05, 0.1, 0.25, 0.6))
CONFIGS: Dict[str, Config] = {c.name: c for c in (
    Config("f32_subset", route="fp32 pass kernels (under the prefilter image's 4 096-row floor); subset shards; host filter evaluation"),
    Config("f32_noprefilter_dim72", dim=72, prefilter=False, route="fp32 scan at a dim that is no multiple of 64; subset shards"),
    # ids stay unique for the first half, so that batches of 70 reach the device fusion (rows that share an id fuse per query)
    Config("f32_bitmap_device_large", routes=_BITMAP_DEVICE, host_routes=(("filter_route", "bitmap"),), **_LARGE,
           q_p=(1, 1, 1, 1, 1, 1, 4), reuse_from=30,
           route="prefilter image for k <= 16 (batches ranked by the tiled search), fp32 pass kernels above; filtered kernels; device filters, strings and RRF"),
    Config("bf16_subset_large", dtype="bf16", host=False, **_LARGE, route="bf16 tiled search / pass kernels; subset shards"),
    Config("bf16_bitmap", dtype="bf16", routes=(("filter_route", "bitmap"),), route="bf16 pass kernels; filtered kernels over main + tail"),
    Config("int8_subset", dtype="int8", host=False, route="SQ8 scan; subset shards of SQ8 rows"),
    Config("int8_bitmap_large", dtype="int8", host=False, routes=(("filter_route", "bitmap"),), **_LARGE,
           route="SQ8 tile kernel; filtered SQ8 search"),
    Config("f32_ivf_large", ivf=True, host=False, **_LARGE, route="IVF_FLAT overlay, nlist 16; nprobe 16 = every list"),
    Config("three_way", text=True, tail_min=48, route="dense + sparse + full text, main + tail segments of each"),
    Config("text_only", dense=False, sparse=False, text=True, tail_min=48, route="full text alone"),
    Config("falsy_id", text=True, falsy=True, tail_min=48, route="per-query fusion of _hybrid_batch (an empty id)"),
)}
HOST_CONFIGS = [c.name for c in CONFIGS.values() if c.host]
N_OPS = 60

# transitions a configuration's sequences must pass through between them (`check_coverage`)
COVER_ALL = ("query_after_load", "limit_over_64", "shared_id_delete")
COVER_VECTOR = ("dense_append", "dense_rebuild", "sparse_tail", "sparse_fold", "second_pass_alone", "wide_short_and_not",
                "shared_id_fusion")
COVER_TEXT = ("text_tail", "text_fold")


def coverage_wanted(cfg: Config, host: bool) -> Tuple[str, ...]:
    want = list(COVER_ALL)
    if cfg.dense and cfg.sparse:
        want += COVER_VECTOR
        routes = dict(_routes(cfg, host))
        # subset route: more than SUBSET_CACHE masks between two changes; bitmap route: the filtered search of a tail segment
        # whose first row is no multiple of 32 (its bitmap is packed again from that row)
        want.append("subset_eviction" if routes.get("filter_route", "subset") == "subset" else "filtered_unaligned_tail")
        if routes.get("rrf_route") == "device":
            want.append("rrf_device_batch")
    if cfg.falsy:
        want.append("falsy_id_fusion")
    if cfg.text:
        want += COVER_TEXT
    if cfg.ivf:
        want.append("ivf_retrained")
    return tuple(want)


def _routes(cfg: Config, host: bool):
    return cfg.host_routes if host and cfg.host_routes is not None else cfg.routes


# ------------------------------------------------------------------------------------------------ filters
def _has(md, key, kind):
    return isinstance(md.get(key), kind) and not isinstance(md.get(key), bool)


FILTERS: List[Tuple[Optional[str], Callable[[dict], bool], float]] = [
    (None, lambda md: True, 4),
    ('metadata["document_id"] == "d3"', lambda md: md.get("document_id") == "d3", 3),                    # value index, < 1/8
    ('metadata["document_id"] in ["d1", "d4", "d7"]', lambda md: md.get("document_id") in ("d1", "d4", "d7"), 2),
    ('metadata["m"] >= 20 and metadata["m"] < 60', lambda md: _has(md, "m", int) and 20 <= md["m"] < 60, 3),   # wide
    ('metadata["document_id"] != "d0"', lambda md: md.get("document_id") != "d0", 4),
    ('metadata["tag"] LIKE "al%"', lambda md: _has(md, "tag", str) and md["tag"].startswith("al"), 2),
    ('metadata["tag"] not in ["alpha", "beta"]', lambda md: md.get("tag") not in ("alpha", "beta"), 2),
    ('metadata["opt"] >= 3', lambda md: _has(md, "opt", int) and md["opt"] >= 3, 2),                       # half the rows lack it
    ('metadata["document_id"] == "nobody"', lambda md: False, 1),                                          # passes 0 rows
    ('metadata["n"] < 4', lambda md: _has(md, "n", int) and md["n"] < 4, 1),                               # fewer than top_k rows
]
TAGS = ("alpha", "alto", "beta", "gamma", "gal", "delta", "ünï")


def metadata_of(serial: int) -> dict:
    md = {"document_id": f"d{serial % 11}", "n": serial, "m": serial % 100}
    if serial % 8 != 5:
        md["tag"] = TAGS[serial % len(TAGS)]
    if serial % 2 == 0:
        md["opt"] = serial % 7
    return md


# ------------------------------------------------------------------------------------------------ data
def check_unit(rows: np.ndarray) -> None:
    """The property every exact comparison rests on: entries in {0, +-1/8, +-2/8}, squared sum exactly 1 in fp32, bf16-exact."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32
    assert np.isin(np.abs(rows), np.asarray([0, 0.125, 0.25], np.float32)).all()
    assert ((rows * rows).sum(axis=1, dtype=np.float32) == np.float32(1.0)).all()
    assert (T.bf16_round(rows) == rows).all()


def unit_rows(rng: np.random.Generator, n: int, dim: int) -> np.ndarray:
    at = rng.permuted(np.tile(np.arange(dim), (n, 1)), axis=1)[:, :NONZERO]
    mag = np.where(np.arange(NONZERO) < 48, 0.125, 0.25).astype(np.float32)
    val = mag[None, :] * rng.choice(np.asarray([-1.0, 1.0], np.float32), size=(n, NONZERO))
    rows = np.zeros((n, dim), np.float32)
    np.put_along_axis(rows, at, val.astype(np.float32), axis=1)
    check_unit(rows)
    return rows


_TERM_P = 1.0 / (np.arange(VOCAB) + 6.0)
_TERM_P /= _TERM_P.sum()


def sparse_row(rng: np.random.Generator, n_terms: int) -> Dict[int, float]:
    terms = rng.choice(VOCAB, size=n_terms, replace=False, p=_TERM_P)          # the document's own order: not ascending
    return {int(t): float(w) / 64 for t, w in zip(terms, rng.integers(1, 64, n_terms))}


_ALPHA = "abcdefghijklmnopqrstuvwxyzéüßø"


def _words() -> List[str]:
    rng = np.random.default_rng(77)
    words: List[str] = []
    while len(words) < 40:
        w = "".join(_ALPHA[int(i)] for i in rng.integers(0, len(_ALPHA), int(rng.integers(2, 8))))
        if w not in words and w != "common":
            words.append(w)
    return words


WORDS = _words()
_WORD_P = 1.0 / (np.arange(len(WORDS)) + 1.0) ** 1.1
_WORD_P /= _WORD_P.sum()
_SEPS = (" ", ", ", ". ", "\n", " - ")
_KEY_OF: Dict[str, int] = {}


def _key(word: str) -> int:
    """Term key of one word form (the analyzer lowercases, so the forms of a word share it)."""
    if word not in _KEY_OF:
        keys = FT.term_keys(word)
        assert len(keys) == 1, word
        _KEY_OF[word] = keys[0]
    return _KEY_OF[word]


def text_row(rng: np.random.Generator, allow_empty: bool = True) -> Tuple[str, List[int]]:
    """(text, its term keys).  One row in 16 is empty; every other row ends in "common"."""
    if allow_empty and rng.integers(0, 16) == 0:
        return "", []
    picks = rng.choice(len(WORDS), size=int(rng.integers(1, 10)), p=_WORD_P)
    forms = [(WORDS[i], WORDS[i].capitalize(), WORDS[i].upper())[int(rng.integers(0, 3))] for i in picks] + ["common"]
    seps = [_SEPS[int(j)] for j in rng.integers(0, len(_SEPS), len(forms))]
    return "".join(f + s for f, s in zip(forms, seps)), [_key(f) for f in forms]


def text_query(rng: np.random.Generator) -> Tuple[str, List[int]]:
    picks = rng.choice(len(WORDS), size=int(rng.integers(1, 4)), p=_WORD_P)
    forms = [WORDS[i] for i in picks] + (["Common"] if rng.integers(0, 4) == 0 else [])
    return " ".join(forms), [_key(f) for f in forms]


# ------------------------------------------------------------------------------------------------ the model
@dataclass
class Row:
    id: str
    serial: int
    dense: Optional[np.ndarray]
    sparse: Optional[Dict[int, float]]
    text: str
    keys: List[int]
    meta: dict
    alive: bool = True

    @property
    def enh(self) -> str:
        return f"e{self.serial}"


def _csr(dicts: List[Dict[int, float]]):
    """CSR with ascending terms inside a row (the sums are exact, so the order changes no score)."""
    lens = np.asarray([len(d) for d in dicts], np.int64)
    rows = np.repeat(np.arange(len(dicts)), lens)
    idx = np.asarray([t for d in dicts for t in d], np.int32)
    val = np.asarray([w for d in dicts for w in d.values()], np.float32)
    order = np.lexsort((idx, rows))
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), idx[order], val[order]


Hit = Tuple[int, float]        # (row, score)


def _hit_lists(scores: np.ndarray, local: np.ndarray, rows: np.ndarray) -> List[List[Hit]]:
    return [[(int(rows[j]), float(v)) for v, j in zip(s, i) if j >= 0] for s, i in zip(scores, local)]


class Model:
    def __init__(self, cfg: Config):
        self.cfg, self.rows = cfg, []

    # -- state
    def add(self, rows: List[Row]) -> None:
        self.rows.extend(rows)

    def delete(self, ids) -> None:
        gone = set(ids)
        for r in self.rows:
            if r.id in gone:
                r.alive = False

    def compact(self) -> None:
        self.rows = [r for r in self.rows if r.alive]

    def passing(self, flt: int) -> np.ndarray:
        pred = FILTERS[flt][1]
        return np.asarray([i for i, r in enumerate(self.rows) if r.alive and pred(r.meta)], np.int64)

    # -- one method, the queries of one operation: per query [(row, score)] by (score desc, row asc)
    def dense(self, qs: List[np.ndarray], k: int, rows: np.ndarray) -> List[List[Hit]]:
        kk = min(k, len(rows))
        if kk == 0:
            return [[] for _ in qs]
        block = np.stack([self.rows[i].dense for i in rows])
        search = sq8_ref.search if self.cfg.dtype == "int8" else T.dense_topk
        return _hit_lists(*search(block, np.stack(qs), kk), rows)

    def sparse(self, qs: List[Dict[int, float]], k: int, rows: np.ndarray) -> List[List[Hit]]:
        kk = min(k, len(rows))
        if kk == 0:
            return [[] for _ in qs]
        found = T.sparse_topk(*_csr([self.rows[j].sparse for j in rows]), VOCAB, *_csr(qs), kk)
        return _hit_lists(*found, rows)                                              # no shared term: not a hit

    def full_text(self, qs: List[List[int]], k: int, rows: np.ndarray) -> List[List[Hit]]:
        if not self.rows:
            return [[] for _ in qs]
        dl = np.asarray([len(r.keys) for r in self.rows], np.int64)
        flat = np.asarray([x for r in self.rows for x in r.keys], np.uint64)
        oracle = FT.Bm25Oracle.from_arrays(flat, dl)
        oracle.set_live(np.asarray([r.alive for r in self.rows], dtype=bool))       # statistics of the live rows
        allow = np.zeros(len(self.rows), dtype=bool)
        allow[rows] = True
        out = []
        for qkeys in qs:
            got, sc = oracle.search(qkeys, k, allow)
            out.append([(int(r), float(v)) for r, v in zip(got, sc)])
        return out

    def method(self, m: str, qs: list, k: int, rows: np.ndarray) -> List[List[Hit]]:
        return getattr(self, m)(qs, k, rows)

    # -- weighted RRF by id, float64, the reference's sequential accumulation
    def fuse(self, lists: Dict[str, List[Hit]], top_k: int, weights: Dict[str, float], rrf_k: int) -> List[Hit]:
        present = [m for m in METHODS if m in lists]
        total = sum(weights.get(m, 0.0) for m in present)
        share = {m: weights.get(m, 0.0) / total for m in present}
        score: Dict[str, float] = {}
        first: Dict[str, int] = {}
        for m in present:
            for rank, (row, _s) in enumerate(lists[m]):
                key = self.rows[row].id
                if not key:
                    continue                                  # skipped, but it kept its rank
                if key not in score:
                    score[key], first[key] = 0.0, row
                score[key] += share[m] * (1.0 / (rrf_k + rank + 1))
        order = sorted(score, key=lambda key: -score[key])    # stable: ties first seen
        return [(first[key], 1.0 - score[key]) for key in order[:top_k]]

    # -- the queries of one operation (they share mode, top_k, filter and weights)
    def answer(self, mode: str, qs: List[dict], top_k: int, flt: int, weights: Optional[Dict[str, float]],
               rrf_k: int) -> List[List[Hit]]:
        rows = self.passing(flt)
        if mode == "filter_only":
            return [[(int(r), 1.0) for r in rows[:top_k]]]
        if mode in METHODS:
            return self.method(mode, [q[mode] for q in qs], top_k, rows)
        if mode == "hybrid":
            weights, use = {"dense": 0.5, "sparse": 0.5}, ("dense", "sparse")
        else:
            weights = {m: float(w) for m, w in weights.items() if m in METHODS and w > 0 and (m != "full_text" or self.cfg.text)}
            use = [m for m in METHODS if m in weights and qs[0].get(m) is not None]
        lists = {m: self.method(m, [q[m] for q in qs], 2 * top_k, rows) for m in use}
        if len(lists) == 1:
            return [one[:top_k] for one in next(iter(lists.values()))]
        return [self.fuse({m: lists[m][i] for m in lists}, top_k, weights, rrf_k) for i in range(len(qs))]

    def expected(self, hits: List[Hit]) -> List[tuple]:
        return [(self.rows[r].id, float(s).hex(), self.rows[r].enh) for r, s in hits]


def got_of(results) -> List[tuple]:
    return [(r.id, float(r.score).hex(), r.enhanced_text) for r in results]


# ------------------------------------------------------------------------------------------------ stand-ins (CPU run)
def _allowed(words, n_allow: int, n_rows: int) -> np.ndarray:
    words = np.ascontiguousarray(words, dtype=np.uint32)
    r = np.arange(min(int(n_allow), n_rows), dtype=np.int64)
    return r[((words[r // 32] >> (r % 32).astype(np.uint32)) & 1).astype(bool)] if len(r) else r


def _pad(s, i, k):
    pad = k - s.shape[1]
    return np.pad(s, ((0, 0), (0, pad)), constant_values=-np.inf), np.pad(i, ((0, 0), (0, pad)), constant_values=-1)


class ModelDense(CpuDense):
    def __len__(self):
        return len(self.rows)

    def search_filtered(self, queries, k, allow_words, n_allow, stream=None):
        rows = _allowed(allow_words, n_allow, len(self.rows))
        q = np.asarray(queries, np.float32)
        kk = min(k, len(rows))
        if kk == 0:
            return np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), -1, np.int64)
        s, i = T.dense_topk(self.rows[rows], q, kk)
        return _pad(s, np.where(i >= 0, rows[np.where(i >= 0, i, 0)], -1), k)


class ModelSparse(CpuSparse):
    def __init__(self, vocab, indptr, indices, values, device=0):
        super().__init__(vocab, np.array(indptr), np.array(indices), np.array(values), device)
        self.n_docs = len(indptr) - 1

    def search_filtered(self, queries, k, allow_words, n_allow, stream=None):
        queries = list(queries)
        rows = _allowed(allow_words, n_allow, self.n_docs)
        kk = min(k, len(rows))
        if kk == 0:
            return np.full((len(queries), k), -np.inf, np.float32), np.full((len(queries), k), -1, np.int64)
        s, i = T.sparse_topk(*vs.csr_take_rows(*self.csr, rows), self.vocab, *vs.dicts_to_csr(queries), kk)
        return _pad(s, np.where(i >= 0, rows[np.where(i >= 0, i, 0)], -1), k)


class stand_ins:
    """The store's device layers replaced by exact CPU ones (tests only); `dense` / `sparse` / `text` override a class."""

    def __init__(self, dense=None, sparse=None, text=None):
        from full_text_sharded_cases import CpuTextIndex

        self.classes = (dense or ModelDense, sparse or ModelSparse, text or CpuTextIndex)

    def __enter__(self):
        from verbatim_rag_amd.distributed import merge_topk

        self.saved = (vs._lib.load, vs._lib.require_gpu, vs.DenseShard, vs.SparseShard, vs.TextIndex, vs._merge_parts)
        vs._lib.load, vs._lib.require_gpu = (lambda: None), (lambda: None)
        vs.DenseShard, vs.SparseShard, vs.TextIndex = self.classes
        vs._merge_parts = lambda scores, rows, k, device: merge_topk(scores, rows, k)
        return self

    def __exit__(self, *exc):
        vs._lib.load, vs._lib.require_gpu, vs.DenseShard, vs.SparseShard, vs.TextIndex, vs._merge_parts = self.saved


# ------------------------------------------------------------------------------------------------ the runner
class Mismatch(AssertionError):
    pass


class StoreFault(RuntimeError):
    """A store call failed inside the library (or a search leg was dropped after such a failure): not a wrong answer."""


class _Warnings(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.failed: List[str] = []

    def emit(self, record):
        msg = record.getMessage()
        if "failed" in msg:
            self.failed.append(msg)


@dataclass
class Coverage:
    seen: Dict[str, int] = field(default_factory=dict)
    queries: int = 0
    empty: int = 0
    rows_max: int = 0

    def hit(self, name: str) -> None:
        self.seen[name] = self.seen.get(name, 0) + 1

    def merge(self, other: "Coverage") -> None:
        for k, v in other.seen.items():
            self.seen[k] = self.seen.get(k, 0) + v
        self.rows_max = max(self.rows_max, other.rows_max)


def check_coverage(cfg: Config, total: Coverage, host: bool) -> None:
    missing = [name for name in coverage_wanted(cfg, host) if not total.seen.get(name)]
    assert not missing, f"{cfg.name}: the sequences never passed through {missing} (seen: {total.seen})"


Q_SIZES = (1, 2, 3, 5, 17, 33, 70)
TOP_KS = (1, 5, 10, 40, 64, 70)
ADD_SIZES = (1, 7, 64, 300)
W2 = {"dense": 0.7, "sparse": 0.3}
W3 = {"dense": 0.5, "sparse": 0.3, "full_text": 0.2}      # on a store without full text: a weight on a method it lacks
W_TEXT = {"full_text": 1.0, "dense": 0.5}                 # on the full-text-only store: one method left


class Runner:
    """One sequence: `Runner(cfg, seed, tmp_dir, host).run()`.  The same (cfg, seed) draws the same operations on the CPU and
    on the GPU: nothing the store returns feeds the generator."""

    def __init__(self, cfg: Config, seed: int, tmp_dir: str, host: bool, n_ops: int = N_OPS, start: Optional[int] = None,
                 race: bool = False, modes: Optional[list] = None):
        """`race=True` adds one more operation: an insert that lands inside a filtered `query`, between the moment the query
        builds its row mask and its search (what an insert from another thread does).  The query must answer as if it had run
        first.  Off in the standard sequences, whose draws it would shift.  `modes`: the (mode, weights, weight) choices of
        the queries instead of the configuration's (the negative controls narrow them to single methods)."""
        self.race = race
        self.cfg, self.seed, self.tmp, self.host, self.n_ops = cfg, seed, str(tmp_dir), host, n_ops
        self.rng = np.random.default_rng([sorted(CONFIGS).index(cfg.name), seed])
        self.model = Model(cfg)
        self.cover = Coverage()
        self.log: List[str] = []
        self.serial = 0
        self.start = cfg.start if start is None else start
        self.store = None
        self.params = {"nprobe": 16} if cfg.ivf else None
        self.modes = modes or self._modes()
        self._prev: Dict[str, Any] = {}
        self._ivf_trained: Optional[int] = None
        self.saves = 0
        self.after_load = False

    def _modes(self) -> List[Tuple[str, Optional[dict], float]]:
        c = self.cfg
        if not c.dense:
            return [("full_text", None, 3), ("weighted", W_TEXT, 2)]
        modes = [("dense", None, 3), ("sparse", None, 2), ("hybrid", None, 3), ("weighted", W2, 2), ("weighted", W3, 2)]
        if c.text:
            modes += [("full_text", None, 2), ("weighted", {"sparse": 0.4, "full_text": 0.6}, 1)]
        return modes

    # -- the store
    def _kwargs(self) -> dict:
        return dict(_routes(self.cfg, self.host))

    def _tune(self, st) -> None:
        st.SPARSE_TAIL_MIN = st.TEXT_TAIL_MIN = self.cfg.tail_min     # on the instance: the folds come within 60 operations
        st.dense_headroom = self.cfg.headroom

    def _new_store(self):
        c = self.cfg
        st = vs.GpuVectorStore(dense_dim=c.dim if c.dense else None, sparse_vocab=VOCAB if c.sparse else None, enable_dense=c.dense,
                               enable_sparse=c.sparse, enable_full_text=c.text, dense_dtype=c.dtype, dense_prefilter=c.prefilter,
                               dense_headroom=c.headroom, index_type="IVF_FLAT" if c.ivf else "FLAT", nlist=16, nprobe=16,
                               **self._kwargs())
        self._tune(st)
        return st

    def _call(self, fn, *a, **kw):
        try:
            return fn(*a, **kw)
        except vs._lib.VragError as e:
            raise StoreFault(f"{self._where()}: {e}") from e

    def _where(self) -> str:
        return f"config {self.cfg.name!r} seed {self.seed} op {len(self.log) - 1}: {self.log[-1] if self.log else ''}"

    def _fail(self, what: str, got, want) -> None:
        at = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
        err = Mismatch(f"{self._where()}\n  {what}: {len(got)} hits for {len(want)} expected, first difference at rank {at}\n"
                       f"  got      {got[at:at + 3]}\n  expected {want[at:at + 3]}\n"
                       f"  replay: Runner(CONFIGS[{self.cfg.name!r}], {self.seed}, tmp_dir, host={self.host}).run()\n  ops: "
                       + " | ".join(self.log))
        err.runner, err.op, err.got, err.want, err.at = self, self.log[-1], got, want, at      # for the negative controls
        raise err

    # -- operations
    def _fresh_rows(self, n: int, reuse: bool) -> List[Row]:
        c, rng = self.cfg, self.rng
        dense = unit_rows(rng, n, c.dim) if c.dense else None
        rows = []
        known = [r.id for r in self.model.rows]
        for j in range(n):
            serial = self.serial
            self.serial += 1
            key = f"id{serial}"
            if reuse and known and rng.integers(0, 5) == 0:
                key = known[int(rng.integers(0, len(known)))]           # a live or a dead row's id
            elif c.falsy and rng.integers(0, 12) == 0:
                key = ""
            text, keys = text_row(rng) if c.text else (f"text {serial}", [])
            rows.append(Row(key, serial, dense[j] if c.dense else None,
                            sparse_row(rng, int(rng.integers(0, 10)) if rng.integers(0, 12) else 0) if c.sparse else None,
                            text, keys, metadata_of(serial)))
        return rows

    def _add(self, n: int, reuse: bool, bulk: bool) -> None:
        rows = self._fresh_rows(n, reuse)
        c = self.cfg
        dense = sparse = None
        if c.dense:
            dense = np.stack([r.dense for r in rows]) if bulk else [r.dense.tolist() for r in rows]
        if c.sparse:
            sparse = [r.sparse for r in rows]
            if bulk:                                                    # CSR with the documents' own term order
                indptr = np.concatenate([[0], np.cumsum([len(d) for d in sparse])]).astype(np.int64)
                sparse = (indptr, np.asarray([t for d in sparse for t in d], np.int64),
                          np.asarray([w for d in sparse for w in d.values()], np.float32))
        self._call(self.store.add_vectors, [r.id for r in rows], dense, sparse, [r.text for r in rows], [r.enh for r in rows],
                   [dict(r.meta) for r in rows])
        self.model.add(rows)
        self._changed()

    def _changed(self) -> None:
        self._prev.pop("subsets", None)

    def _delete(self, n: int) -> None:
        rng, rows = self.rng, self.model.rows
        live = sorted({r.id for r in rows if r.alive})
        dead = sorted({r.id for r in rows if not r.alive})
        counts: Dict[str, int] = {}
        for r in rows:
            if r.alive:
                counts[r.id] = counts.get(r.id, 0) + 1
        shared = sorted(k for k, v in counts.items() if v > 1)
        ids = [live[int(i)] for i in rng.choice(len(live), size=min(n, len(live)), replace=False)] if live else []
        ids.append(f"unknown{len(self.log)}")
        if dead:
            ids.append(dead[int(rng.integers(0, len(dead)))])
        if shared and rng.integers(0, 2):
            ids.append(shared[int(rng.integers(0, len(shared)))])
        if any(k in shared for k in ids):
            self.cover.hit("shared_id_delete")
        self._call(self.store.delete, ids)
        self.model.delete(ids)
        self._changed()

    def _save_load(self) -> None:
        path = os.path.join(self.tmp, f"{self.cfg.name}-{self.seed}-{self.saves}")
        self.saves += 1
        self._call(self.store.save, path)
        self.store.close()
        self.store = self._call(vs.GpuVectorStore.load, path, **self._kwargs())
        self._tune(self.store)
        self.model.compact()
        self._prev = {}
        self.after_load = True

    def _queries(self, n: int) -> List[dict]:
        c, rng, out = self.cfg, self.rng, []
        stored = [r for r in self.model.rows if r.alive]
        fresh = unit_rows(rng, n, c.dim) if c.dense else None
        for j in range(n):
            q: Dict[str, Any] = {"dense": None, "sparse": None, "full_text": None, "text": None}
            if c.dense:
                copy = stored and rng.integers(0, 3) == 0                # a stored row: score exactly 1 for it
                q["dense"] = stored[int(rng.integers(0, len(stored)))].dense if copy else fresh[j]
            if c.sparse:
                q["sparse"] = sparse_row(rng, int(rng.integers(1, 7)))
            if c.text:
                q["text"], q["full_text"] = text_query(rng)
            out.append(q)
        return out

    def _store_kwargs(self, mode, weights, top_k, flt, rrf_k) -> dict:
        kw = dict(top_k=top_k, filter=FILTERS[flt][0], rrf_k=rrf_k)
        if mode == "weighted":
            kw["hybrid_weights"] = dict(weights)
        else:
            kw["search_type"] = mode
        if self.params is not None:
            kw["search_params"] = dict(self.params)
        return kw

    def _single(self, q: dict, kw: dict):
        d = q["dense"]
        return self._call(self.store.query, dense_query=None if d is None else d.tolist(), sparse_query=q["sparse"],
                          text_query=q["text"], **kw)

    def _racing_single(self, q: dict, kw: dict, n: int):
        """`query` with an insert of `n` rows right after it has built its mask (a mask of None has nothing to go stale: the
        insert then follows the query)."""
        st, rows = self.store, self._fresh_rows(n, reuse=False)
        build = st._mask

        def insert():
            self._call(st.add_vectors, [r.id for r in rows], np.stack([r.dense for r in rows]) if self.cfg.dense else None,
                       [r.sparse for r in rows] if self.cfg.sparse else None, [r.text for r in rows], [r.enh for r in rows],
                       [dict(r.meta) for r in rows])

        def mask_then_insert(flt):
            mask = build(flt)
            if mask is not None and "raced" not in self._prev:
                self._prev["raced"] = True
                insert()
                self.cover.hit("racing_add")
            return mask

        st._mask = mask_then_insert
        try:
            got = self._single(q, kw)
        finally:
            del st._mask
        if not self._prev.pop("raced", False):
            insert()
        self.model.add(rows)
        self._changed()
        return got

    def _fused(self, mode: str, weights, q: dict) -> List[str]:
        if mode == "hybrid":
            return ["dense", "sparse"]
        return [m for m in METHODS if m in weights and q.get(m) is not None and (m != "full_text" or self.cfg.text)]

    def _note_routes(self, mode: str, qs: List[dict], top_k: int, flt: int, weights=None) -> None:
        """Coverage that only the model can tell: which pass of `_topk_rows` answers these queries."""
        rows_all = self.model.rows
        n = len(rows_all)
        passing = self.model.passing(flt)
        limit = top_k if mode in METHODS else 2 * top_k
        if limit > 64:
            self.cover.hit("limit_over_64")
        if self.after_load:
            self.cover.hit("query_after_load")
        if mode in ("hybrid", "weighted") and len(self._fused(mode, weights, qs[0])) > 1:
            live = [r.id for r in rows_all if r.alive]
            st = self.store
            if len(set(live)) < len(live):
                self.cover.hit("shared_id_fusion")
            if "" in live and len(qs) > 1:
                self.cover.hit("falsy_id_fusion")
            if st.rrf_route == "device" and len(qs) >= st.RRF_DEVICE_MIN_QUERIES and st._all_ids_truthy and st._ids_unique:
                self.cover.hit("rrf_device_batch")
        legs = [m for m in ("dense", "sparse") if (mode == m or mode in ("hybrid", "weighted")) and qs[0].get(m) is not None]
        if not legs or len(passing) == n or len(passing) == 0:
            return
        if len(passing) * 8 < n:
            self.cover.hit("second_pass_alone")
            self._second_pass = "sparse" in legs
            return
        ok = np.zeros(n, dtype=bool)
        ok[passing] = True
        want = min(limit, len(passing))
        everything = np.arange(n, dtype=np.int64)
        plain = Model(Config("plain", dtype=self.cfg.dtype))
        plain.rows = rows_all
        for m in legs:
            tops = plain.method(m, [q[m] for q in qs], limit, everything)   # what the resident shard (dead rows too) returns
            short = [sum(ok[r] for r, _s in top) < want and len(top) == limit for top in tops]
            if any(short) and not all(short):
                self.cover.hit("wide_short_and_not")

    def _query_op(self, batch: bool) -> None:
        rng = self.rng
        mode, weights, _w = self.modes[int(rng.choice(len(self.modes), p=self._mode_p))]
        n_q = int(rng.choice(Q_SIZES, p=np.asarray(self.cfg.q_p, float) / sum(self.cfg.q_p))) if batch else 1
        top_k = int(rng.choice(TOP_KS))
        flt = int(rng.choice(len(FILTERS), p=self._filter_p))
        rrf_k = (60, 10)[int(rng.integers(0, 2))]
        qs = self._queries(n_q)
        self.log.append(f"{'batch' if batch else 'query'} {mode}{'' if weights is None else sorted(weights)} Q={n_q} k={top_k} f={flt} rrf={rrf_k}")
        self._second_pass = False
        self._note_routes(mode, qs, top_k, flt, weights)
        want = [self.model.expected(hits) for hits in self.model.answer(mode, qs, top_k, flt, weights, rrf_k)]
        self.cover.queries += 1
        self.cover.empty += all(not w for w in want)
        kw = self._store_kwargs(mode, weights, top_k, flt, rrf_k)
        pick = int(rng.integers(0, n_q))
        if batch:
            dq = [q["dense"].tolist() for q in qs] if self.cfg.dense else None
            sq = [q["sparse"] for q in qs] if self.cfg.sparse else None
            tq = [q["text"] for q in qs] if self.cfg.text else None
            got = self._call(self.store.query_batch, dense_queries=dq, sparse_queries=sq, text_queries=tq, **kw)
            if len(got) != n_q:
                self._fail("query_batch length", [len(got)], [n_q])
            for i in range(n_q):
                if got_of(got[i]) != want[i]:
                    self._fail(f"query_batch element {i}", got_of(got[i]), want[i])
        racing = self.race and not batch and mode != "full_text" and "full_text" not in (weights or ()) and rng.integers(0, 2) == 0
        if racing:
            self.log[-1] += " +racing add 7"
            one = got_of(self._racing_single(qs[pick], kw, 7))
        else:
            one = got_of(self._single(qs[pick], kw))
        if one != want[pick]:
            self._fail(f"query (element {pick})", one, want[pick])
        if self.cfg.ivf and mode == "dense":
            self._ivf_sound(qs[pick], top_k, flt)

    def _ivf_sound(self, q: dict, top_k: int, flt: int) -> None:
        """nprobe = 2 finds fewer rows, never wrong ones: live passing rows, the model's score bits, (score desc, row asc)."""
        got = self._call(self.store.query, dense_query=q["dense"].tolist(), top_k=top_k, search_type="dense",
                         filter=FILTERS[flt][0], search_params={"nprobe": 2})
        row_of = {r.enh: i for i, r in enumerate(self.model.rows)}
        passing = set(self.model.passing(flt).tolist())
        seen, last = set(), None
        for hit in got:
            row = row_of[hit.enhanced_text]
            score = np.float32((self.model.rows[row].dense * q["dense"]).sum(dtype=np.float32))       # exact in any order
            key = (-float(hit.score), row)
            if row not in passing or row in seen or float(hit.score).hex() != float(score).hex() or (last is not None and key <= last):
                self._fail("nprobe=2 soundness", got_of(got), [(self.model.rows[row].id, float(score).hex(), hit.enhanced_text)])
            seen.add(row)
            last = key

    def _filter_only(self) -> None:
        top_k = int(self.rng.choice(TOP_KS))
        flt = int(self.rng.choice(len(FILTERS), p=self._filter_p))
        self.log.append(f"filter_only k={top_k} f={flt}")
        want = self.model.expected(self.model.answer("filter_only", [], top_k, flt, None, 60)[0])
        got = got_of(self._call(self.store.query, top_k=top_k, filter=FILTERS[flt][0]))
        if got != want:
            self._fail("filter-only query", got, want)

    # -- store state after a query (the flush has run)
    def _observe(self) -> None:
        st, prev, cov = self.store, self._prev, self.cover
        cov.rows_max = max(cov.rows_max, len(st))
        if self.cfg.dense:
            now = (id(st._dense), st._dense_cap, st._dense_flushed)
            was = prev.get("dense")
            if was is not None and now[2] > was[2]:
                cov.hit("dense_append" if now[:2] == was[:2] else "dense_rebuild")
            prev["dense"] = now
            if self.cfg.ivf:
                stats = st.ivf_stats()
                trained = None if stats is None else stats["trained_rows"]
                if trained is not None and self._ivf_trained is not None and trained != self._ivf_trained:
                    cov.hit("ivf_retrained")
                self._ivf_trained = trained if trained is not None else self._ivf_trained
        if self.cfg.sparse:
            parts = len(st._sparse_parts)
            if parts == 2:
                cov.hit("sparse_tail")
            elif prev.get("sparse_parts") == 2 and parts == 1:
                cov.hit("sparse_fold")
            prev["sparse_parts"] = parts
        if self.cfg.text and st._text is not None and prev.get("text_rows") != st._text_flushed:
            segments = st._text.stats()["segments"]
            if segments == 2:
                cov.hit("text_tail")
            elif prev.get("text_segments") == 2 and segments == 1:
                cov.hit("text_fold")
            prev["text_segments"], prev["text_rows"] = segments, st._text_flushed
        if (getattr(self, "_second_pass", False) and st._filter_route == "bitmap" and len(st._sparse_parts) == 2
                and st._sparse_parts[1][1] % 32):
            cov.hit("filtered_unaligned_tail")
        self._second_pass = False
        keys = set(st._subsets)
        if "subsets" in prev and prev["subsets"] - keys:                  # no insert or delete since: the cache was full
            assert len(keys) == st.SUBSET_CACHE
            cov.hit("subset_eviction")
        prev["subsets"] = keys

    # -- the sequence
    def run(self) -> Coverage:
        watch = _Warnings()
        vs.logger.addHandler(watch)
        try:
            self._run(watch)
        finally:
            vs.logger.removeHandler(watch)
            if self.store is not None:
                self.store.close()
        return self.cover

    def _run(self, watch: _Warnings) -> None:
        rng = self.rng
        self._mode_p = np.asarray([w for _m, _x, w in self.modes], float) / sum(w for _m, _x, w in self.modes)
        self._filter_p = np.asarray([w for _e, _p, w in FILTERS], float) / sum(w for _e, _p, w in FILTERS)
        self.store = self._new_store()
        self.log.append(f"add {self.start}")
        self._add(self.start, reuse=False, bulk=True)
        ops = ("add", "delete", "query", "batch", "save_load", "filter_only")
        op_p = np.asarray([0.30, 0.10, 0.12, 0.40, 0.04, 0.04])
        while len(self.log) < self.n_ops:
            op = ops[int(rng.choice(len(ops), p=op_p))]
            if op == "add":
                n = int(rng.choice(ADD_SIZES, p=self.cfg.size_p))
                reuse, bulk = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
                reuse = reuse and len(self.log) >= self.cfg.reuse_from
                self.log.append(f"add {n}{' reuse' if reuse else ''}{' bulk' if bulk else ''}")
                self._add(n, reuse, bulk)
            elif op == "delete":
                n = int(rng.choice((1, 5, 60), p=(0.4, 0.4, 0.2)))
                self.log.append(f"delete {n}")
                self._delete(n)
            elif op == "save_load":
                self.log.append("save_load")
                self._save_load()
            elif op == "filter_only":
                self._filter_only()
                self._observe()
            else:
                self._query_op(batch=op == "batch")
                self._observe()
            if watch.failed:
                raise StoreFault(f"{self._where()}: {watch.failed[0]}")
        assert self.cover.empty * 4 <= max(self.cover.queries, 1), (self.cfg.name, self.seed, self.cover.empty, self.cover.queries)


def run_config(name: str, seeds, tmp_dir, host: bool) -> Coverage:
    total = Coverage()
    for seed in seeds:
        total.merge(Runner(CONFIGS[name], seed, tmp_dir, host).run())
    return total
