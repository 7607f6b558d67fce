"""Reference of the grouping search for the tests: a FULL ranking of the passing rows by the oracle (sequential fmaf chains, order
(score desc, row asc)), grouped in Python.  No test functions here: the host test's stand-in shard, the raw-ABI GPU test and the
store GPU test share it.  Everything is compared with `==` on ids, group codes and score bits."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from oracle import topk_ref as T


def group_ranked(scores: np.ndarray, rows: np.ndarray, codes: np.ndarray, n_groups: int, group_size: int):
    """One query's full ranking (`rows` best first, -1 = none, with their `scores`) -> (scores `[n_groups, group_size]`,
    rows likewise, codes `[n_groups]`): groups in the order of their best row, each with its first `group_size` rows;
    missing entries -inf / -1 / -1."""
    out_s = np.full((n_groups, group_size), -np.inf, np.float32)
    out_r = np.full((n_groups, group_size), -1, np.int64)
    out_g = np.full(n_groups, -1, np.int32)
    have = rows >= 0
    r, s = np.asarray(rows)[have], np.asarray(scores, np.float32)[have]
    if len(r) == 0:
        return out_s, out_r, out_g
    c = np.asarray(codes)[r]
    distinct, first, inverse = np.unique(c, return_index=True, return_inverse=True)
    group_rank = np.empty(len(distinct), np.int64)
    group_rank[np.argsort(first, kind="stable")] = np.arange(len(distinct))      # groups by the position of their best row
    by_code = np.argsort(c, kind="stable")                                        # ranking order kept inside a group
    starts = np.concatenate([[0], np.nonzero(np.diff(c[by_code]))[0] + 1])
    run = np.cumsum(np.concatenate([[0], np.diff(c[by_code]) != 0]))
    within = np.empty(len(c), np.int64)
    within[by_code] = np.arange(len(c)) - starts[run]                              # a row's rank inside its group
    g = group_rank[inverse.reshape(-1)]
    keep = (g < n_groups) & (within < group_size)
    out_s[g[keep], within[keep]] = s[keep]
    out_r[g[keep], within[keep]] = r[keep]
    shown = group_rank < n_groups
    out_g[group_rank[shown]] = distinct[shown]
    return out_s, out_r, out_g


def rank_passing(rows: np.ndarray, queries: np.ndarray, passing: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The full ranking of the row numbers `passing` (ascending; None = all) per query: `oracle.topk_ref.dense_topk(rows[passing],
    Q, k=n_passing)` with the ids mapped back -> (scores `[Q, n_passing]`, rows `[Q, n_passing]`)."""
    rows = np.ascontiguousarray(rows, np.float32)
    queries = np.ascontiguousarray(queries, np.float32).reshape(-1, rows.shape[1])
    passing = np.arange(len(rows), dtype=np.int64) if passing is None else np.asarray(passing, np.int64)
    if len(passing) == 0:
        return np.empty((len(queries), 0), np.float32), np.empty((len(queries), 0), np.int64)
    s, i = T.dense_topk(rows[passing], queries, len(passing))
    return s, np.where(i >= 0, passing[np.where(i >= 0, i, 0)], -1)


def group_all(scores: np.ndarray, ranked: np.ndarray, codes: np.ndarray, n_groups: int, group_size: int):
    """`group_ranked` for every query of a ranking -> (scores `[Q, n_groups, group_size]`, rows likewise, codes `[Q, n_groups]`)."""
    nq = len(scores)
    out_s = np.full((nq, n_groups, group_size), -np.inf, np.float32)
    out_r = np.full((nq, n_groups, group_size), -1, np.int64)
    out_g = np.full((nq, n_groups), -1, np.int32)
    for q in range(nq):
        out_s[q], out_r[q], out_g[q] = group_ranked(scores[q], ranked[q], codes, n_groups, group_size)
    return out_s, out_r, out_g


def grouped_topk(rows: np.ndarray, queries: np.ndarray, codes: np.ndarray, n_groups: int, group_size: int,
                 passing: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The expected answer of `vrag_dense_index_search_grouped` over `rows` (fp32 as the index holds them: bf16-rounded for a
    bf16 index): the full ranking of the passing rows grouped by `codes[row]`."""
    return group_all(*rank_passing(rows, queries, passing), codes, n_groups, group_size)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
