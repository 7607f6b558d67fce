"""Data and float64 references of the IVF tests (tests/test_ivf_unit_gpu.py, tests/test_ivf_host.py): nothing here runs a kernel.

Two kinds of data.
  grid    entries k / 8, k in [-4, 4] (dyadic, bf16-exact): x . c is a multiple of 1/64, 1/2 |c|^2 of 1/128, both below 2^9, so
          every assignment score is exact in fp32 in ANY summation order and ties are frequent; the scan's scores are exact too.
  normal  standard normal rows scaled to unit length.  Scores are then O(1) and a dot product's terms O(1 / dim): an fp32 sum of
          dim such terms is off by about sqrt(dim) * 2^-24 * 0.1 ~ 1e-7 (at most dim * 2^-24 ~ 5e-5 if every rounding went the same
          way), two orders below the 1e-5 gap under which a query's probe set is allowed to differ from the float64 one.
Centroids always include one that attracts no row (`far`), one that attracts exactly one row (`single`) and otherwise rows of the
data, so lists come out empty, of one row and of sizes that are no multiple of 16 (asserted on the CPU by tests/test_ivf_host.py)."""
import functools

import numpy as np

# (dim, n, dtype, nlist, data): a sample of {64, 384, 768} x {257, 3001, 20000} x {0, 1, 2} x {1, 7, 64} x {grid, normal} in which
# every value, every (dtype, data) pair and both extremes of every axis occur
CASES = [
    (64, 257, 0, 1, "grid"),
    (64, 3001, 1, 7, "normal"),
    (384, 257, 2, 7, "grid"),
    (384, 3001, 0, 64, "normal"),
    (768, 3001, 1, 64, "grid"),
    (768, 20000, 2, 64, "normal"),
    (64, 20000, 0, 64, "grid"),
    (384, 20000, 1, 7, "normal"),
    (768, 257, 2, 1, "normal"),
]
NQ_MAX = 100
APPENDED = 40
GAP = 1e-5          # float64 gap between the nprobe-th and the next list score under which a query may be left out
LEFT_OUT_MAX = 0.10


def bf16_round(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def data(kind, dim, n, nlist):
    """(X [n + APPENDED, dim], Q [NQ_MAX, dim], centroids [nlist, dim]); read-only.  Rows [n, n + APPENDED) are appended later and
    lead query 0's ranking.  Query 1 points at the `far` centroid and query 2 at the `single` one (nlist >= 7)."""
    rng = np.random.default_rng(7919 * dim + 31 * n + nlist + (5 if kind == "grid" else 0))
    if kind == "grid":
        X = rng.integers(-4, 5, (n + APPENDED, dim)).astype(np.float32) / np.float32(8)
        Q = rng.integers(-4, 5, (NQ_MAX, dim)).astype(np.float32) / np.float32(8)
        X[n // 2] = X[n // 3]                      # two equal rows: equal scores for every query
    else:
        X = _unit(rng.standard_normal((n + APPENDED, dim)))
        Q = _unit(rng.standard_normal((NQ_MAX, dim)))
    picks = np.sort(rng.choice(n, nlist, replace=False))
    C = X[picks].copy()
    if nlist >= 7:
        lone = int(np.setdiff1d(np.arange(n), np.concatenate([picks, [n // 2, n // 3]]))[n // 5])
        if kind == "grid":
            C[0] = np.float32(0.5)                 # far: 1/2 |c|^2 = dim / 8 outweighs a random row's product with it
            C[1] = X[lone] * np.float32(2)         # single: its row scores 0 there and less than 0 everywhere else, other rows far less
            Q[1] = np.float32(0.5)
            Q[2] = X[lone]
        else:
            far = _unit(rng.standard_normal((1, dim)))[0]
            C[0] = far * np.float32(5)             # x . c <= 5 < 1/2 |c|^2 - 1/2: no row prefers it to a row centroid
            C[1] = X[lone] * np.float32(1.5)
            Q[1] = far * np.float32(10)
            Q[2] = X[lone] * np.float32(10)
    X[n:] = Q[:1] * np.float32(2)
    for a in (X, Q, C):
        a.flags.writeable = False
    return X, Q, C


def stored(X, dtype):
    return bf16_round(X) if dtype == 0 else X


def list_scores64(A, C):
    """float64 assignment scores [len(A), nlist] = a . c - 1/2 |c|^2."""
    C64 = C.astype(np.float64)
    return A.astype(np.float64) @ C64.T - 0.5 * (C64 * C64).sum(axis=1)[None, :]


def assign64(A, C):
    """The rule in float64: argmax, the lowest list on ties (np.argmax returns the first maximum)."""
    return np.argmax(list_scores64(A, C), axis=1)


def probes64(Q, C, nprobe):
    """(probe sets [nq, nprobe] by (score desc, list asc), gap [nq] between the nprobe-th and the next score; inf when all are probed)."""
    S = list_scores64(Q, C)
    order = np.lexsort((np.broadcast_to(np.arange(S.shape[1]), S.shape), -S), axis=1)
    ranked = np.take_along_axis(S, order, axis=1)
    gap = ranked[:, nprobe - 1] - ranked[:, nprobe] if nprobe < S.shape[1] else np.full(len(Q), np.inf)
    return order[:, :nprobe], gap


def lists_of(assign, nlist):
    """(list_off [nlist + 1], list_rows [n]) of a stable counting sort: rows ascending inside a list."""
    rows = np.argsort(assign, kind="stable").astype(np.uint32)
    off = np.zeros(nlist + 1, np.uint32)
    np.cumsum(np.bincount(assign, minlength=nlist), out=off[1:])
    return off, rows


def clusters(dim, n, n_clusters=16, sigma=0.01, seed=3):
    """Well-separated clusters for the training tests: unit-length centres, isotropic noise of `sigma` per coordinate, clusters in
    contiguous blocks of rows.  Lloyd's rounds only ever reach a pure partition from a start with a centroid in every cluster, and
    the start is fixed (evenly strided rows, no RNG), so the blocks are cut where that start needs them: row floor(c * n /
    n_clusters) -- the initial centroid c of n_clusters lists over all rows -- is the FIRST row of cluster c, not the last of c - 1."""
    rng = np.random.default_rng(seed + dim + n)
    centres = _unit(rng.standard_normal((n_clusters, dim)))
    label = (np.arange(n) * n_clusters + n_clusters - 1) // n
    X = (centres[label] + sigma * rng.standard_normal((n, dim))).astype(np.float32)
    return X, label


TRAIN_CASES = [(64, 3001, 1, 16, 1 << 40), (384, 3001, 0, 16, 1 << 40), (768, 3001, 2, 64, 1 << 40), (64, 20000, 1, 64, 64 * 64),
               (384, 257, 0, 64, 100)]          # (dim, n, dtype, nlist, max_train_rows)


def training_rows(n, max_train_rows, nlist):
    """(sample rows, rows of the initial centroids) of vrag_ivf_index_train: sample item i = row i * n / n_train, initial centroid c =
    sample item c * n_train / nlist."""
    n_train = min(n, max_train_rows)
    sample = np.arange(n_train) * n // n_train
    return sample, sample[np.arange(nlist) * n_train // nlist]
