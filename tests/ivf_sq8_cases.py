"""Data and float64 references of the IVF_SQ8 tests (tests/test_ivf_sq8_unit_gpu.py, tests/test_ivf_sq8_host.py): nothing here
runs a kernel.  The SQ8 rule itself is tests/sq8_ref.py; the float64 assignment / probe rule is tests/ivf_cases.py's.

Two kinds of data.
  integer  rows and queries with column 0 = +-127 (random sign) and the other columns integers in [-4, 4], the whole vector scaled
           by 2^-j (j = 0 or 7).  The SQ8 scale is then 127 * 2^-j / 127 = 2^-j exactly, the codes are the entries and the vector a
           row stands for, x^ = code * scale, IS the row (asserted against sq8_ref.quantize on the CPU).  Centroids are rows or
           small-integer vectors on the same 2^-j grid, so every product and every partial sum of an assignment or probe score is an
           integer multiple of 2^-2j below 2^24 of them: exact in fp32 in ANY summation order.  No row and no query may be left out
           on this data, and ties are allowed to occur (two equal rows; forty equal appended rows).
  normal   standard normal rows and queries scaled to unit length, as in ivf_cases.py: the fp32 sums err by ~1e-7, so a row's list
           or a query's probe set may differ from the float64 rule over x^ only where the float64 gap between the deciding list
           scores is under GAP = 1e-5 (ivf_cases.py's bound and reasoning); at most ROWS_LEFT_OUT_MAX of the rows and
           QUERIES_LEFT_OUT_MAX of the queries may be left out (by the float64 rule on the CPU, these cases: at most 0.065 % of the rows
           and no query are that close).
Centroids always include one that attracts no row (`far`, list 0) and one that attracts exactly one row (`single`, list 1) when
nlist >= 7, otherwise rows of the data, so lists come out empty, of one row and of sizes that are no multiple of 16.
dim 100 gives stride 112: pad codes and a partial last 64-byte k-step."""
import functools

import numpy as np

import sq8_ref as R
from ivf_cases import _unit

# (dim, n, nlist, data, j): a sample of {64, 100, 384, 768} x {257, 3001, 20000} x {1, 7, 64} x {integer, normal} in which every
# value and both scalings of the integer data occur
CASES = [
    (64, 257, 1, "integer", 0),
    (100, 3001, 7, "normal", 0),
    (384, 257, 7, "integer", 7),
    (100, 3001, 64, "integer", 0),
    (768, 3001, 64, "integer", 7),
    (768, 20000, 64, "normal", 0),
    (64, 20000, 64, "integer", 0),
    (384, 20000, 7, "normal", 0),
    (100, 257, 1, "normal", 0),
]
BIG = (768, 20000, 64, "normal", 0)      # the case of the query-slicing test
NQ_MAX = 100
NQ_BIG = 300
APPENDED = 40
GAP = 1e-5
ROWS_LEFT_OUT_MAX = 0.01
QUERIES_LEFT_OUT_MAX = 0.10


def _integer(rng, n, dim):
    a = rng.integers(-4, 5, (n, dim)).astype(np.float32)
    a[:, 0] = np.float32(127) * (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
    return a


@functools.lru_cache(maxsize=None)
def data(kind, dim, n, nlist, j=0):
    """(X [n + APPENDED, dim], Q [NQ_MAX, dim], centroids [nlist, dim]); read-only.  Rows [n, n + APPENDED) are appended later and
    lead query 0's ranking.  Query 1 points at the `far` centroid and query 2 at the `single` one (nlist >= 7)."""
    rng = np.random.default_rng(104729 * dim + 31 * n + nlist + (5 if kind == "integer" else 0) + j)
    if kind == "integer":
        X, Q = _integer(rng, n + APPENDED, dim), _integer(rng, NQ_MAX, dim)
        X[n // 2] = X[n // 3]                      # two equal rows: equal scores for every query
    else:
        X, Q = _unit(rng.standard_normal((n + APPENDED, dim))), _unit(rng.standard_normal((NQ_MAX, dim)))
    picks = np.sort(rng.choice(n, nlist, replace=False))
    if kind == "integer" and nlist >= 7:           # a row centroid of either sign, so that every row has one on its side
        X[picks[2], 0], X[picks[3], 0] = np.float32(127), np.float32(-127)
    C = X[picks].copy()
    if nlist >= 7:
        lone = int(np.setdiff1d(np.arange(n), np.concatenate([picks, [n // 2, n // 3]]))[n // 5])
        if kind == "integer":
            far = np.full(dim, 40, np.float32)     # x . far <= 160 (dim - 1) < 1/2 |far|^2 = 800 (dim - 1), by more than any row centroid loses
            far[0] = 0
            X[lone, 1:] = np.float32(4)            # the one row that leans on (1, ..., 1): 3/2 of it outside column 0 is its centroid
            single = X[lone] * np.float32(1.5)
            single[0] = X[lone, 0]
            C[0], C[1] = far, single
            Q[1], Q[2] = far * np.float32(2), X[lone]
        else:
            far = _unit(rng.standard_normal((1, dim)))[0]
            C[0] = far * np.float32(5)             # x . c <= 5 < 1/2 |c|^2 - 1/2: no row prefers it to a row centroid
            C[1] = X[lone] * np.float32(1.5)
            Q[1] = far * np.float32(10)
            Q[2] = X[lone] * np.float32(10)
    X[n:] = Q[:1] * np.float32(2)
    if kind == "integer":
        scale = np.float32(2.0 ** -j)
        X, Q, C = X * scale, Q * scale, C * scale
    for a in (X, Q, C):
        a.flags.writeable = False
    return X, Q, C


def dequantized(codes, scales):
    """x^[c] = fl((float)code[c] * scale): one fp32 product per element."""
    return codes.astype(np.float32) * np.asarray(scales, np.float32)[:, None]


@functools.lru_cache(maxsize=None)
def reference(case):
    """(codes, scales, x^ of rows [0, n + APPENDED), SQ8 scores [NQ_MAX, n + APPENDED]) of a case by tests/sq8_ref.py; read-only,
    computed once and shared by the tests of the case."""
    dim, n, nlist, kind, j = case
    X, Q, _C = data(kind, dim, n, nlist, j)
    cr, sr = R.quantize(X)
    cq, sq = R.quantize(Q)
    out = (cr, sr, dequantized(cr, sr), R.scores(cq, sq, cr, sr))
    for a in out:
        a.flags.writeable = False
    return out
