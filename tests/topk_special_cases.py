"""Search inputs far from magnitude 1: signed zeros, denormal scores and extreme scales, for every search route
(tests/test_topk_special_values_host.py proves each construction against the oracle alone, tests/test_topk_special_values_gpu.py
runs them).  All inputs are finite; NaN and +-inf are outside the contract.

A family is one kernel family at the smallest shape of tests/topk_instantiation_cases.py that selects it:

    Family(name, kind, dtype, dim, n, nq, k, base, via, expect, fallback)

base      the data set of the instantiation table ("grid" | "gauss") that the scaled kinds multiply
expect    the launch set of an ordinary search of that shape, looked up in the instantiation table where the shape is one of its
          cases (`_table`), stated here otherwise
fallback  what the full scan behind the prefilter's flags adds (prefilter families only; empty elsewhere)

Data kinds of a dense family:

    "scaled-75" "scaled-60" "scaled+60" "scaled+66"
              rows = base rows * 2^e, queries = base queries * 2^-e.  Both scalings are exact (every element stays normal), so every
              product, every partial sum and therefore every score and the whole ranking are the unscaled set's, bit for bit.
    "tiny"    rows = integers |g| <= 4 times 2^-72, queries = integers |g| <= 4 times 2^-74: every product is a multiple of 2^-146 of
              at most 16 * 2^-146, every partial sum of up to 1 536 of them stays below 2^-131: all scores are denormals that fp32
              holds exactly in any summation order (`tiny_bound`).
    "zeros"   rows and queries of magnitude 2^-80 g: every product (at most 2^-156) underflows, every score is +-0.  Row 0 is the
              negated sign pattern of query 0 (its chain score is -0.0, and it has the lowest id: an order that puts -0 below +0
              shows in the ids), some rows hold -0.0 elements, some are all zero, and six rows of magnitude 2^-66 g score denormals
              above and below the zeros.  The last query of a batch is all zero: the whole shard ties.
    "zeroq"   the same rows, every query all zero.
    "scaled+126"  (prefilter families only) grid rows times 2^126 and grid queries times 2^-126: every element and every score is
              finite, but the rows' norms are beyond fp32.  The prefilter has no bound for such rows and must answer by the full scan.

The rule a result is held to (`compare`): ids equal the oracle's; scores equal the oracle's bit for bit where the oracle's score is
not zero; where it is zero the score is a zero of either sign -- a tree-shaped sum gives +0 where the chain gives -0, so the sign of
a zero is no part of the contract, the tie between zeros is.
"""
import zlib
from collections import namedtuple

import numpy as np

import test_topk_instantiations_gpu as G          # the instantiation table's data builders
import topk_instantiation_cases as T

Family = namedtuple("Family", "name kind dtype dim n nq k base via expect fallback")

SCALES = (-75, -60, 60, 66)
SCALED = tuple(f"scaled{e:+d}" for e in SCALES)
DENSE_KINDS = SCALED + ("tiny", "zeros", "zeroq")
OVERFLOW = "scaled+126"
TINY_X_EXP, TINY_Q_EXP, TINY_G = -72, -74, 4
ZERO_EXP, ZERO_BIG_EXP = -80, -66
MAX_DIM = 1536

ML, MS = T.ML, T.MS


def _table(dtype, dim, n, nq, k, data, via="host", kind="dense"):
    """The expected launch set of that case of the instantiation table."""
    hits = [c for c in T.CASES if (c.kind, c.dtype, c.dim, c.n, c.nq, c.k, c.data, c.via) == (kind, dtype, dim, n, nq, k, data, via)]
    assert len(hits) == 1, (dtype, dim, n, nq, k, data, via)
    return hits[0].expect


def _fam(name, dtype, dim, n, nq, k, base, via="host", expect=None, fallback=()):
    expect = _table(dtype, dim, n, nq, k, base) if expect is None else frozenset(expect)
    return Family(name, "dense", dtype, dim, n, nq, k, base, via, expect, frozenset(fallback))


_X6, _X3 = {("EXACT", 6, 0), ML}, {("EXACT", 3, 0), ML}
PFC = ("PF_COMBINE", 0, 0)

DENSE = [
    _fam("scalar-bf16", "bf16", 24, 129, 1, 10, "grid"),
    _fam("scalar-f32", "f32", 24, 129, 1, 17, "grid"),
    _fam("mfma", "bf16", 128, 127, 32, 16, "grid"),
    _fam("mfma2", "bf16", 384, 129, 3, 16, "grid"),
    _fam("exact", "f32", 32, 129, 5, 10, "gauss"),
    _fam("exact2", "f32", 384, 129, 5, 10, "gauss"),
    # the three prefilter routes; behind their flags the host call of the one-pass route runs the plain scan, the batch routes the
    # gated scan and the per-query pick (the "bunched" cases of the instantiation table)
    _fam("pf-one", "f32+image", 256, 4097, 1, 16, "grid", fallback=_X6),
    _fam("pf-multi", "f32+image", 256, 4097, 2, 16, "gauss", fallback=_X6),
    _fam("pf-collect", "f32+image", 512, 4097, 5, 16, "gauss", fallback=_X3 | {PFC}),
    _fam("pf-64", "f32+image", 512, 4224, 257, 1, "gauss", fallback=_X3 | {PFC}),
    # the tiled search logs none of its own kernels (tests/test_topk_unit_gpu.py); 4 096 rows of 64 are the smallest shard it takes
    _fam("tiled-bf16", "bf16", 64, 4096, 3, 10, "grid", expect=()),
    # the device call of a shard on the scan route launches what the host call does
    _fam("device", "f32", 32, 129, 5, 10, "gauss", via="device", expect=_table("f32", 32, 129, 5, 10, "gauss")),
    _fam("paged-65", "f32", 8, 2049, 1, 65, "grid"),
    _fam("paged-200", "f32", 8, 2049, 1, 200, "grid", expect=_table("f32", 8, 2049, 1, 65, "grid")),
    # the filtered kernels are not logged; their per-query merge is
    _fam("filtered", "f32", 32, 129, 5, 10, "gauss", via="filtered", expect={ML}),
]

# Routes whose matrix-core instruction flushes denormal products or sums (nothing in their code can change that): on "tiny" data
# every product and every partial sum is denormal, so such a route returns the other well-defined answer -- every score zero, ids
# 0 .. k-1.  family name -> the instruction.
FLUSHES = {}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(("special",) + key).encode()))


def _case(f, data=None):
    """The family as a case of the instantiation table (its data builders take one)."""
    return T.Case(f.kind, f.dtype, f.dim, f.n, f.nq, f.k, data or f.base, f.expect, 64, 64 if f.kind == "dense" else 63, "host")


def _pow2(e):
    return np.float32(2.0) ** np.float32(e)


def base_data(f):
    """(rows, queries) of the family's unscaled data set."""
    c = _case(f)
    X = G.dense_rows(T.index_key(c))
    return X, G.dense_queries(c, X)


def scaled(X, Q, e):
    return X * _pow2(e), Q * _pow2(-e)


def tiny_bound(dim):
    """The largest |partial sum| of a tiny dot product, as an exponent: dim * (G 2^-72) (G 2^-74) <= 2^result."""
    return int(np.ceil(np.log2(dim * TINY_G * TINY_G))) + TINY_X_EXP + TINY_Q_EXP


def tiny_data(f):
    rng = _rng("tiny", f.name)
    X = rng.integers(-TINY_G, TINY_G + 1, size=(f.n, f.dim)).astype(np.float32) * _pow2(TINY_X_EXP)
    Q = rng.integers(-TINY_G, TINY_G + 1, size=(f.nq, f.dim)).astype(np.float32) * _pow2(TINY_Q_EXP)
    if f.n > 8:
        X[f.n // 2] = X[f.n // 3]                 # an exact tie between denormal scores
    return X, Q


ZERO_BIG_ROWS = 6


def zeros_data(f, zero_queries=False):
    rng = _rng("zeros", f.name)
    n, dim, nq = f.n, f.dim, f.nq
    gq = rng.integers(1, TINY_G + 1, size=(nq, dim)) * rng.choice([-1, 1], size=(nq, dim))
    Q = gq.astype(np.float32) * _pow2(ZERO_EXP)
    X = rng.integers(-TINY_G, TINY_G + 1, size=(n, dim)).astype(np.float32) * _pow2(ZERO_EXP)
    sign0 = np.sign(gq[0]).astype(np.float32)
    X[0] = -sign0 * _pow2(ZERO_EXP)               # every product with query 0 is negative: the chain ends in -0.0
    if n > 1:
        X[1] = sign0 * _pow2(ZERO_EXP)            # ... and its mirror image in +0.0
    for r in range(2, n, 5):                      # -0.0 elements
        X[r, rng.integers(0, dim, size=max(1, dim // 8))] = np.float32(-0.0)
    for r in range(3, n, 7):                      # all-zero rows, of either sign
        X[r] = np.float32(-0.0) if r % 2 else np.float32(0.0)
    if n >= 64:                                   # denormal scores above and below the zeros (query 0)
        at = rng.choice(np.arange(8, n), size=ZERO_BIG_ROWS, replace=False)
        for j, r in enumerate(at):
            X[r] = (1 if j % 2 else -1) * (1 + j // 2) * sign0 * _pow2(ZERO_BIG_EXP)
    if zero_queries:
        Q[:] = 0
    elif nq > 1:
        Q[-1] = 0
        Q[-1, ::3] = np.float32(-0.0)
    return X, Q


def dense_kinds(f):
    return DENSE_KINDS + ((OVERFLOW,) if f.fallback else ())


def dense_data(f, kind):
    if kind == OVERFLOW:
        c = _case(f, "grid")
        X = G.dense_rows(T.index_key(c))
        return scaled(X, G.dense_queries(c, X), 126)
    if kind.startswith("scaled"):
        return scaled(*base_data(f), int(kind[len("scaled"):]))
    if kind == "tiny":
        return tiny_data(f)
    return zeros_data(f, zero_queries=kind == "zeroq")


def dense_expect(f, kind):
    """The launch set of the family on that kind of data.  The prefilter's bound has an absolute floor of 1e-30 (its slack against
    its own rounding), far above every denormal score: on "tiny", "zeros" and "zeroq" data every row is within the bound of every
    other, each query is flagged and the full scan answers it.  So it does where the rows' norms overflow ("scaled+126")."""
    if f.fallback and (kind == OVERFLOW or not kind.startswith("scaled")):
        return f.expect | f.fallback
    return f.expect


def filter_mask(n):
    """The 50 % mask of the filtered families: every other row, row 0 among them."""
    return np.arange(n) % 2 == 0


# ---------------------------------------------------------------------------------------------------------------- worst case
WORST_N, WORST_DIM, WORST_K, WORST_BATCH = 50_000, 128, 10, 70


def worst_case(e=0):
    """The construction of test_prefilter_bound_holds_where_bf16_rounding_is_worst_case (tests/test_topk_gpu.py), rows times 2^e and
    queries times 2^-e: ten rows T whose bf16 image loses 2^-8 of their norm along the query, behind forty decoys whose image
    scores are above T's and whose exact scores are below.  -> (X, Q [2, dim], Qb [70, dim], decoys, truth)"""
    rng = np.random.default_rng(61)
    n, dim, k = WORST_N, WORST_DIM, WORST_K
    h = dim // 2
    X = (0.01 * rng.standard_normal((n, dim))).astype(np.float32)
    decoys = rng.choice(np.arange(100, 30_000), size=40, replace=False)
    truth = np.sort(rng.choice(np.arange(40_000, n), size=k, replace=False))
    X[decoys] = 0.0
    X[decoys, h:] = np.float32(1.0 - 2.0 ** -9 + 2.0 ** -20)
    X[truth] = 0.0
    X[truth, :h] = np.float32(1.0 + 2.0 ** -8)
    Q = np.ones((2, dim), dtype=np.float32)
    Q[0, h:] = np.float32(1.0 + 1.485 * 2.0 ** -8)
    Q[1] = rng.standard_normal(dim).astype(np.float32)
    Qb = np.repeat(Q[:1], WORST_BATCH, axis=0) * np.linspace(0.5, 2.0, WORST_BATCH, dtype=np.float32)[:, None]
    return X * _pow2(e), Q * _pow2(-e), Qb * _pow2(-e), decoys, truth


# ---------------------------------------------------------------------------------------------------------------- sparse
SFamily = namedtuple("SFamily", "name vocab nq k via expect")
SCAT = T.SCAT


def _stable(vocab, nq, k, data="grid"):
    return _table("csr", vocab, T.SPARSE_DOCS, nq, k, data, kind="sparse")


SPARSE = [
    SFamily("sparse-ldsq", 30522, 1, 10, "host", _stable(30522, 1, 10)),
    SFamily("sparse-hbmq", 65536, 2, 10, "host", _stable(65536, 2, 10)),
    SFamily("sparse-multi", 30522, 17, 10, "host", _stable(30522, 17, 10)),
    # the filtered kernel is not logged; the scatter of the query's dense vector and the per-query merge are
    SFamily("sparse-filtered", 30522, 2, 10, "filtered", frozenset({SCAT, ML})),
]
SPARSE_KINDS = tuple(f"{b}{e:+d}" for b in ("grid", "gauss") for e in SCALES) + ("denorm",)
DENORM_DOC_EXP, DENORM_HIT_EXP, DENORM_MISS_EXP, DENORM_G, DENORM_HIT_TERMS = -75, -70, -80, 5, 3


def sparse_data(f, kind):
    """(indptr, idx, val), (q_indptr, q_idx, q_val) of the instantiation table's corpus and queries with the kind's weights.

    "grid-75" ..: the grid or |Gaussian| weights, documents times 2^e and queries times 2^-e.
    "denorm": document weights 2^-75 g, g in 1 .. 5.  The first three terms of a query (hot terms: documents share them) weigh
    2^-70 g', the others 2^-80 g': a product of the first kind is a multiple of 2^-145 (a positive denormal; sums stay below
    2^-136 and are exact), one of the second kind at most 25 * 2^-155 < 2^-150 and rounds to +0 wherever it is added.  A document
    that shares only terms of the second kind scores +0 and is NOT a hit; one that shares a term of the first kind is."""
    rows = "gauss" if kind.startswith("gauss") else "grid"
    c = T.Case("sparse", "csr", f.vocab, T.SPARSE_DOCS, f.nq, f.k, rows, f.expect, 192, 63, "host")
    indptr, idx, val = G.sparse_corpus(T.index_key(c))
    qp, qi, qv = G.sparse_queries(c)
    if kind == "denorm":
        rng = _rng("denorm", f.name)
        val = rng.integers(1, DENORM_G + 1, size=len(val)).astype(np.float32) * _pow2(DENORM_DOC_EXP)
        g = rng.integers(1, DENORM_G + 1, size=len(qv)).astype(np.float32)
        pos = np.arange(len(qv)) - np.repeat(qp[:-1], np.diff(qp))
        qv = g * np.where(pos < DENORM_HIT_TERMS, _pow2(DENORM_HIT_EXP), _pow2(DENORM_MISS_EXP))
    else:
        e = int(kind[len(rows):])
        val, qv = val * _pow2(e), qv * _pow2(-e)
    return (indptr, idx, val.astype(np.float32)), (qp, qi, qv.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- SQ8
SQ8_DIM, SQ8_N, SQ8_NQ = 64, 257, 6


def sq8_data():
    """Rows and queries for tests/sq8_ref.py.  Gaussian rows whose maxima lie near 2^-100 (rows 0 .. 39), near 2^+100 (40 .. 79), in
    the denormals (80 .. 99) and near 1 (104 ..); row 5 is all zero, row 6 all -0.0; rows 100 .. 103 have a maximum of at most
    39 * 2^-149, so max / 127 underflows to zero in fp32 (every element non-zero, so the reference's division is defined: codes
    +-127, scale 0).  Queries: near 1; near 2^-37 (its scale times a 2^-100 row's is a denormal, and so are those scores); near
    2^+20; denormal; all zero; the sign pattern of row 0 at 2^-100 (against the 2^-100 rows the scale product underflows: scores
    of +0 and -0)."""
    rng = _rng("sq8")
    X = rng.standard_normal((SQ8_N, SQ8_DIM)).astype(np.float32)
    X[:40] *= _pow2(-100)
    X[40:80] *= _pow2(100)
    X[80:100] *= _pow2(-140)
    X[100:104] = rng.choice([-1, 1], size=(4, SQ8_DIM)).astype(np.float32) * rng.integers(1, 40, size=(4, SQ8_DIM)).astype(np.float32) * _pow2(-149)
    X[5] = 0.0
    X[6] = np.float32(-0.0)
    Q = rng.standard_normal((SQ8_NQ, SQ8_DIM)).astype(np.float32)
    Q[1] *= _pow2(-37)
    Q[2] *= _pow2(20)
    Q[3] *= _pow2(-140)
    Q[4] = 0.0
    Q[5] = np.sign(X[0]) * _pow2(-100)
    return X, Q


# ---------------------------------------------------------------------------------------------------------------- shard merge
def merge_lists():
    """Per-shard lists [3 shards][4 queries][8] sorted by (score desc, id asc) under the rule "zeros of either sign tie", with
    zero-score entries whose sign differs across and within shards, denormals on both sides of them and -1 tails.  -> scores, ids"""
    rng = _rng("merge")
    W, Q, K = 3, 4, 8
    pool = np.array([2.0 ** -140, 2.0 ** -149, 0.0, -0.0, 0.0, -0.0, -(2.0 ** -149), -(2.0 ** -130), 1.5], np.float32)
    scores = np.full((W, Q, K), -np.inf, np.float32)
    ids = np.full((W, Q, K), -1, np.int64)
    for q in range(Q):
        perm = rng.permutation(W * K)                      # global ids, unique across the shards
        for w in range(W):
            m = K if q < 3 else (K, 3, 0)[w]               # the last query: a short list and an empty one
            s = rng.choice(pool, size=m)
            if q == 1:
                s = np.where(np.arange(m) % 2 == (w % 2), np.float32(0.0), np.float32(-0.0))     # nothing but zeros
            i = np.sort(perm[w * K:w * K + m])
            order = np.lexsort((i, -(s + np.float32(0.0)).astype(np.float64)))    # + 0.0: -0 -> +0, the tie by id
            scores[w, q, :m], ids[w, q, :m] = s[order], i[order]
    return scores, ids


def merge_oracle(scores, ids, k):
    """All entries of a query by (score desc, id asc) with float comparison -- zeros tie -- in plain Python."""
    W, Q, K = scores.shape
    out_s, out_i = np.full((Q, k), -np.inf, np.float32), np.full((Q, k), -1, np.int64)
    for q in range(Q):
        ent = [(float(scores[w, q, j]), int(ids[w, q, j])) for w in range(W) for j in range(K) if ids[w, q, j] >= 0]
        ent.sort(key=lambda t: (-t[0], t[1]))       # -(-0.0) == 0.0 == -(0.0): the zeros compare equal
        for j, (s, i) in enumerate(ent[:k]):
            out_s[q, j], out_i[q, j] = s, i
    return out_s, out_i


# ---------------------------------------------------------------------------------------------------------------- the rule
def compare(s, i, rs, ri, what):
    """The failures of one result against the oracle's (rs, ri) as text."""
    out = []
    if not np.array_equal(i, ri):
        out.append(f"ids differ from the oracle at {np.argwhere(i != ri)[:4].tolist()}: got {i[i != ri][:4].tolist()}, want {ri[i != ri][:4].tolist()}")
    zero = rs == 0
    if not np.array_equal(s.view(np.uint32)[~zero], rs.view(np.uint32)[~zero]):
        bad = ~zero & (s.view(np.uint32) != rs.view(np.uint32))
        out.append(f"score bits differ from the oracle at {np.argwhere(bad)[:4].tolist()}: got {s[bad][:4].tolist()}, want {rs[bad][:4].tolist()}")
    if not (s[zero] == 0).all():
        out.append(f"{int((s[zero] != 0).sum())} scores are not zero where the oracle's are")
    return [f"{what}: {m}" for m in out]


def flushed_answer(nq, k, n):
    """What a route that flushes denormals returns on "tiny" data: every score zero, ids ascending."""
    kk = min(k, n)
    s, i = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)
    s[:, :kk], i[:, :kk] = 0.0, np.arange(kk)
    return s, i
