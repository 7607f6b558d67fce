"""vrag_dense_index_search_filtered / vrag_sparse_index_search_filtered against oracle/topk_ref.c run over the passing rows
only (ids mapped back; dtype 0 on the bf16-rounded rows).  Everything is compared for exact equality: ids and score bits.

Shapes.  vrag_dense_index_create takes dims that are multiples of 8 only, so 4 and 260 cannot be built: the test pins that
refusal and runs 8 and 264 (not a multiple of 16 / of the 256-column staging round) in their place, beside 64 and 768.
Every row count, batch size and k of the list below is reached in every index through the rotation in `_combos`.

"Every bit set == the unfiltered call": the unfiltered search promises the oracle's chain bit for bit on dyadic-grid data
(every summation order is exact there) and, on arbitrary data, where its exact fp32 kernels run (fp32 rows, dim % 32 == 0,
dim <= 768, k <= 16; csrc/topk.hip dense_use_exact); elsewhere it differs from the chain by summation order, so there the
all-set mask is held to the oracle alone."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import topk_ref as T

pytestmark = pytest.mark.gpu

ROWS = [1, 31, 32, 33, 4095, 4097, 70001]
NQS = [1, 2, 17, 33]
KS = [1, 5, 64, 65, 200]
DENSE_SHAPES = [(8, 1), (64, 31), (264, 32), (768, 33), (64, 4095), (264, 4097), (768, 4097), (8, 4097), (64, 70001), (264, 70001)]
MARGIN, CANARY_F, CANARY_I = 64, np.float32(12345.5), np.int64(-777)
_FP, _LP = C.POINTER(C.c_float), C.POINTER(C.c_int64)


def test_shapes_cover_the_list():
    assert {r for _d, r in DENSE_SHAPES} == set(ROWS) and {d for d, _r in DENSE_SHAPES} == {8, 64, 264, 768}


@pytest.mark.parametrize("dim", [4, 260, 12, 8 * 513])
def test_dims_the_index_refuses(dim):
    """4 and 260 of the issue's list (and one dim that is no multiple of 4): no index, so nothing to search."""
    from verbatim_rag_amd import _lib

    h = C.c_void_p()
    assert _lib.load().vrag_dense_index_create(dim, 16, 1, 0, C.byref(h)) == -1 and not h.value


def _masks(rng, n):
    half = rng.random(n) < 0.5
    words_clear = half.copy()
    for w in range(0, (n + 31) // 32, 2):
        words_clear[32 * w:32 * w + 32] = False
    if n > 2048:
        words_clear[:2048] = False          # two whole workgroups of the compaction without a bit
    one = np.zeros(n, bool)
    one[rng.choice(n, max(1, n // 100), replace=False)] = True
    first, last, tail = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    first[0], last[n - 1] = True, True
    tail[(n - 1) // 32 * 32:] = True
    return [("none", np.zeros(n, bool)), ("row0", first), ("last", last), ("all", np.ones(n, bool)), ("1pct", one),
            ("50pct", half), ("words_clear", words_clear), ("last_word", tail)]


def _combos(j):
    return [(NQS[j % 4], KS[j % 5]), (NQS[(j + 2) % 4], KS[(j + 3) % 5])]


def _words(mask):
    from verbatim_rag_amd.vector_stores import _bitmap

    return _bitmap(mask)


def _guarded(nq, k):
    s = np.full(nq * k + 2 * MARGIN, CANARY_F, np.float32)
    i = np.full(nq * k + 2 * MARGIN, CANARY_I, np.int64)
    return s, i


def _unguard(s, i, nq, k):
    for buf, canary in ((s, CANARY_F), (i, CANARY_I)):
        assert (buf[:MARGIN] == canary).all() and (buf[MARGIN + nq * k:] == canary).all(), "write outside the result arrays"
    return s[MARGIN:MARGIN + nq * k].reshape(nq, k).copy(), i[MARGIN:MARGIN + nq * k].reshape(nq, k).copy()


def _dense_filtered(sh, Q, k, mask, n_allow=None):
    """The raw call with canary margins around both result arrays."""
    from verbatim_rag_amd import _lib

    Q = np.ascontiguousarray(Q, np.float32)
    words = _words(mask)
    s, i = _guarded(len(Q), k)
    rc = sh._lib.vrag_dense_index_search_filtered(
        sh._h, Q.ctypes.data_as(_FP), len(Q), k, words.ctypes.data_as(C.c_void_p), len(mask) if n_allow is None else n_allow,
        C.cast(C.c_void_p(s.ctypes.data + 4 * MARGIN), _FP), C.cast(C.c_void_p(i.ctypes.data + 8 * MARGIN), _LP), None)
    assert rc == 0, _lib.last_error()
    return _unguard(s, i, len(Q), k)


def _pad(s, i, k):
    pad = k - s.shape[1]
    return (np.pad(s, ((0, 0), (0, pad)), constant_values=-np.inf).astype(np.float32),
            np.pad(i, ((0, 0), (0, pad)), constant_values=-1).astype(np.int64))


def _ref_dense(stored, Q, k, passing):
    kk = min(k, len(passing))
    if kk == 0:
        return np.full((len(Q), k), -np.inf, np.float32), np.full((len(Q), k), -1, np.int64)
    s, i = T.dense_topk(stored[passing], Q, kk)
    return _pad(s, passing[i], k)


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what


@functools.lru_cache(maxsize=None)
def _dense_data(data, dim, n):
    rng = np.random.default_rng(1000 * dim + n + (7 if data == "grid" else 0))
    if data == "grid":      # dyadic grid, few levels: exact sums in any order, bf16-exact, exact ties all over the ranking
        X = rng.integers(-4, 5, (n + 40, dim)).astype(np.float32) / np.float32(8)
        Q = rng.integers(-4, 5, (33, dim)).astype(np.float32) / np.float32(8)
        if n > 2:
            X[n // 2] = X[n // 3]
    else:
        X = rng.standard_normal((n + 40, dim)).astype(np.float32)
        Q = rng.standard_normal((33, dim)).astype(np.float32)
    X[n:] = np.repeat(Q[:1], 40, axis=0) * np.float32(2)        # the rows appended later: at the head of query 0's ranking
    X.flags.writeable = Q.flags.writeable = False
    return X, Q


@pytest.mark.parametrize("dim,n", DENSE_SHAPES)
@pytest.mark.parametrize("dtype,data", [(0, "grid"), (1, "grid"), (2, "grid"), (1, "normal"), (2, "normal")])
def test_dense_filtered_equals_the_oracle_over_the_passing_rows(dtype, data, dim, n):
    from verbatim_rag_amd.vector_stores import DenseShard

    X, Q = _dense_data(data, dim, n)
    stored = T.bf16_round(X) if dtype == 0 else X
    rng = np.random.default_rng(n + dim + dtype)
    sh = DenseShard(dim, n + 64, "bf16" if dtype == 0 else "f32", prefilter=dtype == 2)
    try:
        sh.add(X[:n])
        plain = [(1, 5), (33, 5), (2, 65), (17, 16)]
        before = [sh.search(Q[:nq], k) for nq, k in plain]
        for j, (name, mask) in enumerate(_masks(rng, n)):
            passing = np.nonzero(mask)[0]
            for nq, k in _combos(j):
                got = _dense_filtered(sh, Q[:nq], k, mask)
                _same(got, _ref_dense(stored, Q[:nq], k, passing), (name, nq, k))
                if name == "all" and (data == "grid" or (dim % 32 == 0 and dim <= 768 and k <= 16)):
                    _same(got, sh.search(Q[:nq], k), ("all == unfiltered", nq, k))
                if name == "none":
                    assert (got[1] == -1).all() and np.isneginf(got[0]).all()
            _same(sh.search_filtered(Q[:2], 5, _words(mask), n), _ref_dense(stored, Q[:2], 5, passing), (name, "class method"))
        for k in (5, 65):       # nothing passes, one page and paged (the "none" mask above meets k = 1 and k = 65 too)
            _same(_dense_filtered(sh, Q[:2], k, np.ones(n, bool), n_allow=0), _ref_dense(stored, Q[:2], k, passing[:0]), ("n_allow = 0", k))
        for (nq, k), want in zip(plain, before):
            _same(sh.search(Q[:nq], k), want, ("unfiltered after the filtered calls", nq, k))
        # a mask built before an append stays valid: rows at or beyond n_allow never appear, with or without bits for them
        all_n = _dense_filtered(sh, Q[:17], 5, np.ones(n, bool))
        sh.add(X[n:])
        for nq, k in ((17, 5), (1, 65)):
            want = _ref_dense(stored, Q[:nq], k, np.arange(n))
            _same(_dense_filtered(sh, Q[:nq], k, np.ones(n, bool)), want, ("after the append", nq, k))
            _same(_dense_filtered(sh, Q[:nq], k, np.ones(n + 40, bool), n_allow=n), want, ("bits beyond n_allow", nq, k))
        _same(_dense_filtered(sh, Q[:17], 5, np.ones(n, bool)), all_n, "same bits as before the append")
        got = _dense_filtered(sh, Q[:2], 5, np.ones(n + 100, bool))       # n_allow beyond the index: the index's rows
        _same(got, _ref_dense(stored, Q[:2], 5, np.arange(n + 40)), "n_allow > size")
    finally:
        sh.close()


# ---------------------------------------------------------------------------------------------------------------- sparse
SPARSE_KS = KS
SPARSE_NQS = [1, 9, 17]


@functools.lru_cache(maxsize=None)
def _sparse_data(vocab, n, weights):
    rng = np.random.default_rng(vocab + 31 * n + len(weights))
    hot = np.concatenate([np.arange(0, 160), np.arange(vocab - 40, vocab)])          # terms that queries and documents share
    lens = rng.integers(0, 41, n + 40)
    if n >= 63:
        lens[[0, 5, 17, n - 1]] = [0, 40, 3, 0]
    else:
        lens[0] = 7
    lens[n:] = 30

    def val(m):
        return rng.integers(1, 64, m).astype(np.float32) / np.float32(64) if weights == "grid" else rng.random(m, dtype=np.float32) + np.float32(0.01)

    indptr = np.zeros(n + 41, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = np.concatenate([np.sort(rng.choice(hot, int(m), replace=False)) for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    values = val(int(indptr[-1]))
    queries = []
    for q in range(17):
        m = 0 if q == 4 else int(rng.integers(1, 25))                                  # query 4 has no term
        t = np.sort(rng.choice(hot, m, replace=False))
        queries.append({int(a): float(b) for a, b in zip(t, val(m))})
    for a in (indptr, indices, values):
        a.flags.writeable = False
    return indptr, indices, values, queries


def _sparse_filtered(sh, queries, k, mask, n_allow=None):
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.vector_stores import _IP, dicts_to_csr

    qp, qi, qv = dicts_to_csr(queries)
    words = _words(mask)
    nq = len(queries)
    s, i = _guarded(nq, k)
    rc = sh._lib.vrag_sparse_index_search_filtered(
        sh._h, qp.ctypes.data_as(_LP), qi.ctypes.data_as(_IP), qv.ctypes.data_as(_FP), nq, k, words.ctypes.data_as(C.c_void_p),
        len(mask) if n_allow is None else n_allow, C.cast(C.c_void_p(s.ctypes.data + 4 * MARGIN), _FP),
        C.cast(C.c_void_p(i.ctypes.data + 8 * MARGIN), _LP), None)
    assert rc == 0, _lib.last_error()
    return _unguard(s, i, nq, k)


def _ref_sparse(csr, vocab, queries, k, passing):
    from verbatim_rag_amd.vector_stores import csr_take_rows, dicts_to_csr

    kk = min(k, len(passing))
    if kk == 0:
        return np.full((len(queries), k), -np.inf, np.float32), np.full((len(queries), k), -1, np.int64)
    s, i = T.sparse_topk(*csr_take_rows(*csr, passing), vocab, *dicts_to_csr(queries), kk)
    return _pad(s, np.where(i >= 0, passing[np.where(i >= 0, i, 0)], -1), k)


@pytest.mark.parametrize("weights", ["grid", "uniform"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
@pytest.mark.parametrize("vocab", [1000, 30522])
def test_sparse_filtered_equals_the_oracle_over_the_passing_documents(vocab, n, weights):
    from verbatim_rag_amd.vector_stores import SparseShard

    indptr, indices, values, queries = _sparse_data(vocab, n, weights)
    csr = (indptr[:n + 1], indices[:indptr[n]], values[:indptr[n]])
    rng = np.random.default_rng(vocab + n)
    sh = SparseShard(vocab, *csr)
    try:
        plain = [(1, 5), (17, 5), (9, 65)]
        before = [sh.search(queries[:nq], k) for nq, k in plain]
        for j, (name, mask) in enumerate(_masks(rng, n)):
            passing = np.nonzero(mask)[0]
            for jj in (j, j + 3):
                nq, k = SPARSE_NQS[jj % 3], SPARSE_KS[jj % 5]
                got = _sparse_filtered(sh, queries[:nq], k, mask)
                _same(got, _ref_sparse(csr, vocab, queries[:nq], k, passing), (name, nq, k))
                if name == "all":
                    _same(got, sh.search(queries[:nq], k), ("all == unfiltered", nq, k))
                if name == "none":
                    assert (got[1] == -1).all() and np.isneginf(got[0]).all()
            _same(sh.search_filtered(queries[:9], 5, _words(mask), n), _ref_sparse(csr, vocab, queries[:9], 5, passing), (name, "class method"))
        for k in (5, 65):       # nothing passes, one page and paged (the "none" mask above meets k = 1 and k = 65 too)
            _same(_sparse_filtered(sh, queries[:2], k, np.ones(n, bool), n_allow=0), _ref_sparse(csr, vocab, queries[:2], k, passing[:0]), ("n_allow = 0", k))
        for (nq, k), want in zip(plain, before):
            _same(sh.search(queries[:nq], k), want, ("unfiltered after the filtered calls", nq, k))
    finally:
        sh.close()
    # n_allow shorter than the index: the 40 documents behind it (30 shared terms each) must not appear
    big = SparseShard(vocab, indptr, indices, values)
    try:
        for nq, k in ((9, 5), (1, 65)):
            want = _ref_sparse(csr, vocab, queries[:nq], k, np.arange(n))
            _same(_sparse_filtered(big, queries[:nq], k, np.ones(n, bool)), want, ("n_allow < n_docs", nq, k))
            _same(_sparse_filtered(big, queries[:nq], k, np.ones(n + 40, bool), n_allow=n), want, ("bits beyond n_allow", nq, k))
        got = _sparse_filtered(big, queries[:9], 5, np.ones(n + 100, bool))
        _same(got, _ref_sparse((indptr, indices, values), vocab, queries[:9], 5, np.arange(n + 40)), "n_allow > n_docs")
    finally:
        big.close()


def test_refusals_return_their_code_and_leave_the_handles_usable():
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.vector_stores import _IP, DenseShard, SparseShard, dicts_to_csr

    X, Q = _dense_data("grid", 64, 31)
    indptr, indices, values, queries = _sparse_data(1000, 63, "grid")
    csr = (indptr[:64], indices[:indptr[63]], values[:indptr[63]])
    dense, sparse = DenseShard(64, 64, "f32"), SparseShard(1000, *csr)
    lib = dense._lib
    try:
        dense.add(X[:31])
        mask = np.ones(31, bool)
        words = _words(mask)
        wp = words.ctypes.data_as(C.c_void_p)
        s, i = _guarded(2, 5)
        sp, ip = C.cast(C.c_void_p(s.ctypes.data + 4 * MARGIN), _FP), C.cast(C.c_void_p(i.ctypes.data + 8 * MARGIN), _LP)
        q = np.ascontiguousarray(Q[:2])
        qp = q.ctypes.data_as(_FP)
        bad_dense = [(qp, 2, 5, None, 31), (qp, 2, 0, wp, 31), (qp, 2, 1025, wp, 31), (qp, 0, 5, wp, 31), (qp, -1, 5, wp, 31),
                     (qp, 2, 5, wp, -1), (None, 2, 5, wp, 31)]
        for a in bad_dense:
            assert lib.vrag_dense_index_search_filtered(dense._h, a[0], a[1], a[2], a[3], a[4], sp, ip, None) == -1, a
            assert _lib.last_error()
        assert lib.vrag_dense_index_search_filtered(None, qp, 2, 5, wp, 31, sp, ip, None) == -1
        assert lib.vrag_dense_index_search_filtered(dense._h, qp, 2, 5, wp, 31, None, ip, None) == -1
        _unguard(s, i, 2, 5)                                              # nothing was written
        _same(_dense_filtered(dense, Q[:2], 5, mask), _ref_dense(X, Q[:2], 5, np.arange(31)), "dense handle after the refusals")
        with pytest.raises(ValueError):
            dense.search_filtered(Q[:2], 5, words[:0], 31)               # a bitmap shorter than n_allow never reaches the library

        cp, ci, cv = dicts_to_csr(queries[:2])
        a3 = (cp.ctypes.data_as(_LP), ci.ctypes.data_as(_IP), cv.ctypes.data_as(_FP))
        m63 = np.ones(63, bool)
        w63 = _words(m63)
        w63p = w63.ctypes.data_as(C.c_void_p)
        for nq, k, w, n_allow in [(2, 5, None, 63), (2, 0, w63p, 63), (2, 1025, w63p, 63), (0, 5, w63p, 63), (2, 5, w63p, -1)]:
            assert lib.vrag_sparse_index_search_filtered(sparse._h, *a3, nq, k, w, n_allow, sp, ip, None) == -1, (nq, k, n_allow)
        bad_term = np.array([1000], np.int32)
        one_ptr, one_val = np.array([0, 1], np.int64), np.array([1.0], np.float32)
        assert lib.vrag_sparse_index_search_filtered(sparse._h, one_ptr.ctypes.data_as(_LP), bad_term.ctypes.data_as(_IP),
                                                     one_val.ctypes.data_as(_FP), 1, 5, w63p, 63, sp, ip, None) == -1
        _unguard(s, i, 2, 5)
        _same(_sparse_filtered(sparse, queries[:2], 5, m63), _ref_sparse(csr, 1000, queries[:2], 5, np.arange(63)),
              "sparse handle after the refusals")
    finally:
        dense.close()
        sparse.close()
