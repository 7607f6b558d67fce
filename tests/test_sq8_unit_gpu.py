"""vrag_sq8_index_* through the product ABI (csrc/sq8.hip) against tests/sq8_ref.py, bit for bit: the stored codes and scales,
the search under the scan kernel, the tile kernel and the automatic route, the filtered search, appends and refusals.

Data: Gaussian rows and queries with per-vector magnitudes spread over 1e-3 .. 1e3 (a swapped row / query scale shows), a block
of exact duplicate rows that one query equals (ties -> id asc at the head of its list), a few all-zero rows and one all-zero
query (every score +0: the whole list is id asc).  One index per (dim, n), built once and shared."""
import ctypes as C

import numpy as np
import pytest

import sq8_ref as R

pytestmark = pytest.mark.gpu

MARGIN, CANARY_F, CANARY_I = 64, np.float32(12345.5), np.int64(-777)
_FP, _LP = C.POINTER(C.c_float), C.POINTER(C.c_int64)
NQ_MAX, EXTRA = 100, 40          # queries per data set; append room of every index
ZERO_Q, DUP_Q = 3, 1             # the all-zero query; the query that equals the duplicated row

# (dim, n, nq, k): every dim of {24, 64, 384, 768}, n of {1, 63, 64, 128, 257, 4097, 40000}, nq of {1, 4, 5, 17, 64, 65, 100},
# k of {1, 10, 64, 65, 128, 200, 1024}.  The pages of k > 64: (24, 64, 5, 65) a first page exactly full and an empty second;
# (24, 128, 4, 128) two exactly full pages, the loop ends on k; (64, 257, 4, 1024) the largest k, sixteen pages, exhausted in the fifth
CASES = [
    (24, 1, 1, 1), (24, 63, 4, 10), (24, 257, 5, 64), (24, 4097, 100, 200), (24, 64, 5, 65), (24, 128, 4, 128), (64, 257, 4, 1024),
    (64, 63, 17, 65), (64, 257, 64, 10), (64, 4097, 65, 10), (64, 40000, 4, 64), (64, 40000, 17, 1),
    (384, 1, 5, 10), (384, 257, 100, 1), (384, 4097, 1, 200), (384, 4097, 17, 64), (384, 40000, 64, 10),
    (768, 63, 65, 200), (768, 257, 1, 10), (768, 4097, 64, 65), (768, 4097, 5, 1), (768, 40000, 100, 10), (768, 40000, 1, 64),
]
_DATA, _BUILT, _SCORES = {}, {}, {}


def _ids(case):
    return "d%d-n%d-q%d-k%d" % case


def _data(dim, n):
    """(rows [n + EXTRA, dim], queries [NQ_MAX, dim]) fp32; rows [n, n + EXTRA) are the append room's."""
    if (dim, n) not in _DATA:
        rng = np.random.default_rng(1000 * dim + n)
        X = (rng.standard_normal((n + EXTRA, dim)) * 10.0 ** rng.uniform(-3, 3, (n + EXTRA, 1))).astype(np.float32)
        Q = (rng.standard_normal((NQ_MAX, dim)) * 10.0 ** rng.uniform(-3, 3, (NQ_MAX, 1))).astype(np.float32)
        if n >= 63:
            X[40:49] = X[40] / np.linalg.norm(X[40]) * np.float32(1e6)     # nine copies, longer than any other row: ties at the head
            X[[5, 17, n - 1]] = 0.0                  # all-zero rows, the last row among them
            Q[DUP_Q] = X[40] * np.float32(0.5)       # same codes as the duplicated row: its copies lead this list
            Q[10:20] = X[20:30] + (0.1 * np.abs(X[20:30]).max(axis=1, keepdims=True) * rng.standard_normal((10, dim))).astype(np.float32)
        Q[ZERO_Q] = 0.0
        _DATA[(dim, n)] = (X, Q)
    return _DATA[(dim, n)]


def _built(dim, n):
    if (dim, n) not in _BUILT:
        from verbatim_rag_amd.vector_stores import Sq8Shard

        sh = Sq8Shard(dim, n + EXTRA)
        sh.add(_data(dim, n)[0][:n])
        _BUILT[(dim, n)] = sh
    return _BUILT[(dim, n)]


def _ref_scores(dim, n):
    """Reference scores [NQ_MAX, n] of the data set, computed once."""
    if (dim, n) not in _SCORES:
        X, Q = _data(dim, n)
        cr, sr = R.quantize(X[:n])
        cq, sq = R.quantize(Q)
        _SCORES[(dim, n)] = R.scores(cq, sq, cr, sr)
    return _SCORES[(dim, n)]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for sh in _BUILT.values():
        sh.close()
    _BUILT.clear()
    _DATA.clear()
    _SCORES.clear()


def _search(sh, Q, k, allow=None, n_allow=0):
    """The raw call with canary margins around the two result arrays -> (scores, ids)."""
    from verbatim_rag_amd import _lib

    Q = np.ascontiguousarray(Q, np.float32)
    nq = len(Q)
    s = np.full(nq * k + 2 * MARGIN, CANARY_F, np.float32)
    i = np.full(nq * k + 2 * MARGIN, CANARY_I, np.int64)
    sp, ip = C.cast(C.c_void_p(s.ctypes.data + 4 * MARGIN), _FP), C.cast(C.c_void_p(i.ctypes.data + 8 * MARGIN), _LP)
    if allow is None:
        rc = sh._lib.vrag_sq8_index_search(sh._h, Q.ctypes.data_as(_FP), nq, k, sp, ip, None)
    else:
        words = np.ascontiguousarray(allow, np.uint32)
        rc = sh._lib.vrag_sq8_index_search_filtered(sh._h, Q.ctypes.data_as(_FP), nq, k, words.ctypes.data, n_allow, sp, ip, None)
    assert rc == 0, _lib.last_error()
    for buf, canary in ((s, CANARY_F), (i, CANARY_I)):
        assert (buf[:MARGIN] == canary).all() and (buf[MARGIN + nq * k:] == canary).all(), "write outside the result arrays"
    return s[MARGIN:MARGIN + nq * k].reshape(nq, k).copy(), i[MARGIN:MARGIN + nq * k].reshape(nq, k).copy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what


# ---------------------------------------------------------------------------------------------------------------- 1. the stored rows
@pytest.mark.parametrize("dim", [24, 64, 384, 768])
def test_read_returns_the_rule_after_every_kind_of_append(dim):
    import torch

    from verbatim_rag_amd.vector_stores import Sq8Shard

    X = _data(dim, 257)[0]
    codes, scales = R.quantize(X)
    sh = Sq8Shard(dim, len(X))
    try:
        assert len(sh) == 0
        sh.add(X[:100])
        c, s = sh.read()
        assert len(sh) == 100 and np.array_equal(c, codes[:100]) and np.array_equal(s.view(np.uint32), scales[:100].view(np.uint32))
        t = torch.from_numpy(X[100:257]).cuda()
        sh.add_device(t.data_ptr(), 157)
        c, s = sh.read()
        assert len(sh) == 257 and np.array_equal(c, codes[:257]) and np.array_equal(s.view(np.uint32), scales[:257].view(np.uint32))
        sh.add(X[257:])                              # a second host append
        c, s = sh.read()
        assert len(sh) == len(X) and np.array_equal(c, codes) and np.array_equal(s.view(np.uint32), scales.view(np.uint32))
        c, s = sh.read(250, 20)                      # a window; either output alone
        assert np.array_equal(c, codes[250:270]) and np.array_equal(s, scales[250:270])
        only = np.empty(3, np.float32)
        assert sh._lib.vrag_sq8_index_read(sh._h, 5, 3, None, only.ctypes.data) == 0 and np.array_equal(only, scales[5:8])
        assert scales[5] == 0 and not codes[5].any() and codes.min() == -127 and codes.max() == 127
    finally:
        sh.close()


# ---------------------------------------------------------------------------------------------------------------- 2. search
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_search_equals_the_reference_on_every_route(case):
    dim, n, nq, k = case
    sh, Q = _built(dim, n), _data(dim, n)[1][:nq]
    want = R.topk(_ref_scores(dim, n)[:nq], k)
    try:
        for route in (1, 2, 0):
            sh.set_route(route)
            _same(_search(sh, Q, k), want, (case, route))
    finally:
        sh.set_route(0)
    if n >= 63 and nq > ZERO_Q:
        assert np.array_equal(want[1][ZERO_Q, :min(k, n)], np.arange(min(k, n))), "the all-zero query's list is id asc"
    if n >= 63 and nq > DUP_Q:
        assert np.array_equal(want[1][DUP_Q, :min(k, 9)], np.arange(40, 40 + min(k, 9))), "the duplicated rows lead their query's list"


@pytest.mark.parametrize("k", [5, 65])
def test_an_empty_index_answers_no_hits(k):
    from verbatim_rag_amd.vector_stores import Sq8Shard

    sh = Sq8Shard(64, 16)
    try:
        for route in (1, 2, 0):
            sh.set_route(route)
            s, i = _search(sh, _data(64, 257)[1][:3], k)
            assert len(sh) == 0 and (i == -1).all() and np.isneginf(s).all(), route
    finally:
        sh.close()


@pytest.mark.parametrize("nq", [1, 5, 64, 100])
@pytest.mark.parametrize("dim,n,k", [(768, 4097, 10), (24, 4097, 65)])
def test_the_two_routes_return_the_same_bits(dim, n, k, nq):
    sh, Q = _built(dim, n), _data(dim, n)[1][:nq]
    try:
        sh.set_route(1)
        scan = _search(sh, Q, k)
        sh.set_route(2)
        tile = _search(sh, Q, k)
    finally:
        sh.set_route(0)
    _same(scan, tile, (dim, n, k, nq))
    assert (scan[1][:, :min(k, n)] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. filtered search
@pytest.mark.parametrize("dim,n,nq,k", [(24, 257, 5, 10), (768, 4097, 17, 65), (64, 40000, 65, 10), (384, 4097, 4, 200), (24, 64, 5, 65)])
def test_filtered_search_equals_the_reference_over_the_passing_rows(dim, n, nq, k):
    from verbatim_rag_amd.vector_stores import _bitmap

    sh, Q, S = _built(dim, n), _data(dim, n)[1][:nq], _ref_scores(dim, n)[:nq]
    every_third = np.arange(n) % 3 == 0
    single = np.zeros(n, bool)
    single[n // 2] = True
    try:
        for route in (1, 2):
            sh.set_route(route)
            _same(_search(sh, Q, k, _bitmap(np.ones(n, bool)), n), _search(sh, Q, k), ("all ones", route))
            for name, mask in (("every third", every_third), ("single", single)):
                _same(_search(sh, Q, k, _bitmap(mask), n), R.topk(S, k, np.nonzero(mask)[0]), (name, route))
            short = n - n // 4                       # a mask shorter than the index: rows at or beyond it do not pass
            _same(_search(sh, Q, k, _bitmap(np.ones(n, bool)), short), R.topk(S, k, np.arange(short)), ("n_allow < size", route))
            _same(_search(sh, Q, k, _bitmap(every_third), short), R.topk(S, k, np.nonzero(every_third[:short])[0]), ("n_allow < size, every third", route))
            for words, n_allow in ((_bitmap(np.zeros(n, bool)), n), (None, 0), (_bitmap(np.ones(n, bool)), 0)):
                if words is None:
                    words = np.zeros(1, np.uint32)
                s, i = _search(sh, Q, k, words, n_allow)
                assert (i == -1).all() and np.isneginf(s).all(), ("none", route)
    finally:
        sh.set_route(0)


# ---------------------------------------------------------------------------------------------------------------- 4. appends
@pytest.mark.parametrize("dim,n", [(64, 257), (768, 4097)])
def test_a_search_right_after_an_append_sees_exactly_size_rows(dim, n):
    """Before the append nothing of the append room shows; right after it the appended rows -- copies of the first queries, so each
    leads its query's list -- are there, and the lists equal the reference over all n + EXTRA rows."""
    X, Q = _data(dim, n)
    X = X.copy()
    X[n:n + 8] = Q[20:28] / np.linalg.norm(Q[20:28], axis=1, keepdims=True) * np.float32(1e8)     # longer than any other row
    sh = _built(dim, n)
    try:
        for route in (1, 2):
            sh.set_route(route)
            _same(_search(sh, Q[:30], 10), R.topk(_ref_scores(dim, n)[:30], 10), ("before", route))
        sh.add(X[n:])
        assert len(sh) == n + EXTRA
        want = R.search(X, Q[:30], 10)
        assert np.array_equal(want[1][20:28, 0], np.arange(n, n + 8))
        for route in (1, 2, 0):
            sh.set_route(route)
            _same(_search(sh, Q[:30], 10), want, ("after", route))
    finally:
        _BUILT.pop((dim, n)).close()                 # the index has grown: the next user builds it afresh


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_handle_usable():
    from verbatim_rag_amd import _lib

    lib = _lib.load()
    for dim in (0, 4097, -8):
        h = C.c_void_p()
        assert lib.vrag_sq8_index_create(dim, 100, 0, C.byref(h)) == -1 and not h.value and "dim" in _lib.last_error()
    h = C.c_void_p()
    assert lib.vrag_sq8_index_create(64, 0, 0, C.byref(h)) == -1 and not h.value
    assert lib.vrag_sq8_index_create(64, 100, 0, None) == -1
    assert lib.vrag_sq8_index_size(None) == -1
    dim, n = 64, 257
    sh, Q = _built(dim, n), np.ascontiguousarray(_data(dim, n)[1][:2])
    s, i = np.empty((2, 1025), np.float32), np.empty((2, 1025), np.int64)
    qp, sp, ip = Q.ctypes.data_as(_FP), s.ctypes.data_as(_FP), i.ctypes.data_as(_LP)
    for k in (0, 1025, -1):
        assert lib.vrag_sq8_index_search(sh._h, qp, 2, k, sp, ip, None) == -1 and "k must be" in _lib.last_error()
        assert lib.vrag_sq8_index_search_filtered(sh._h, qp, 2, k, None, 0, sp, ip, None) == -1 and "k must be" in _lib.last_error()
    assert lib.vrag_sq8_index_search(sh._h, qp, 0, 5, sp, ip, None) == -1
    for args in ((None, qp, 2, 5, sp, ip, None), (sh._h, None, 2, 5, sp, ip, None), (sh._h, qp, 2, 5, None, ip, None), (sh._h, qp, 2, 5, sp, None, None)):
        assert lib.vrag_sq8_index_search(*args) == -1 and _lib.last_error()
    assert lib.vrag_sq8_index_search_filtered(sh._h, qp, 2, 5, None, 10, sp, ip, None) == -1 and "bitmap" in _lib.last_error()
    assert lib.vrag_sq8_index_search_filtered(sh._h, qp, 2, 5, None, -1, sp, ip, None) == -1
    assert lib.vrag_sq8_index_search_filtered(sh._h, qp, 2, 5, None, 0, sp, ip, None) == 0 and (i.ravel()[:10] == -1).all()    # an empty mask may be null
    for route in (-1, 3, 100):
        assert lib.vrag_sq8_index_set_route(sh._h, route) == -1 and "route" in _lib.last_error()
    assert lib.vrag_sq8_index_add(sh._h, None, 5) == -1 and lib.vrag_sq8_index_add(sh._h, qp, 0) == -1
    assert lib.vrag_sq8_index_add_device(sh._h, None, 5, None) == -1
    assert lib.vrag_sq8_index_read(sh._h, 0, n + 1, None, None) == -1 and lib.vrag_sq8_index_read(sh._h, -1, 1, None, None) == -1
    big = np.zeros((n + EXTRA + 1, dim), np.float32)
    assert lib.vrag_sq8_index_add(sh._h, big.ctypes.data_as(_FP), len(big)) == -3 and len(sh) == n      # VRAG_ERR_CAPACITY, nothing added
    _same(_search(sh, Q, 5), R.topk(_ref_scores(dim, n)[:2], 5), "after the refusals")
