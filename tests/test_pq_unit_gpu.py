"""vrag_pq_index_* through the product ABI (csrc/pq.hip) against tests/pq_ref.py, bit for bit: the stored codes, the search and
the filtered search, appends, compaction, the deterministic training and every refusal of the contract.

Codebooks are SET (Gaussian, with two identical centroids in sub-space 0, which a block of rows sits on exactly: the lower code
wins), not trained.  Data: Gaussian rows and queries with per-vector magnitudes spread over 1e-3 .. 1e3, a block of exact
duplicate rows that one query points along (ties -> id asc at the head of its list), a few all-zero rows and one all-zero query
(every score +0: the whole list is id asc).  One index and one reference score matrix per (dim, m, n), built once and shared."""
import ctypes as C

import numpy as np
import pytest

import pq_ref as R

pytestmark = pytest.mark.gpu

MARGIN, CANARY_F, CANARY_I = 64, np.float32(12345.5), np.int64(-777)
_FP, _LP = C.POINTER(C.c_float), C.POINTER(C.c_int64)
NQ_MAX, EXTRA = 65, 40           # queries per data set; append room of every index
ZERO_Q, DUP_Q = 3, 1             # the all-zero query; the query along the duplicated row
TWIN_LO, TWIN_HI = 7, 200        # the two identical centroids of sub-space 0

# the launch constants of csrc/pq.hip that decide how many steps a workgroup of the scan takes
PQ_THREADS, PQ_R, PQ_SLICE, PQ_WAVES, KMAX, LDS_BUDGET, WGS_PER_CU_MAX = 1024, 4, 64, 16, 64, 160 * 1024, 2
PQ_WG_STEP = PQ_THREADS * PQ_R
BIG = (24, 3, 40003)             # every workgroup of its 64-query launch takes more than one step (asserted below)

# (dim, m, n, ((nq, k), ...)): every (dim, m) of the contract's list, n of {1, 63, 64, 65, 257, 4097} and BIG, nq of {1, 5, 17, 65}
# (65 = a slice of 64 and one of 1), k of {1, 10, 64, 65, 200}: (.., 64, .., k 65) a first page exactly full and an empty second,
# k 200 on 257 rows four pages with the last one short, on 63 rows an exhausted first page
CASES = [
    (24, 3, 1, ((1, 1), (5, 10), (17, 65))),
    (24, 3, 64, ((5, 65), (65, 64), (1, 200))),
    (24, 1, 4097, ((65, 10), (17, 200), (1, 64))),
    (64, 64, 257, ((17, 10), (65, 200), (5, 1))),
    (64, 16, 4097, ((65, 65), (5, 64), (1, 10))),
    (136, 17, 65, ((65, 10), (5, 200), (17, 64))),
    (136, 17, 63, ((1, 1), (17, 200))),
    (384, 48, 257, ((5, 10), (65, 65))),
    (768, 96, 257, ((1, 10), (17, 64), (65, 200))),
    (768, 128, 257, ((65, 10), (5, 65), (1, 1))),
    (*BIG, ((64, 10), (65, 65), (1, 200))),
]
_DATA, _BUILT, _REF = {}, {}, {}


def _ids(case):
    return "d%d-m%d-n%d" % case[:3]


def _codebooks(dim, m):
    rng = np.random.default_rng(7 * dim + m)
    cb = rng.standard_normal((m, 256, dim // m)).astype(np.float32)
    cb[0, TWIN_HI] = cb[0, TWIN_LO]
    return cb


def _data(dim, m, n):
    """(rows [n + EXTRA, dim], queries [NQ_MAX, dim], codebooks) fp32; rows [n, n + EXTRA) are the append room's."""
    key = (dim, m, n)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * dim + 10 * m + n)
        cb = _codebooks(dim, m)
        X = (rng.standard_normal((n + EXTRA, dim)) * 10.0 ** rng.uniform(-3, 3, (n + EXTRA, 1))).astype(np.float32)
        Q = (rng.standard_normal((NQ_MAX, dim)) * 10.0 ** rng.uniform(-3, 3, (NQ_MAX, 1))).astype(np.float32)
        if n >= 63:
            X[40:49] = X[40] / np.linalg.norm(X[40]) * np.float32(1e3)      # nine copies: ties at the head of DUP_Q's list
            X[[5, 17, n - 1]] = 0.0                  # all-zero rows, the last row among them
            X[50:56, :dim // m] = cb[0, TWIN_HI]     # sub-vector 0 ON the twin centroids: a(7) == a(200) exactly
            Q[DUP_Q] = X[40] * np.float32(0.5)
        Q[ZERO_Q] = 0.0
        _DATA[key] = (X, Q, cb)
    return _DATA[key]


def _ref(dim, m, n):
    """(reference codes [n, m], reference scores [NQ_MAX, n]) of the data set, computed once."""
    key = (dim, m, n)
    if key not in _REF:
        X, Q, cb = _data(dim, m, n)
        codes = R.encode(X[:n], cb)
        _REF[key] = (codes, R.scores(R.lut(Q, cb), codes))
    return _REF[key]


def _new(dim, m, capacity, cb=None):
    from verbatim_rag_amd.vector_stores import PqShard

    sh = PqShard(dim, m, capacity)
    if cb is not None:
        sh.set_codebooks(cb)
    return sh


def _built(dim, m, n):
    key = (dim, m, n)
    if key not in _BUILT:
        X, _Q, cb = _data(dim, m, n)
        sh = _new(dim, m, n + EXTRA, cb)
        sh.add(X[:n])
        _BUILT[key] = sh
    return _BUILT[key]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for sh in _BUILT.values():
        sh.close()
    _BUILT.clear()
    _DATA.clear()
    _REF.clear()


def _search(sh, Q, k, allow=None, n_allow=0):
    """The raw call with canary margins around the two result arrays -> (scores, ids)."""
    from verbatim_rag_amd import _lib

    Q = np.ascontiguousarray(Q, np.float32)
    nq = len(Q)
    s = np.full(nq * k + 2 * MARGIN, CANARY_F, np.float32)
    i = np.full(nq * k + 2 * MARGIN, CANARY_I, np.int64)
    sp, ip = C.cast(C.c_void_p(s.ctypes.data + 4 * MARGIN), _FP), C.cast(C.c_void_p(i.ctypes.data + 8 * MARGIN), _LP)
    if allow is None:
        rc = sh._lib.vrag_pq_index_search(sh._h, Q.ctypes.data_as(_FP), nq, k, sp, ip, None)
    else:
        words = np.ascontiguousarray(allow, np.uint32)
        rc = sh._lib.vrag_pq_index_search_filtered(sh._h, Q.ctypes.data_as(_FP), nq, k, words.ctypes.data, n_allow, sp, ip, None)
    assert rc == 0, _lib.last_error()
    for buf, canary in ((s, CANARY_F), (i, CANARY_I)):
        assert (buf[:MARGIN] == canary).all() and (buf[MARGIN + nq * k:] == canary).all(), "write outside the result arrays"
    return s[MARGIN:MARGIN + nq * k].reshape(nq, k).copy(), i[MARGIN:MARGIN + nq * k].reshape(nq, k).copy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what


def _read_canaried(sh, first, n):
    """vrag_pq_index_read with canary margins around the codes."""
    from verbatim_rag_amd import _lib

    buf = np.full(n * sh.m + 2 * MARGIN, 0xA5, np.uint8)
    rc = sh._lib.vrag_pq_index_read(sh._h, first, n, C.c_void_p(buf.ctypes.data + MARGIN))
    assert rc == 0, _lib.last_error()
    assert (buf[:MARGIN] == 0xA5).all() and (buf[MARGIN + n * sh.m:] == 0xA5).all(), "write outside the codes"
    return buf[MARGIN:MARGIN + n * sh.m].reshape(n, sh.m).copy()


# ---------------------------------------------------------------------------------------------------------------- 1. the stored codes
@pytest.mark.parametrize("dim,m", [(24, 3), (24, 1), (64, 64), (64, 16), (136, 17), (384, 48), (768, 96), (768, 128)])
def test_read_returns_the_rule_after_every_kind_of_append(dim, m):
    import torch

    X, _Q, cb = _data(dim, m, 257)
    codes = R.encode(X, cb)
    assert (codes[50:56, 0] == TWIN_LO).all() and not (codes[:, 0] == TWIN_HI).any(), "identical centroids resolve to the lower code"
    sh = _new(dim, m, len(X), cb)
    try:
        assert len(sh) == 0 and np.array_equal(sh.codebooks().view(np.uint32), cb.view(np.uint32))
        sh.add(X[:100])
        assert len(sh) == 100 and np.array_equal(_read_canaried(sh, 0, 100), codes[:100])
        t = torch.from_numpy(X[100:257]).cuda()
        sh.add_device(t.data_ptr(), 157)
        assert len(sh) == 257 and np.array_equal(sh.read(), codes[:257])
        sh.add(X[257:])                              # a second host append
        assert len(sh) == len(X) and np.array_equal(sh.read(), codes)
        assert np.array_equal(_read_canaried(sh, 250, 20), codes[250:270])       # a window
    finally:
        sh.close()


# ---------------------------------------------------------------------------------------------------------------- 2. search
def _scan_plan(m, n, nqs, n_cu):
    """(row ranges, rows per range) of one scan launch: pq_scan_ranges of csrc/pq.hip."""
    lds = m * 1024 + PQ_WAVES * KMAX * 8
    wgs_per_cu = max(1, min(WGS_PER_CU_MAX, LDS_BUDGET // lds))
    n_wg = min(max(1, -(-n_cu * wgs_per_cu // nqs)), -(-n // PQ_THREADS))
    return n_wg, -(-n // n_wg)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_search_equals_the_reference(case):
    dim, m, n, searches = case
    sh, Q = _built(dim, m, n), _data(dim, m, n)[1]
    codes, S = _ref(dim, m, n)
    assert np.array_equal(sh.read(), codes)
    if case[:3] == BIG:
        import torch

        n_wg, per = _scan_plan(m, n, 64, torch.cuda.get_device_properties(0).multi_processor_count)
        assert n_wg > 1 and per > PQ_WG_STEP, "every workgroup of the 64-query launch takes more than one step of its main loop"
    for nq, k in searches:
        want = R.topk(S[:nq], k)
        _same(_search(sh, Q[:nq], k), want, (case[:3], nq, k))
        if n >= 63 and nq > ZERO_Q:
            assert np.array_equal(want[1][ZERO_Q, :min(k, n)], np.arange(min(k, n))), "the all-zero query's list is id asc"
        if n >= 63 and nq > DUP_Q:
            assert len(set(S[DUP_Q, 40:49].view(np.uint32).tolist())) == 1, "the duplicated rows tie exactly"
            copies = [r for r in want[1][DUP_Q].tolist() if 40 <= r < 49]
            assert copies == list(range(40, 40 + len(copies))), "ties come back id asc"


@pytest.mark.parametrize("k", [5, 65])
def test_an_empty_index_answers_no_hits(k):
    X, Q, cb = _data(64, 16, 257)
    sh = _new(64, 16, 16, cb)
    try:
        s, i = _search(sh, Q[:3], k)
        assert len(sh) == 0 and (i == -1).all() and np.isneginf(s).all()
    finally:
        sh.close()


# ---------------------------------------------------------------------------------------------------------------- 3. filtered search
@pytest.mark.parametrize("dim,m,n,nq,k", [(24, 3, 64, 5, 65), (64, 16, 4097, 17, 10), (768, 96, 257, 5, 200), (136, 17, 65, 65, 10),
                                          (*BIG, 65, 10)])
def test_filtered_search_equals_the_reference_over_the_passing_rows(dim, m, n, nq, k):
    from verbatim_rag_amd.vector_stores import _bitmap

    sh, Q, S = _built(dim, m, n), _data(dim, m, n)[1][:nq], _ref(dim, m, n)[1][:nq]
    rng = np.random.default_rng(n)
    random = rng.random(n) < 0.3
    single = np.zeros(n, bool)
    single[n // 2] = True
    _same(_search(sh, Q, k, _bitmap(np.ones(n, bool)), n), _search(sh, Q, k), "all ones")
    for name, mask in (("random", random), ("single", single)):
        _same(_search(sh, Q, k, _bitmap(mask), n), R.topk(S, k, np.nonzero(mask)[0]), name)
    short = n - n // 4                               # a mask shorter than the index: rows at or beyond it do not pass
    _same(_search(sh, Q, k, _bitmap(np.ones(n, bool)), short), R.topk(S, k, np.arange(short)), "n_allow < size")
    _same(_search(sh, Q, k, _bitmap(random), short), R.topk(S, k, np.nonzero(random[:short])[0]), "n_allow < size, random")
    for words, n_allow in ((_bitmap(np.zeros(n, bool)), n), (np.zeros(1, np.uint32), 0), (_bitmap(np.ones(n, bool)), 0)):
        s, i = _search(sh, Q, k, words, n_allow)
        assert (i == -1).all() and np.isneginf(s).all(), "none"


# ---------------------------------------------------------------------------------------------------------------- 4. appends, compaction
@pytest.mark.parametrize("dim,m,n", [(64, 16, 257), (768, 96, 257)])
def test_a_search_right_after_an_append_sees_exactly_size_rows(dim, m, n):
    X, Q, cb = _data(dim, m, n)
    sh = _built(dim, m, n)
    try:
        _same(_search(sh, Q[:30], 10), R.topk(_ref(dim, m, n)[1][:30], 10), "before")
        sh.add(X[n:])
        assert len(sh) == n + EXTRA
        codes = R.encode(X, cb)
        assert np.array_equal(sh.read(), codes)
        _same(_search(sh, Q[:30], 10), R.topk(R.scores(R.lut(Q[:30], cb), codes), 10), "after")
    finally:
        _BUILT.pop((dim, m, n)).close()              # the index has grown: the next user builds it afresh


@pytest.mark.parametrize("dim,m,n", [(136, 17, 65), (64, 16, 4097)])
def test_compact_keeps_the_codes_and_the_lists_of_the_kept_rows(dim, m, n):
    X, Q, cb = _data(dim, m, n)
    codes, S = _ref(dim, m, n)
    rng = np.random.default_rng(3)
    keep = rng.random(n) < 0.6
    keep[0], keep[n - 1] = False, True
    kept = np.nonzero(keep)[0]
    sh = _built(dim, m, n)
    try:
        assert sh.compact(keep) == len(kept) == len(sh)
        assert np.array_equal(_read_canaried(sh, 0, len(kept)), codes[kept])
        assert np.array_equal(sh.codebooks().view(np.uint32), cb.view(np.uint32))
        for nq, k in ((17, 10), (5, 65)):
            want_s, want_i = R.topk(S[:nq], k, kept)                     # ids of the old numbering -> ranks among the kept rows
            new_id = np.where(want_i >= 0, np.searchsorted(kept, np.maximum(want_i, 0)), -1)
            _same(_search(sh, Q[:nq], k), (want_s, new_id), ("after compact", nq, k))
        assert sh.compact(np.ones(len(kept), bool)) == len(kept)         # nothing to drop
        sh.add(X[n:n + 5])                                               # appends go behind the compacted rows
        assert np.array_equal(sh.read(len(kept), 5), R.encode(X[n:n + 5], cb))
    finally:
        _BUILT.pop((dim, m, n)).close()


# ---------------------------------------------------------------------------------------------------------------- 5. training
def _clustered(rng, n, dim, centres):
    c = rng.standard_normal((centres, dim)).astype(np.float32)
    return (c[rng.integers(0, centres, n)] + 0.05 * rng.standard_normal((n, dim))).astype(np.float32)


def test_training_equals_the_numpy_restatement_and_repeats():
    dim, m, n, iters = 24, 3, 2000, 3
    X = _clustered(np.random.default_rng(11), n, dim, 300)
    want = R.train(X, m, iters)
    a, b = _new(dim, m, 16), _new(dim, m, 16)
    try:
        a.train(X, iters)
        b.train(X, iters)
        got = a.codebooks()
        assert np.array_equal(got.view(np.uint32), b.codebooks().view(np.uint32)), "two trainings of the same rows"
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the numpy restatement"
        a.train(X, 0)                                # no round: the initial centroids, sample rows c * n // 256
        assert np.array_equal(a.codebooks(), R.split(X, m)[:, (np.arange(256) * n) // 256, :])
    finally:
        a.close()
        b.close()


def test_training_lowers_the_distortion_of_clustered_rows():
    dim, m, n = 32, 4, 3000
    X = _clustered(np.random.default_rng(12), n, dim, 400)
    err = []
    for iters in (0, 5):
        sh = _new(dim, m, n)
        try:
            sh.train(X, iters)
            sh.add(X)
            approx = R.decode(sh.read(), sh.codebooks())
            err.append(float(((X.astype(np.float64) - approx.astype(np.float64)) ** 2).sum(axis=1).mean()))
        finally:
            sh.close()
    print(f"distortion after 0 rounds {err[0]:.5f}, after 5 rounds {err[1]:.5f}")
    assert err[1] < err[0]


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_handle_usable():
    from verbatim_rag_amd import _lib

    lib = _lib.load()
    for dim, m, word in ((0, 1, "dim"), (4097, 1, "dim"), (-8, 1, "dim"), (64, 0, "m must"), (64, 129, "m must"), (64, 5, "divide"),
                         (4096, 32, "sub-vector"), (130, 2, "sub-vector")):
        h = C.c_void_p()
        assert lib.vrag_pq_index_create(dim, m, 100, 0, C.byref(h)) == -1 and not h.value and word in _lib.last_error(), (dim, m)
    h = C.c_void_p()
    for cap in (0, -1, 0xFFFFFFFF):
        assert lib.vrag_pq_index_create(64, 16, cap, 0, C.byref(h)) == -1 and not h.value
    assert lib.vrag_pq_index_create(64, 16, 100, -1, C.byref(h)) == -1 and not h.value
    assert lib.vrag_pq_index_create(64, 16, 100, 0, None) == -1
    assert lib.vrag_pq_index_size(None) == -1
    dim, m, n = 64, 16, 257
    X, Q, cb = _data(dim, m, n)
    Q2 = np.ascontiguousarray(Q[:2])
    s, i = np.empty((2, 1025), np.float32), np.empty((2, 1025), np.int64)
    qp, sp, ip = Q2.ctypes.data_as(_FP), s.ctypes.data_as(_FP), i.ctypes.data_as(_LP)
    xp, cbp = X.ctypes.data_as(_FP), cb.ctypes.data_as(_FP)

    # before codebooks exist: no rows, no searches, nothing to read back
    raw = _new(dim, m, 100)
    try:
        assert lib.vrag_pq_index_add(raw._h, xp, 5) == -1 and "codebooks" in _lib.last_error()
        assert lib.vrag_pq_index_add_device(raw._h, C.c_void_p(16), 5, None) == -1 and "codebooks" in _lib.last_error()
        assert lib.vrag_pq_index_search(raw._h, qp, 2, 5, sp, ip, None) == -1 and "codebooks" in _lib.last_error()
        assert lib.vrag_pq_index_search_filtered(raw._h, qp, 2, 5, None, 0, sp, ip, None) == -1 and "codebooks" in _lib.last_error()
        assert lib.vrag_pq_index_read_codebooks(raw._h, cbp) == -1
        assert lib.vrag_pq_index_set_codebooks(raw._h, None) == -1 and lib.vrag_pq_index_set_codebooks(None, cbp) == -1
        for args in ((raw._h, None, 10, 1), (raw._h, xp, 0, 1), (raw._h, xp, 10, -1), (raw._h, xp, 10, 1001), (None, xp, 10, 1)):
            assert lib.vrag_pq_index_train(*args) == -1 and _lib.last_error()
        assert len(raw) == 0
    finally:
        raw.close()

    sh = _built(dim, m, n)
    for k in (0, 1025, -1):
        assert lib.vrag_pq_index_search(sh._h, qp, 2, k, sp, ip, None) == -1 and "k must be" in _lib.last_error()
        assert lib.vrag_pq_index_search_filtered(sh._h, qp, 2, k, None, 0, sp, ip, None) == -1 and "k must be" in _lib.last_error()
    assert lib.vrag_pq_index_search(sh._h, qp, 0, 5, sp, ip, None) == -1
    for args in ((None, qp, 2, 5, sp, ip, None), (sh._h, None, 2, 5, sp, ip, None), (sh._h, qp, 2, 5, None, ip, None), (sh._h, qp, 2, 5, sp, None, None)):
        assert lib.vrag_pq_index_search(*args) == -1 and _lib.last_error()
    assert lib.vrag_pq_index_search_filtered(sh._h, qp, 2, 5, None, 10, sp, ip, None) == -1 and "bitmap" in _lib.last_error()
    assert lib.vrag_pq_index_search_filtered(sh._h, qp, 2, 5, None, -1, sp, ip, None) == -1
    assert lib.vrag_pq_index_search_filtered(sh._h, qp, 2, 5, None, 0, sp, ip, None) == 0 and (i.ravel()[:10] == -1).all()    # an empty mask may be null
    # the codebooks are frozen once the index holds rows
    assert lib.vrag_pq_index_set_codebooks(sh._h, cbp) == -1 and "frozen" in _lib.last_error()
    assert lib.vrag_pq_index_train(sh._h, xp, 100, 1) == -1 and "frozen" in _lib.last_error()
    assert lib.vrag_pq_index_add(sh._h, None, 5) == -1 and lib.vrag_pq_index_add(sh._h, qp, 0) == -1
    assert lib.vrag_pq_index_add_device(sh._h, None, 5, None) == -1
    codes = np.empty((n + 1, m), np.uint8)
    assert lib.vrag_pq_index_read(sh._h, 0, n + 1, codes.ctypes.data) == -1 and lib.vrag_pq_index_read(sh._h, -1, 1, codes.ctypes.data) == -1
    assert lib.vrag_pq_index_read(sh._h, 0, 1, None) == -1
    new_size = C.c_int64(-5)
    words = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    assert lib.vrag_pq_index_compact(sh._h, words.ctypes.data, n - 1, C.byref(new_size)) == -1       # the bitmap covers exactly the rows
    assert lib.vrag_pq_index_compact(sh._h, words.ctypes.data, n, None) == -1
    big = np.zeros((n + EXTRA + 1, dim), np.float32)
    assert lib.vrag_pq_index_add(sh._h, big.ctypes.data_as(_FP), len(big)) == -3 and len(sh) == n      # VRAG_ERR_CAPACITY, nothing added
    _same(_search(sh, Q2, 5), R.topk(_ref(dim, m, n)[1][:2], 5), "after the refusals")
