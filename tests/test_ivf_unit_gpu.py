"""vrag_ivf_index_* through the product ABI (csrc/ivf.hip): assignment against the float64 rule, the anchor (nprobe = nlist is
vrag_dense_index_search_filtered under an all-ones bitmap, bit for bit), the restatement (float64 probe set, then the oracle's
top-k over the union of the probed lists), missing hits, nesting, training, appends and refusals.

Data, centroids and the float64 references: tests/ivf_cases.py (its docstring says why `normal` rows are unit length: the fp32
assignment sums then err by ~1e-7, far under the 1e-5 gap below which a query's probe set may differ from the float64 one).
One index per case, built once and shared by the tests of that case."""
import ctypes as C

import numpy as np
import pytest

import ivf_cases as V
from oracle import topk_ref as T

pytestmark = pytest.mark.gpu

MARGIN, CANARY_F, CANARY_I = 64, np.float32(12345.5), np.int64(-777)
_FP, _LP = C.POINTER(C.c_float), C.POINTER(C.c_int64)
NQS, KS = [1, 17, 100], [1, 10, 64]
_BUILT = {}


def _ids(case):
    return "d%d-n%d-t%d-l%d-%s" % case


def _built(case):
    """(shard, overlay, X, Q, centroids, stored rows, list_off, list_rows) of a case after set_centroids + sync."""
    if case not in _BUILT:
        from verbatim_rag_amd.vector_stores import DenseShard, IvfOverlay

        dim, n, dtype, nlist, kind = case
        X, Q, Cn = V.data(kind, dim, n, nlist)
        sh = DenseShard(dim, n + V.APPENDED, "bf16" if dtype == 0 else "f32", prefilter=dtype == 2)
        sh.add(X[:n])
        ov = IvfOverlay(sh, nlist)
        ov.set_centroids(Cn)
        ov.sync()
        cent, off, rows = ov.read()
        _BUILT[case] = (sh, ov, X, Q, cent, V.stored(X, dtype), off, rows)
    return _BUILT[case]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for sh, *_ in _BUILT.values():
        sh.close()          # closes the overlay first
    _BUILT.clear()


def _search(ov, Q, k, nprobe):
    """The raw call with canary margins around the three result arrays -> (scores, ids, scanned)."""
    from verbatim_rag_amd import _lib

    Q = np.ascontiguousarray(Q, np.float32)
    nq = len(Q)
    s = np.full(nq * k + 2 * MARGIN, CANARY_F, np.float32)
    i = np.full(nq * k + 2 * MARGIN, CANARY_I, np.int64)
    seen = np.full(nq + 2 * MARGIN, CANARY_I, np.int64)
    rc = ov._lib.vrag_ivf_index_search(
        ov._h, Q.ctypes.data_as(_FP), nq, k, nprobe, C.cast(C.c_void_p(s.ctypes.data + 4 * MARGIN), _FP),
        C.cast(C.c_void_p(i.ctypes.data + 8 * MARGIN), _LP), C.cast(C.c_void_p(seen.ctypes.data + 8 * MARGIN), _LP), None)
    assert rc == 0, _lib.last_error()
    for buf, canary, m in ((s, CANARY_F, nq * k), (i, CANARY_I, nq * k), (seen, CANARY_I, nq)):
        assert (buf[:MARGIN] == canary).all() and (buf[MARGIN + m:] == canary).all(), "write outside the result arrays"
    return (s[MARGIN:MARGIN + nq * k].reshape(nq, k).copy(), i[MARGIN:MARGIN + nq * k].reshape(nq, k).copy(),
            seen[MARGIN:MARGIN + nq].copy())


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what


def _ref_over(rows_f32, Q, k, passing):
    """The oracle's top-k over the rows `passing` (ascending), ids mapped back, -1 / -inf tail."""
    kk = min(k, len(passing))
    s = np.full((len(Q), k), -np.inf, np.float32)
    i = np.full((len(Q), k), -1, np.int64)
    if kk:
        ss, ii = T.dense_topk(rows_f32[passing], Q, kk)
        s[:, :kk], i[:, :kk] = ss, passing[ii]
    return s, i


# ---------------------------------------------------------------------------------------------------------------- 1. assignment
@pytest.mark.parametrize("case", V.CASES, ids=_ids)
def test_lists_partition_the_rows_and_follow_the_rule(case):
    dim, n, dtype, nlist, kind = case
    sh, ov, X, Q, cent, rows_f32, off, rows = _built(case)
    assert np.array_equal(cent, V.data(kind, dim, n, nlist)[2]), "centroids do not read back as set"
    assert ov.stats() == {"nlist": nlist, "rows": n, "largest_list": int(np.diff(off.astype(np.int64)).max())}
    assert off[0] == 0 and off[-1] == n and (np.diff(off.astype(np.int64)) >= 0).all()
    assert np.array_equal(np.sort(rows), np.arange(n, dtype=np.uint32)), "the lists do not partition [0, n)"
    got = np.empty(n, np.int64)
    for l in range(nlist):
        seg = rows[off[l]:off[l + 1]]
        assert (np.diff(seg.astype(np.int64)) > 0).all(), f"list {l} is not ascending"
        got[seg] = l
    S = V.list_scores64(rows_f32[:n], cent)
    if kind == "grid":
        assert np.array_equal(got, np.argmax(S, axis=1)), "a row is not in the float64 argmax list (lowest on ties)"
    else:
        bound = dim * 2.0 ** -22 * np.linalg.norm(rows_f32[:n].astype(np.float64), axis=1).max() * np.linalg.norm(cent.astype(np.float64), axis=1).max()
        worst = (S.max(axis=1) - S[np.arange(n), got]).max()
        print(f"{_ids(case)}: worst score deficit of an assigned list {worst:.3e}, bound {bound:.3e}")
        assert worst <= bound
    if nlist >= 7:
        sizes = np.diff(off.astype(np.int64))
        assert sizes[0] == 0 and sizes[1] == 1 and (sizes % 16 != 0).any()


# ---------------------------------------------------------------------------------------------------------------- 2. anchor
@pytest.mark.parametrize("case", V.CASES, ids=_ids)
def test_probing_every_list_is_the_filtered_search_with_every_bit_set(case):
    from verbatim_rag_amd.vector_stores import _bitmap

    dim, n, dtype, nlist, kind = case
    sh, ov, X, Q, *_ = _built(case)
    words = _bitmap(np.ones(n, bool))
    for nq in NQS:
        for k in KS:
            for nprobe in (nlist, nlist + 5):        # clamped to nlist
                s, i, seen = _search(ov, Q[:nq], k, nprobe)
                _same((s, i), sh.search_filtered(Q[:nq], k, words, n), (nq, k, nprobe))
                assert (seen == n).all()


# ---------------------------------------------------------------------------------------------------------------- 3. restatement
@pytest.mark.parametrize("case", [c for c in V.CASES if c[3] > 1], ids=_ids)
def test_fewer_probes_equal_the_oracle_over_the_probed_lists(case):
    dim, n, dtype, nlist, kind = case
    sh, ov, X, Q, cent, rows_f32, off, rows = _built(case)
    j = V.CASES.index(case)
    left_out = total = 0
    for nprobe in (1, 3):
        nq, k = NQS[(j + nprobe) % 3], KS[(j + nprobe // 2) % 3]
        for nq, k in ((nq, k), (100, 10)):
            probe, gap = V.probes64(Q[:nq], cent, nprobe)
            s, i, seen = _search(ov, Q[:nq], k, nprobe)
            for q in range(nq):
                total += 1
                if kind != "grid" and gap[q] < V.GAP:
                    left_out += 1
                    continue
                passing = np.sort(np.concatenate([rows[off[l]:off[l + 1]] for l in probe[q]])).astype(np.int64)
                _same((s[q:q + 1], i[q:q + 1]), _ref_over(rows_f32, Q[q:q + 1], k, passing), (nprobe, nq, k, q))
                assert seen[q] == len(passing), (nprobe, nq, k, q)
    print(f"{_ids(case)}: {left_out} of {total} queries left out")
    assert left_out <= V.LEFT_OUT_MAX * total


# ---------------------------------------------------------------------------------------------------------------- 4. missing hits
@pytest.mark.parametrize("case", [c for c in V.CASES if c[3] >= 7], ids=_ids)
def test_missing_hits(case):
    dim, n, dtype, nlist, kind = case
    sh, ov, X, Q, cent, rows_f32, off, rows = _built(case)
    for k in (1, 10, 64):
        s, i, seen = _search(ov, Q[1:3], k, 1)      # query 1 probes the empty list, query 2 the list of one row
        assert (i[0] == -1).all() and np.isneginf(s[0]).all() and seen[0] == 0
        lone = int(rows[off[1]])
        assert i[1, 0] == lone and seen[1] == 1 and (i[1, 1:] == -1).all() and np.isneginf(s[1, 1:]).all()
        _same((s[1:2], i[1:2]), _ref_over(rows_f32, Q[2:3], k, np.array([lone])), k)
    s, i, seen = _search(ov, Q[1:2], 64, 2)         # the empty list and one more: a sorted head, then the tail
    m = int(seen[0])
    head = min(m, 64)
    assert (i[0, :head] >= 0).all() and (i[0, head:] == -1).all() and np.isneginf(s[0, head:]).all()
    assert (np.diff(s[0, :head]) <= 0).all()


# ---------------------------------------------------------------------------------------------------------------- 5. nesting
@pytest.mark.parametrize("case", [c for c in V.CASES if c[3] > 1], ids=_ids)
def test_kth_score_never_drops_as_nprobe_grows(case):
    dim, n, dtype, nlist, kind = case
    sh, ov, X, Q, *_ = _built(case)
    for k in KS:
        kth = [_search(ov, Q, k, nprobe)[0][:, k - 1] for nprobe in (1, 3, nlist)]
        assert (kth[0] <= kth[1]).all() and (kth[1] <= kth[2]).all(), k


# ---------------------------------------------------------------------------------------------------------------- 6. training
def _trained(dim, n, dtype, nlist, X, iters, max_rows):
    from verbatim_rag_amd.vector_stores import DenseShard, IvfOverlay

    sh = DenseShard(dim, n, "bf16" if dtype == 0 else "f32", prefilter=dtype == 2)
    try:
        sh.add(X)
        out = []
        for _ in range(2):
            ov = IvfOverlay(sh, nlist)
            ov.train(iters, max_rows)
            ov.sync()
            out.append(ov.read())
            ov.close()
        return out
    finally:
        sh.close()


@pytest.mark.parametrize("dim,n,dtype,nlist,max_rows", V.TRAIN_CASES)
def test_training_is_reproducible_and_lists_are_pure(dim, n, dtype, nlist, max_rows):
    X, label = V.clusters(dim, n)
    a, b = _trained(dim, n, dtype, nlist, X, 10, max_rows)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two trainings of the same rows differ"
    cent, off, rows = a
    assert off[-1] == n and np.array_equal(np.sort(rows), np.arange(n, dtype=np.uint32))
    for l in range(nlist):
        assert len(np.unique(label[rows[off[l]:off[l + 1]]])) <= 1, f"list {l} holds rows of more than one cluster"
    if nlist == 16:   # one list per cluster, all rows in the sample: converged after the first round, so the lists ARE the members
        rows_f32 = V.stored(X, dtype).astype(np.float64)
        assert (np.diff(off.astype(np.int64)) > 0).all()
        for l in range(nlist):
            mem = rows[off[l]:off[l + 1]]
            tol = (len(mem) + 1) * 2.0 ** -24 * np.abs(rows_f32[mem]).max()
            err = np.abs(cent[l].astype(np.float64) - rows_f32[mem].mean(axis=0)).max()
            assert err <= tol, (l, err, tol)


def test_initial_centroids_and_the_first_update():
    """iters = 0 leaves the evenly strided sample rows; one round on grid rows (exact scores, exact sums) gives the float64 means of
    the float64 assignment to those rows, an empty list keeping its centroid."""
    dim, n, nlist = 64, 3001, 7
    X = V.data("grid", dim, n, nlist)[0][:n]
    for max_rows, n_train in ((1 << 40, n), (1000, 1000)):
        sample, first = V.training_rows(n, max_rows, nlist)
        assert len(sample) == n_train
        (c0, _o, _r), _ = _trained(dim, n, 1, nlist, X, 0, max_rows)
        assert np.array_equal(c0, X[first])
        (c1, off, rows), _ = _trained(dim, n, 1, nlist, X, 1, max_rows)
        a = V.assign64(X[sample], c0)
        for l in range(nlist):
            mem = sample[a == l]
            want = X[mem].astype(np.float64).mean(axis=0) if len(mem) else c0[l].astype(np.float64)
            assert np.abs(c1[l].astype(np.float64) - want).max() <= (len(mem) + 1) * 2.0 ** -24 * 0.5, l
        # the lists are the rule under the updated centroids (no longer on the grid: held to the fp32 accumulation bound)
        got = np.empty(n, np.int64)
        for l in range(nlist):
            got[rows[off[l]:off[l + 1]]] = l
        S = V.list_scores64(X, c1)
        bound = dim * 2.0 ** -22 * np.linalg.norm(X.astype(np.float64), axis=1).max() * np.linalg.norm(c1.astype(np.float64), axis=1).max()
        assert (S.max(axis=1) - S[np.arange(n), got]).max() <= bound


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_first_update_at_768_columns(dtype):
    """The mean bound on every non-empty list where a thread of the update owns three columns (768 = 3 x 256), on bf16, fp32 and
    prefilter shards: one round over all rows of a grid corpus, members = the float64 assignment to the initial centroids."""
    dim, n, nlist = 768, 3001, 64
    X = V.data("grid", dim, n, nlist)[0][:n]
    sample, first = V.training_rows(n, 1 << 40, nlist)
    (c1, _off, _rows), _ = _trained(dim, n, dtype, nlist, X, 1, 1 << 40)
    a = V.assign64(X, X[first])
    assert len(np.unique(a)) > nlist // 2
    for l in range(nlist):
        mem = sample[a == l]
        want = X[mem].astype(np.float64).mean(axis=0) if len(mem) else X[first[l]].astype(np.float64)
        assert np.abs(c1[l].astype(np.float64) - want).max() <= (len(mem) + 1) * 2.0 ** -24 * 0.5, l


# ---------------------------------------------------------------------------------------------------------------- 7. appends
@pytest.mark.parametrize("case", [V.CASES[1], V.CASES[6]], ids=_ids)
def test_rows_added_after_a_sync_wait_for_the_next_one(case):
    from verbatim_rag_amd.vector_stores import _bitmap

    dim, n, dtype, nlist, kind = case
    sh, ov, X, Q, *_ = _built(case)
    before = _search(ov, Q[:17], 10, nlist)
    sh.add(X[n:])
    try:
        after = _search(ov, Q[:17], 10, nlist)
        _same(after[:2], before[:2], "rows appended to the base showed up before a sync")
        assert (after[1] < n).all() and (after[2] == n).all()
        ov.sync()
        assert ov.stats()["rows"] == n + V.APPENDED
        s, i, seen = _search(ov, Q[:17], 10, nlist)
        assert (i[0] >= n).all() and (seen == n + V.APPENDED).all()       # the appended rows lead query 0's ranking
        _same((s, i), sh.search_filtered(Q[:17], 10, _bitmap(np.ones(n + V.APPENDED, bool)), n + V.APPENDED), "after the sync")
    finally:
        _BUILT.pop(case)[0].close()     # the case's index has grown: the next user builds it afresh


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_leave_the_handle_usable():
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.vector_stores import DenseShard, IvfOverlay

    lib = _lib.load()
    X, Q, Cn = V.data("grid", 64, 257, 7)
    sh = DenseShard(64, 300, "f32")
    try:
        sh.add(X[:257])
        for nlist in (0, 16385):
            h = C.c_void_p()
            assert lib.vrag_ivf_index_create(sh._h, nlist, C.byref(h)) == -1 and not h.value and "nlist" in _lib.last_error()
        h = C.c_void_p()
        assert lib.vrag_ivf_index_create(None, 7, C.byref(h)) == -1 and not h.value
        ov = IvfOverlay(sh, 7)
        q = np.ascontiguousarray(Q[:2])
        s, i = np.empty((2, 64), np.float32), np.empty((2, 64), np.int64)

        def call(queries, k, nprobe=3):
            return lib.vrag_ivf_index_search(ov._h, queries, 2, k, nprobe, s.ctypes.data_as(_FP), i.ctypes.data_as(_LP), None, None)

        assert lib.vrag_ivf_index_sync(ov._h) == -1 and "centroids" in _lib.last_error()
        ov.set_centroids(Cn)
        assert call(q.ctypes.data_as(_FP), 5) == -1 and "sync" in _lib.last_error()      # search before any sync
        ov.sync()
        for k in (0, 65):
            assert call(q.ctypes.data_as(_FP), k) == -1 and "k must be" in _lib.last_error()
        assert call(None, 5) == -1 and _lib.last_error()
        assert call(q.ctypes.data_as(_FP), 5, 0) == -1 and "nprobe" in _lib.last_error()
        assert lib.vrag_ivf_index_search(ov._h, q.ctypes.data_as(_FP), 2, 5, 3, None, i.ctypes.data_as(_LP), None, None) == -1
        assert lib.vrag_ivf_index_train(ov._h, -1, 100) == -1 and lib.vrag_ivf_index_train(ov._h, 3, 0) == -1
        got = ov.search(q, 5, 7)                                                         # and the handle still answers
        from verbatim_rag_amd.vector_stores import _bitmap

        _same(got, sh.search_filtered(q, 5, _bitmap(np.ones(257, bool)), 257), "after the refusals")
    finally:
        sh.close()
