"""vrag_ivf_index_* over an SQ8 base through the product ABI (csrc/ivf.hip, csrc/ivf_sq8.hip): assignment against the float64
rule over x^, the anchor (nprobe = nlist is vrag_sq8_index_search on either route and tests/sq8_ref.py, bit for bit), the restatement
(float64 probe set, then sq8_ref's top-k over the union of the probed lists), missing hits, nesting, training, appends, compaction,
refusals and one call through the query slices.

Data, centroids and references: tests/ivf_sq8_cases.py.  One index per case, built once and shared by the tests of that case.
Not tested: the refusal of "a base other than the one the overlay was created on" -- the overlay keeps its base's handle, so the ABI
offers no way to hand it another one short of destroying the base under it."""
import ctypes as C

import numpy as np
import pytest

import ivf_cases as V
import ivf_sq8_cases as S
import sq8_ref as R

pytestmark = pytest.mark.gpu

MARGIN, CANARY_F, CANARY_I = 64, np.float32(12345.5), np.int64(-777)
_FP, _LP = C.POINTER(C.c_float), C.POINTER(C.c_int64)
NQS, KS = [1, 17, 100], [1, 10, 64]
_BUILT = {}


def _ids(case):
    return "d%d-n%d-l%d-%s-j%d" % case


def _built(case):
    """(shard, overlay, Q, centroids, x^ of the stored rows, list_off, list_rows) of a case after set_centroids + sync."""
    if case not in _BUILT:
        from verbatim_rag_amd.vector_stores import IvfOverlay, Sq8Shard

        dim, n, nlist, kind, j = case
        X, Q, Cn = S.data(kind, dim, n, nlist, j)
        sh = Sq8Shard(dim, n + S.APPENDED)
        sh.add(X[:n])
        ov = IvfOverlay(sh, nlist)
        ov.set_centroids(Cn)
        ov.sync()
        cent, off, rows = ov.read()
        _BUILT[case] = (sh, ov, Q, cent, S.dequantized(*sh.read()), off, rows)
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


def _lists(off, rows, n):
    """list of every row from (list_off, list_rows); asserts the partition and the ascending order."""
    assert off[0] == 0 and off[-1] == n and (np.diff(off.astype(np.int64)) >= 0).all()
    assert np.array_equal(np.sort(rows), np.arange(n, dtype=np.uint32)), "the lists do not partition [0, n)"
    got = np.empty(n, np.int64)
    for l in range(len(off) - 1):
        seg = rows[off[l]:off[l + 1]]
        assert (np.diff(seg.astype(np.int64)) > 0).all(), f"list {l} is not ascending"
        got[seg] = l
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. assignment
@pytest.mark.parametrize("case", S.CASES, ids=_ids)
def test_lists_partition_the_rows_and_follow_the_rule_over_dequantised_rows(case):
    dim, n, nlist, kind, j = case
    sh, ov, Q, cent, xhat, off, rows = _built(case)
    assert np.array_equal(cent, S.data(kind, dim, n, nlist, j)[2]), "centroids do not read back as set"
    assert np.array_equal(xhat, S.reference(case)[2][:n]), "the stored rows are not the rule's"
    assert ov.stats() == {"nlist": nlist, "rows": n, "largest_list": int(np.diff(off.astype(np.int64)).max())}
    got = _lists(off, rows, n)
    L = V.list_scores64(xhat, cent)
    want = np.argmax(L, axis=1)
    if kind == "integer":
        assert np.array_equal(got, want), "a row is not in the float64 argmax list (lowest on ties)"
    else:
        other = np.nonzero(got != want)[0]
        deficit = L[other, want[other]] - L[other, got[other]]
        print(f"{_ids(case)}: {len(other)} of {n} rows assigned otherwise, worst float64 gap {deficit.max() if len(other) else 0.0:.3e}")
        assert (deficit < S.GAP).all() and len(other) <= S.ROWS_LEFT_OUT_MAX * n
    if nlist >= 7:
        sizes = np.diff(off.astype(np.int64))
        assert sizes[0] == 0 and sizes[1] == 1 and (sizes % 16 != 0).any()


# ---------------------------------------------------------------------------------------------------------------- 2. anchor
@pytest.mark.parametrize("case", S.CASES, ids=_ids)
def test_probing_every_list_is_the_flat_sq8_search(case):
    dim, n, nlist, kind, j = case
    sh, ov, Q, *_ = _built(case)
    scores = S.reference(case)[3][:, :n]
    try:
        for nq in NQS:
            for k in KS:
                want = R.topk(scores[:nq], k)
                for nprobe in (nlist, nlist + 5):        # clamped to nlist
                    s, i, seen = _search(ov, Q[:nq], k, nprobe)
                    _same((s, i), want, (nq, k, nprobe, "sq8_ref"))
                    assert (seen == n).all()
                for route in (1, 2):
                    sh.set_route(route)
                    _same((s, i), sh.search(Q[:nq], k), (nq, k, "route", route))
    finally:
        sh.set_route(0)


# ---------------------------------------------------------------------------------------------------------------- 3. restatement
@pytest.mark.parametrize("case", [c for c in S.CASES if c[2] > 1], ids=_ids)
def test_fewer_probes_equal_the_reference_over_the_probed_lists(case):
    dim, n, nlist, kind, j = case
    sh, ov, Q, cent, xhat, off, rows = _built(case)
    scores = S.reference(case)[3][:, :n]
    jj = S.CASES.index(case)
    left_out = total = 0
    for nprobe in (1, 3):
        nq, k = NQS[(jj + nprobe) % 3], KS[(jj + nprobe // 2) % 3]
        for nq, k in ((nq, k), (100, 10)):
            probe, gap = V.probes64(Q[:nq], cent, nprobe)
            s, i, seen = _search(ov, Q[:nq], k, nprobe)
            for q in range(nq):
                total += 1
                if kind != "integer" and gap[q] < S.GAP:
                    left_out += 1
                    continue
                passing = np.sort(np.concatenate([rows[off[l]:off[l + 1]] for l in probe[q]])).astype(np.int64)
                _same((s[q:q + 1], i[q:q + 1]), R.topk(scores[q:q + 1], k, passing), (nprobe, nq, k, q))
                assert seen[q] == len(passing), (nprobe, nq, k, q)
    print(f"{_ids(case)}: {left_out} of {total} queries left out")
    assert left_out <= S.QUERIES_LEFT_OUT_MAX * total and (kind != "integer" or left_out == 0)


# ---------------------------------------------------------------------------------------------------------------- 4. missing hits
@pytest.mark.parametrize("case", [c for c in S.CASES if c[2] >= 7], ids=_ids)
def test_missing_hits(case):
    dim, n, nlist, kind, j = case
    sh, ov, Q, cent, xhat, off, rows = _built(case)
    scores = S.reference(case)[3][:, :n]
    for k in (1, 10, 64):
        s, i, seen = _search(ov, Q[1:3], k, 1)      # query 1 probes the empty list, query 2 the list of one row
        assert (i[0] == -1).all() and np.isneginf(s[0]).all() and seen[0] == 0
        lone = int(rows[off[1]])
        assert i[1, 0] == lone and seen[1] == 1 and (i[1, 1:] == -1).all() and np.isneginf(s[1, 1:]).all()
        _same((s[1:2], i[1:2]), R.topk(scores[2:3], k, np.array([lone])), k)
    s, i, seen = _search(ov, Q[1:2], 64, 2)         # the empty list and one more: a sorted head, then the tail
    m = int(seen[0])
    head = min(m, 64)
    assert (i[0, :head] >= 0).all() and (i[0, head:] == -1).all() and np.isneginf(s[0, head:]).all()
    assert (np.diff(s[0, :head]) <= 0).all()


# ---------------------------------------------------------------------------------------------------------------- 5. nesting
@pytest.mark.parametrize("case", [c for c in S.CASES if c[2] > 1], ids=_ids)
def test_kth_score_never_drops_as_nprobe_grows(case):
    dim, n, nlist, kind, j = case
    sh, ov, Q, *_ = _built(case)
    for k in KS:
        kth = [_search(ov, Q, k, nprobe)[0][:, k - 1] for nprobe in (1, 3, nlist)]
        assert (kth[0] <= kth[1]).all() and (kth[1] <= kth[2]).all(), k


# ---------------------------------------------------------------------------------------------------------------- 6. training
def _trained(dim, n, nlist, X, iters, max_rows):
    """Two trainings of one shard -> [(centroids, list_off, list_rows)] * 2 and x^ of its rows."""
    from verbatim_rag_amd.vector_stores import IvfOverlay, Sq8Shard

    sh = Sq8Shard(dim, n)
    try:
        sh.add(X)
        out = []
        for _ in range(2):
            ov = IvfOverlay(sh, nlist)
            ov.train(iters, max_rows)
            ov.sync()
            out.append(ov.read())
            ov.close()
        return out, S.dequantized(*sh.read())
    finally:
        sh.close()


TRAIN_CASES = [(64, 3001, 16, 1 << 40), (100, 3001, 16, 1 << 40), (768, 3001, 64, 1 << 40), (64, 20000, 64, 64 * 64), (384, 257, 64, 100)]


@pytest.mark.parametrize("dim,n,nlist,max_rows", TRAIN_CASES)
def test_training_is_reproducible_and_lists_are_pure(dim, n, nlist, max_rows):
    X, label = V.clusters(dim, n)
    (a, b), _xhat = _trained(dim, n, nlist, X, 10, max_rows)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two trainings of the same rows differ"
    cent, off, rows = a
    got = _lists(off, rows, n)
    for l in range(nlist):
        assert len(np.unique(label[got == l])) <= 1, f"list {l} holds rows of more than one cluster"


@pytest.mark.parametrize("dim,max_rows", [(64, 1 << 40), (100, 1000), (768, 1 << 40)])
def test_initial_centroids_and_the_first_update(dim, max_rows):
    """iters = 0 leaves x^ of the evenly strided sample rows; one round on integer rows (exact assignment scores) gives, bit for
    bit, the fp32 mean of the members' x^ summed in ascending row order (numpy's cumsum is that sum), an empty list keeping its
    centroid.  dim 100: pad columns; dim 768: three columns per thread of the update."""
    n, nlist = 3001, 7 if dim < 768 else 64
    X = S.data("integer", dim, n, nlist, 7)[0][:n]
    sample, first = V.training_rows(n, max_rows, nlist)
    ((c0, _o, _r), _), xhat = _trained(dim, n, nlist, X, 0, max_rows)
    assert np.array_equal(xhat, X) and np.array_equal(c0, xhat[first])
    ((c1, off, rows), _), _ = _trained(dim, n, nlist, X, 1, max_rows)
    a = V.assign64(xhat[sample], c0)
    assert len(np.unique(a)) > 1
    for l in range(nlist):
        mem = sample[a == l]
        want = np.cumsum(xhat[mem], axis=0, dtype=np.float32)[-1] / np.float32(len(mem)) if len(mem) else c0[l]
        assert np.array_equal(c1[l].view(np.uint32), want.view(np.uint32)), l
    _lists(off, rows, n)


# ---------------------------------------------------------------------------------------------------------------- 7. appends
@pytest.mark.parametrize("case", [S.CASES[1], S.CASES[6]], ids=_ids)
def test_rows_added_after_a_sync_wait_for_the_next_one(case):
    dim, n, nlist, kind, j = case
    sh, ov, Q, *_ = _built(case)
    X = S.data(kind, dim, n, nlist, j)[0]
    before = _search(ov, Q[:17], 10, nlist)
    sh.add(X[n:])
    try:
        after = _search(ov, Q[:17], 10, nlist)
        _same(after[:2], before[:2], "rows appended to the base showed up before a sync")
        assert (after[1] < n).all() and (after[2] == n).all()
        ov.sync()
        assert ov.stats()["rows"] == n + S.APPENDED
        s, i, seen = _search(ov, Q[:17], 10, nlist)
        assert (i[0] >= n).all() and (seen == n + S.APPENDED).all()       # the appended rows lead query 0's ranking
        _same((s, i), R.topk(S.reference(case)[3][:17], 10), "after the sync")
        _same((s, i), sh.search(Q[:17], 10), "after the sync, against the FLAT search")
    finally:
        _BUILT.pop(case)[0].close()     # the case's index has grown: the next user builds it afresh


# ---------------------------------------------------------------------------------------------------------------- 8. compaction
@pytest.mark.parametrize("case", [S.CASES[3], S.CASES[7]], ids=_ids)
def test_remap_after_a_compaction_of_the_base(case):
    dim, n, nlist, kind, j = case
    sh, ov, Q, cent, xhat, off, rows = _built(case)
    try:
        before = _lists(off, rows, n)
        keep = np.random.default_rng(n + dim).random(n) < 0.7
        keep[rows[off[1]]] = False                  # the list of one row becomes empty
        assert sh.compact(keep) == int(keep.sum())
        ov.remap(keep)
        m = int(keep.sum())
        cent2, off2, rows2 = ov.read()
        assert cent2.tobytes() == cent.tobytes() and ov.stats()["rows"] == m
        assert np.array_equal(_lists(off2, rows2, m), before[keep]), "a surviving row changed its list"
        assert off2[2] == off2[1]
        for nq, k in ((17, 10), (100, 64)):
            s, i, seen = _search(ov, Q[:nq], k, nlist)
            _same((s, i), sh.search(Q[:nq], k), (nq, k))
            _same((s, i), R.topk(S.reference(case)[3][:nq, :n][:, keep], k), (nq, k, "sq8_ref over the survivors"))
            assert (seen == m).all()
    finally:
        _BUILT.pop(case)[0].close()


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_the_handle_usable():
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.vector_stores import IvfOverlay, Sq8Shard

    lib = _lib.load()
    X, Q, Cn = S.data("integer", 100, 257, 7, 0)[:3]
    sh = Sq8Shard(100, 300)
    try:
        sh.add(X[:257])
        for nlist in (0, 16385):
            h = C.c_void_p()
            assert lib.vrag_ivf_index_create_sq8(sh._h, nlist, C.byref(h)) == -1 and not h.value and "nlist" in _lib.last_error()
        h = C.c_void_p()
        assert lib.vrag_ivf_index_create_sq8(None, 7, C.byref(h)) == -1 and not h.value and "null base" in _lib.last_error()
        assert lib.vrag_ivf_index_create_sq8(sh._h, 7, None) == -1
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
        _same(ov.search(q, 5, 7), sh.search(q, 5), "after the refusals")                 # and the handle still answers
    finally:
        sh.close()


# ---------------------------------------------------------------------------------------------------------------- 10. slices
def test_many_queries_through_the_query_groups_and_slices():
    """nq = 300, nprobe = 64, k = 64 on the 20 000-row case (19 query groups per list) against sq8_ref; then 1 100 queries, which at
    nprobe x k = 4 096 keys per query is more than one slice of 2^22 candidate keys holds, against the FLAT search."""
    dim, n, nlist, kind, j = S.BIG
    sh, ov, *_ = _built(S.BIG)
    X = S.data(kind, dim, n, nlist, j)[0]
    Qb = V._unit(np.random.default_rng(300).standard_normal((1100, dim)))
    s, i, seen = _search(ov, Qb[:S.NQ_BIG], 64, 64)
    _same((s, i), R.search(X[:n], Qb[:S.NQ_BIG], 64), "300 queries")
    assert (seen == n).all()
    s, i, seen = _search(ov, Qb, 64, 64)
    _same((s, i), sh.search(Qb, 64), "1100 queries")
    s3, i3, seen3 = _search(ov, Qb, 64, 3)
    assert (seen3 <= n).all() and (s3[:, 63] <= s[:, 63]).all() and (i3[:, 0] >= 0).all()
