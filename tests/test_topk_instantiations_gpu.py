"""Every dimension-selected instantiation of the dense scan, prefilter, sparse and merge kernels of csrc/topk.hip, pinned to
oracle/topk_ref.c: each search of tests/topk_instantiation_cases.py runs through the harness library's C API, whose launch log
(include/vrag_amd_debug.h, vrag_debug_topk_launch_log_*) says which kernels and template instantiations it launched.  Two checks
per case, no tolerance in either: the logged set equals the case's expected set, and ids and scores equal the oracle's bit for bit.

The ABI's result lists are contiguous [nq][k] arrays, so the output buffers carry their canary as whole rows behind row nq (there is
no slot of a row beyond k that is not the next row's first); they must come back untouched."""
import ctypes as C
import zlib

import numpy as np
import pytest

import topk_instantiation_cases as T
from oracle import topk_ref as O
from verbatim_rag_amd import _lib

pytestmark = pytest.mark.gpu

_FP, _LP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
_ID_NAMES = {v: n for n, v in _lib.DEBUG_TOPK_LAUNCH_IDS.items()}
_DTYPE = {"bf16": 0, "f32": 1, "f32+image": 2}
CANARY_ROWS = 2
CANARY_SCORE, CANARY_ID = np.float32(-12345.5), np.int64(-77)
BUNCHED_COPIES = 4160


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _grid(rng, shape, lim):
    return (rng.integers(-lim, lim + 1, size=shape) / 64.0).astype(np.float32)


# ------------------------------------------------------------------ data
def dense_rows(key):
    _kind, _dtype, dim, n, rows, lim_x = key
    rng = _rng("rows", key)
    if rows == "gauss":
        X = rng.standard_normal((n, dim)).astype(np.float32)
        X /= np.linalg.norm(X, axis=1, keepdims=True)
        if n > 8:
            X[n // 2] = X[3]                      # an exact duplicate: equal scores, the lower id first
        return X
    X = _grid(rng, (n, dim), lim_x)
    if rows in ("tail_last", "tail_first"):
        cols = slice(dim - 8, dim) if rows == "tail_last" else slice(0, 8)
        varied = X[:, cols].copy()
        X[:] = X[0]
        X[:, cols] = varied
    elif rows == "bunched":
        X[rng.choice(n, size=BUNCHED_COPIES, replace=False)] = X[7]
    elif n > 8:
        X[n // 2] = X[n // 3]                     # exact score ties: id ascending must decide
    return X


def dense_queries(c, X):
    rng = _rng("queries", T.case_id(c))
    if c.data == "gauss":
        Q = rng.standard_normal((c.nq, c.dim)).astype(np.float32)
        Q[0] = X[min(3, c.n - 1)] * np.float32(1.7)       # aligned with the duplicated row
        return Q
    if c.data == "grid_pairs":
        mag = rng.integers(257, c.lim_q + 1, size=(c.nq, c.dim)) | 1          # odd, above 2^8: nine or more significant bits
        Q = (mag * rng.choice([-1, 1], size=mag.shape) / 256.0).astype(np.float32)
        assert ((Q.view(np.uint32) & 0xFFFF) != 0).any(axis=1).all(), "the queries must not be bf16 numbers"
        return Q
    Q = _grid(rng, (c.nq, c.dim), c.lim_q)
    if c.data == "bunched":
        Q[0] = X[7]                                       # the copied row itself
    return Q


def sparse_corpus(key):
    """Slices of 64 equally long documents for every load-set edge, 64 of them empty, a partial last slice; documents in
    shuffled order (the index sorts them by length and maps positions back).  Half of a document's terms come from a small hot
    set the queries draw from, the rest from the whole vocabulary, its last terms included."""
    _kind, _dtype, vocab, n, rows, lim_x = key
    rng = _rng("sparse", key)
    lens = np.concatenate([np.full(64, 4 * ng) for ng in T.SPARSE_NG] + [rng.integers(45, 61, T.SPARSE_TAIL_DOCS)])
    assert len(lens) == n and n % 64 != 0 and (lens == 0).sum() >= 64 and lens.max() <= T.SPARSE_MAX_TERMS
    lens = lens[rng.permutation(n)]
    hot = sparse_hot_terms(vocab)
    indptr, idx, val = [0], [], []
    for m in lens:
        m = int(m)
        th = rng.choice(hot, size=min(m // 2, len(hot)), replace=False)
        cold = np.setdiff1d(rng.integers(0, vocab, size=2 * m + 8), hot)
        t = rng.permutation(np.concatenate([th, rng.permutation(cold)[: m - len(th)]]))   # the document's own term order, not ascending
        assert len(t) == m and len(np.unique(t)) == m
        idx.append(t)
        val.append(_sparse_weights(rng, len(t), rows, lim_x))
        indptr.append(indptr[-1] + len(t))
    return (np.asarray(indptr, np.int64), np.concatenate(idx).astype(np.int32), np.concatenate(val).astype(np.float32))


def sparse_hot_terms(vocab):
    return np.concatenate([np.arange(5, 45), [vocab - 1, vocab - 2, vocab - 9]])


def _sparse_weights(rng, m, rows, lim):
    if rows == "gauss":
        return np.abs(rng.standard_normal(m)).astype(np.float32) + np.float32(1e-3)
    return (rng.integers(1, lim + 1, size=m) / 64.0).astype(np.float32)


def sparse_queries(c):
    rng = _rng("sparse queries", T.case_id(c))
    hot = sparse_hot_terms(c.dim)
    rows = "gauss" if c.data == "gauss" else "grid"
    if c.data in ("union1023", "union1024"):
        total = 1023 if c.data == "union1023" else 1024
        cold = np.setdiff1d(rng.choice(c.dim, size=total + 200, replace=False), hot)[: total - len(hot)]
        assert len(np.unique(np.concatenate([hot, cold]))) == total
        parts = [rng.permutation(np.concatenate([hot[j::c.nq], part])) for j, part in enumerate(np.array_split(cold, c.nq))]   # hot terms in every query: every query has hits
    else:
        parts = [np.concatenate([rng.choice(hot, size=6, replace=False), np.setdiff1d(rng.integers(0, c.dim, size=3), hot)]) for _ in range(c.nq)]
    q_indptr = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    q_idx = np.concatenate(parts).astype(np.int32)
    q_val = _sparse_weights(rng, len(q_idx), rows, c.lim_q)
    return q_indptr, q_idx, q_val


# ------------------------------------------------------------------ the harness library
def _read_log(dbg):
    cap = 4096
    buf = (C.c_int32 * (3 * cap))()
    count, ovf = C.c_int32(-1), C.c_int32(-1)
    _lib.check_debug("vrag_debug_topk_launch_log_read", dbg.vrag_debug_topk_launch_log_read(buf, cap, C.byref(count), C.byref(ovf)))
    assert not ovf.value and 0 <= count.value <= cap, "the launch log overflowed"
    e = np.ctypeslib.as_array(buf)[: 3 * count.value].reshape(-1, 3)
    return {(_ID_NAMES[int(i)], int(a), int(b)) for i, a, b in e}


_HIP = None


def _hip_runtime():
    """The HIP runtime the harness library is linked against, opened by the path it is mapped from (one runtime per process:
    _lib._preload_torch_hip_runtime), for the device buffers of vrag_dense_index_search_device."""
    global _HIP
    if _HIP is None:
        _lib.load_debug()
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        _HIP = C.CDLL(path)
        _HIP.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]   # kind 1 = host to device, 2 = device to host
        _HIP.hipFree.argtypes = [C.c_void_p]
    return _HIP


def _outputs(nq, k):
    s = np.full((nq + CANARY_ROWS, k), CANARY_SCORE, np.float32)
    i = np.full((nq + CANARY_ROWS, k), CANARY_ID, np.int64)
    return s, i


def _dense_search(dbg, h, c, Q):
    s, i = _outputs(c.nq, c.k)
    dbg.vrag_debug_topk_launch_log_reset()
    if c.via == "host":
        rc = dbg.vrag_dense_index_search(h, Q.ctypes.data_as(_FP), c.nq, c.k, s.ctypes.data_as(_FP), i.ctypes.data_as(_LP), None)
        _lib.check_debug("vrag_dense_index_search", rc)
    else:
        hip = _hip_runtime()
        ds, di = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(ds), s.nbytes) == 0 and hip.hipMalloc(C.byref(di), i.nbytes) == 0
        try:   # the canary goes up with the buffers and comes back with the lists (null stream: the copies are ordered around the search)
            assert hip.hipMemcpy(ds, s.ctypes.data, s.nbytes, 1) == 0 and hip.hipMemcpy(di, i.ctypes.data, i.nbytes, 1) == 0
            rc = dbg.vrag_dense_index_search_device(h, Q.ctypes.data_as(_FP), c.nq, c.k, None, 0, 0, ds, di, None)
            _lib.check_debug("vrag_dense_index_search_device", rc)
            s[:], i[:] = 0, 0
            assert hip.hipMemcpy(s.ctypes.data, ds, s.nbytes, 2) == 0 and hip.hipMemcpy(i.ctypes.data, di, i.nbytes, 2) == 0
        finally:
            hip.hipFree(ds)
            hip.hipFree(di)
    return _read_log(dbg), s, i


def _check(c, logged, s, i, rs, ri):
    """The failures of one case as text (empty = passed)."""
    out = []
    if logged != c.expect:
        out.append(f"launched {sorted(logged - c.expect)} beyond and not {sorted(c.expect - logged)} of the expected set")
    if not np.array_equal(i[: c.nq], ri):
        out.append(f"ids differ from the oracle at {np.argwhere(i[: c.nq] != ri)[:4].tolist()}")
    if not np.array_equal(s[: c.nq].view(np.uint32), rs.view(np.uint32)):
        out.append(f"score bits differ from the oracle at {np.argwhere(s[: c.nq].view(np.uint32) != rs.view(np.uint32))[:4].tolist()}")
    if not ((s[c.nq:] == CANARY_SCORE).all() and (i[c.nq:] == CANARY_ID).all()):
        out.append("the canary rows behind the last query were written")
    return [f"{T.case_id(c)}: {m}" for m in out]


def _groups(pred):
    g = {}
    for c in T.CASES:
        if pred(c):
            g.setdefault(T.index_key(c), []).append(c)
    return g


DENSE = _groups(lambda c: c.kind == "dense" and c is not T.LARGE)
SPARSE = _groups(lambda c: c.kind == "sparse")


def _key_id(key):
    return "-".join(str(x) for x in key)


def _run_dense(key, cases):
    _lib.require_gpu()
    dbg = _lib.load_debug()
    _kind, dtype, dim, n, _rows, _lim = key
    X = dense_rows(key)
    stored = O.bf16_round(X) if dtype == "bf16" else X        # the oracle sees the rows the index stores
    h = C.c_void_p()
    _lib.check_debug("vrag_dense_index_create", dbg.vrag_dense_index_create(dim, n, _DTYPE[dtype], 0, C.byref(h)))
    failures = []
    try:
        cut = n // 3                                           # appended in two calls
        if cut:
            _lib.check_debug("vrag_dense_index_add", dbg.vrag_dense_index_add(h, X[:cut].ctypes.data_as(_FP), cut))
        _lib.check_debug("vrag_dense_index_add", dbg.vrag_dense_index_add(h, X[cut:].ctypes.data_as(_FP), n - cut))
        for c in cases:
            Q = dense_queries(c, X)
            logged, s, i = _dense_search(dbg, h, c, Q)
            rs, ri = O.dense_topk(stored, Q, c.k, blocked=c.nq >= 16)
            failures += _check(c, logged, s, i, rs, ri)
    finally:
        dbg.vrag_dense_index_destroy(h)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("key", list(DENSE), ids=_key_id)
def test_dense_instantiations(key):
    """One index per (dtype, dim, n, rows); every case of the table on it: the logged launches are the expected set, ids and
    scores are the oracle's bits, the canary rows survive."""
    _run_dense(key, DENSE[key])


def test_dense_exact3_two_pass_form_on_131k_rows():
    """The one large case: 131 201 fp32 rows of 512 (269 MB) are the smallest shard on which dense_topk_exact_kernel<3> runs its
    seeded two-pass form (a 32 768-row prefix, topk_seed_threshold_kernel, the main pass behind the thresholds)."""
    _run_dense(T.index_key(T.LARGE), [T.LARGE])


@pytest.mark.parametrize("key", list(SPARSE), ids=_key_id)
def test_sparse_instantiations(key):
    """One sparse index per (vocabulary, weights); every case of the table on it, as for the dense ones."""
    _lib.require_gpu()
    dbg = _lib.load_debug()
    _kind, _dtype, vocab, n, _rows, _lim = key
    indptr, idx, val = sparse_corpus(key)
    h = C.c_void_p()
    rc = dbg.vrag_sparse_index_create(vocab, n, indptr.ctypes.data_as(_LP), idx.ctypes.data_as(_IP), val.ctypes.data_as(_FP), 0, C.byref(h))
    _lib.check_debug("vrag_sparse_index_create", rc)
    failures = []
    try:
        for c in SPARSE[key]:
            qp, qi, qv = sparse_queries(c)
            s, i = _outputs(c.nq, c.k)
            dbg.vrag_debug_topk_launch_log_reset()
            rc = dbg.vrag_sparse_index_search(h, qp.ctypes.data_as(_LP), qi.ctypes.data_as(_IP), qv.ctypes.data_as(_FP), c.nq, c.k,
                                              s.ctypes.data_as(_FP), i.ctypes.data_as(_LP), None)
            _lib.check_debug("vrag_sparse_index_search", rc)
            rs, ri = O.sparse_topk(indptr, idx, val, vocab, qp, qi, qv, c.k)
            assert (ri[:, 0] >= 0).all(), "every query must have a hit, or the case tests nothing"
            failures += _check(c, _read_log(dbg), s, i, rs, ri)
    finally:
        dbg.vrag_sparse_index_destroy(h)
    assert not failures, "\n".join(failures)
