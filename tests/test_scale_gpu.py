"""Dense search routes on shards past 2^32 elements, 2^32 bytes and 2^24 rows (tests/scale_cases.py: the generator, the shapes, the
case table and why the expected top-k needs no host scan).  One shard at a time -- (family, dtype) in table order, built on the
device in chunks of 2^28 elements through vrag_dense_index_add_device, its last 4 353 rows through the host add -- and on it every
case of the table through the harness library, whose launch log says which kernels answered.  Per case, no tolerance anywhere:
  * ids and score bits equal the planted-row oracle's (-1 / -inf tails where a filter lets fewer than k rows through);
  * the canary rows behind the result arrays are untouched;
  * the launch log holds exactly the case's expected set: a prefilter or tiled case that fell back to a full scan has FAILED;
and per shard the ids returned by its searches contain every edge row.

The pass kernels behind the tiled search (dense_topk_mfma2_kernel<12>, the four-queries scalar kernel) run over bf16 rows of this
size only without the tiled search: a child pytest process runs S.NO_TILED_CASES of this module under VRAG_TOPK_NO_TILED=1 (the
library reads it once per process).

A shard is skipped only when the device shows less free memory than 1.25 x what it needs (S.shard_bytes); a skipped shard is not
verified.  The SQ8 rows of family B go through the product library (vrag_sq8_index_*, both routes; its kernels are not in the launch
log) against tests/sq8_ref.py over the planted rows.  Out of scope: sparse and full-text indexes (their 2^31 lines are in nnz and in
postings, and building them on the host dominates any test)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import scale_cases as S
from verbatim_rag_amd import _lib

pytestmark = pytest.mark.gpu

_FP, _LP = C.POINTER(C.c_float), C.POINTER(C.c_int64)
_DTYPE = {"bf16": 0, "f32": 1, "f32+image": 2}
CANARY_ROWS = 2
CANARY_SCORE, CANARY_ID = np.float32(-12345.5), np.int64(-77)
CHUNK_ELEMS = 1 << 28
NO_TILED = bool(os.environ.get("VRAG_TOPK_NO_TILED"))
TABLE = S.NO_TILED_CASES if NO_TILED else S.CASES

STEPS = []
for _key in S.shard_order(TABLE):
    STEPS.append(("ingest", _key, None))
    STEPS += [("search", _key, c) for c in TABLE if (c.family, c.dtype) == _key]
    STEPS.append(("edges", _key, None))


def _step_id(step):
    what, key, c = step
    return S.case_id(c) if c else f"{key[0]}-{key[1]}-{what}"


# ------------------------------------------------------------------ the harness library
def _dbg():
    _lib.require_gpu()
    dbg = _lib.load_debug()
    for name, (res, args) in _lib.SIGNATURES.items():          # the overlay must come from the library its base comes from
        if name.startswith("vrag_ivf_index_"):
            fn = getattr(dbg, name)
            fn.restype, fn.argtypes = res, args
    return dbg


def _read_log(dbg):
    names = {v: n for n, v in _lib.DEBUG_TOPK_LAUNCH_IDS.items()}
    cap = 4096
    buf = (C.c_int32 * (3 * cap))()
    count, ovf = C.c_int32(-1), C.c_int32(-1)
    _lib.check_debug("vrag_debug_topk_launch_log_read", dbg.vrag_debug_topk_launch_log_read(buf, cap, C.byref(count), C.byref(ovf)))
    assert not ovf.value and 0 <= count.value <= cap, "the launch log overflowed"
    e = np.ctypeslib.as_array(buf)[: 3 * count.value].reshape(-1, 3)
    return {(names[int(i)], int(a), int(b)) for i, a, b in e}


# ------------------------------------------------------------------ one shard at a time
class _Shard:
    def __init__(self, key):
        self.key, self.h, self.found, self.skip = key, C.c_void_p(), set(), None
        self.family = S.FAMILIES[key[0]]
        self.plan = S.family_plan(key[0])


_CURRENT = None


def _api(dtype):
    """(library, function prefix, check) of a shard's index kind."""
    if dtype == "sq8":
        return _lib.load(), "vrag_sq8_index_", _lib.check
    return _dbg(), "vrag_dense_index_", _lib.check_debug


def _close():
    global _CURRENT
    if _CURRENT is not None and _CURRENT.h:
        lib, pre, _check = _api(_CURRENT.key[1])
        getattr(lib, pre + "destroy")(_CURRENT.h)
    _CURRENT = None


@pytest.fixture(scope="module", autouse=True)
def _close_last_shard():
    yield
    _close()


def _verify_rows(plan, r0, r1):
    """Rows of a chunk that are compared with the numpy form: its ends and the neighbourhood of every boundary inside it."""
    rows = set(range(r0, min(r0 + 64, r1))) | set(range(max(r1 - 64, r0), r1))
    for b in plan.bounds:
        if r0 <= b < r1:
            rows |= set(range(max(b - 64, r0), min(b + 64, r1)))
    return np.array(sorted(rows), np.int64)


def _ingest(key):
    import torch

    global _CURRENT
    _close()
    sh = _Shard(key)
    _CURRENT = sh
    dim, n, dtype = sh.family.dim, sh.family.n, key[1]
    lib, pre, check = _api(dtype)
    need = S.shard_bytes(dim, n, dtype)
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    if free0 < 1.25 * need:
        sh.skip = f"shard {key} needs {need / 1e9:.1f} GB and the device shows {free0 / 1e9:.1f} GB free (less than 1.25 x): NOT verified"
        pytest.skip(sh.skip)
    S.check_plan(sh.plan, sorted({c.k for c in TABLE if c.family == key[0]}))   # the k condition, before any search
    if dtype == "sq8":
        check(pre + "create", lib.vrag_sq8_index_create(dim, n, 0, C.byref(sh.h)))
    else:
        check(pre + "create", lib.vrag_dense_index_create(dim, n, _DTYPE[dtype], 0, C.byref(sh.h)))
    device_rows = n - S.HOST_TAIL
    chunk_rows = CHUNK_ELEMS // dim
    starts = list(range(0, device_rows, chunk_rows))
    low = free0
    for r0 in starts:
        r1 = min(r0 + chunk_rows, device_rows)
        X = S.chunk_torch(sh.plan, r0, r1, "cuda")
        assert X.dtype == torch.float32 and X.is_contiguous() and X.numel() <= CHUNK_ELEMS
        if r0 == starts[0] or r0 == starts[-1] or any(r0 <= b < r1 for b in sh.plan.bounds):
            rows = _verify_rows(sh.plan, r0, r1)
            got = X[torch.from_numpy(rows - r0).cuda()].cpu().numpy()
            assert np.array_equal(got, S.rows_numpy(sh.plan, rows)), f"chunk [{r0}, {r1}) differs from the numpy form"
        torch.cuda.synchronize()
        low = min(low, torch.cuda.mem_get_info()[0])
        check(pre + "add_device", getattr(lib, pre + "add_device")(sh.h, X.data_ptr(), r1 - r0, None))
        del X
    tail = S.rows_numpy(sh.plan, np.arange(device_rows, n))
    check(pre + "add", getattr(lib, pre + "add")(sh.h, tail.ctypes.data_as(_FP), n - device_rows))
    assert getattr(lib, pre + "size")(sh.h) == n
    torch.cuda.empty_cache()
    print(f"shard {key}: {n} x {dim}, stated need {need / 1e9:.2f} GB, peak device memory in use during ingest "
          f"{(free0 - low) / 1e9:.2f} GB, after it {(free0 - torch.cuda.mem_get_info()[0]) / 1e9:.2f} GB")
    return sh


def _shard(key):
    sh = _CURRENT if _CURRENT is not None and _CURRENT.key == key else _ingest(key)   # a case selected alone builds its shard
    if sh.skip:
        pytest.skip(sh.skip)
    return sh


# ------------------------------------------------------------------ one case
def _bitmap(n, lo, hi):
    bits = np.zeros((n + 31) // 32 * 32, np.uint8)
    bits[lo:hi] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)


def _expected(sh, c, Q):
    if c.api == "sq8":
        return S.expected_sq8(sh.plan, Q, c.k)
    if c.api == "sq8_filtered":
        lo, hi = S.filter_rows(sh.plan, "upper_half")
        return S.expected_sq8(sh.plan, Q, c.k, allowed=lambda ids: ((ids >= lo) & (ids < hi), False))
    if c.api != "filtered" or c.arg == "all":
        return S.expected(sh.plan, Q, c.k)
    lo, hi = S.filter_rows(sh.plan, c.arg)
    if hi - lo <= 100_000:
        return S.expected_over(sh.plan, np.arange(lo, hi), Q, c.k)
    return S.expected(sh.plan, Q, c.k, allowed=lambda ids: ((ids >= lo) & (ids < hi), False))


def _run_case(sh, c):
    import torch

    dbg = _dbg()
    n, dim = sh.family.n, sh.family.dim
    Q = S.queries(dim, c.nq)
    rs, ri = _expected(sh, c, Q)
    s = np.full((c.nq + CANARY_ROWS, c.k), CANARY_SCORE, np.float32)
    i = np.full((c.nq + CANARY_ROWS, c.k), CANARY_ID, np.int64)
    qp, sp, ip = Q.ctypes.data_as(_FP), s.ctypes.data_as(_FP), i.ctypes.data_as(_LP)
    extra = []
    dbg.vrag_debug_topk_launch_log_reset()
    if c.api == "host":
        _lib.check_debug("vrag_dense_index_search", dbg.vrag_dense_index_search(sh.h, qp, c.nq, c.k, sp, ip, None))
    elif c.api == "filtered":
        lo, hi = S.filter_rows(sh.plan, c.arg)
        words = _bitmap(n, lo, hi)
        rc = dbg.vrag_dense_index_search_filtered(sh.h, qp, c.nq, c.k, words.ctypes.data, n, sp, ip, None)
        _lib.check_debug("vrag_dense_index_search_filtered", rc)
    elif c.api in ("sq8", "sq8_filtered"):
        lib = _lib.load()
        _lib.check("vrag_sq8_index_set_route", lib.vrag_sq8_index_set_route(sh.h, c.arg))
        if c.api == "sq8":
            _lib.check("vrag_sq8_index_search", lib.vrag_sq8_index_search(sh.h, qp, c.nq, c.k, sp, ip, None))
        else:
            words = _bitmap(n, *S.filter_rows(sh.plan, "upper_half"))
            _lib.check("vrag_sq8_index_search_filtered", lib.vrag_sq8_index_search_filtered(sh.h, qp, c.nq, c.k, words.ctypes.data, n, sp, ip, None))
    elif c.api in ("base", "map"):
        ds, di = torch.from_numpy(s).cuda(), torch.from_numpy(i).cuda()
        row_map = torch.arange(n, dtype=torch.int64, device="cuda") * 3 + S.ID_BASE if c.api == "map" else None
        torch.cuda.synchronize()
        rc = dbg.vrag_dense_index_search_device(sh.h, qp, c.nq, c.k, row_map.data_ptr() if c.api == "map" else None, n if c.api == "map" else 0,
                                                0 if c.api == "map" else S.ID_BASE, ds.data_ptr(), di.data_ptr(), None)
        _lib.check_debug("vrag_dense_index_search_device", rc)
        torch.cuda.synchronize()
        s[:], i[:] = ds.cpu().numpy(), di.cpu().numpy()
        ri = np.where(ri >= 0, ri * 3 + S.ID_BASE if c.api == "map" else ri + S.ID_BASE, -1)   # int64 arithmetic on 32-bit rows
    elif c.api == "ivf":
        nlist = c.arg
        ivf = C.c_void_p()
        _lib.check_debug("vrag_ivf_index_create", dbg.vrag_ivf_index_create(sh.h, nlist, C.byref(ivf)))
        try:
            cent = np.ascontiguousarray(S.rows_numpy(sh.plan, np.arange(1000, 1000 + nlist)) * np.float32(8))
            _lib.check_debug("vrag_ivf_index_set_centroids", dbg.vrag_ivf_index_set_centroids(ivf, cent.ctypes.data_as(_FP)))
            _lib.check_debug("vrag_ivf_index_sync", dbg.vrag_ivf_index_sync(ivf))
            off, rows = np.zeros(nlist + 1, np.uint32), np.zeros(n, np.uint32)
            _lib.check_debug("vrag_ivf_index_read", dbg.vrag_ivf_index_read(ivf, None, off.ctypes.data, rows.ctypes.data))
            if not (off[0] == 0 and off[-1] == n and (np.diff(off.astype(np.int64)) >= 0).all()):
                extra.append(f"list offsets {off.tolist()} do not cover {n} rows")
            elif not (np.bincount(rows, minlength=n) == 1).all():
                extra.append("the lists do not partition [0, n)")
            scanned = np.zeros(c.nq, np.int64)
            rc = dbg.vrag_ivf_index_search(ivf, qp, c.nq, c.k, nlist, sp, ip, scanned.ctypes.data_as(_LP), None)
            _lib.check_debug("vrag_ivf_index_search", rc)
            if not (scanned == n).all():
                extra.append(f"nprobe = nlist scanned {scanned.tolist()} rows of {n}")
        finally:
            dbg.vrag_ivf_index_destroy(ivf)
    else:
        raise AssertionError(c.api)
    logged = _read_log(dbg)
    out = extra
    if c.expect is not None and logged != c.expect:
        out.append(f"launched {sorted(logged - c.expect)} beyond and not {sorted(c.expect - logged)} of the expected set")
    if not np.array_equal(i[: c.nq], ri):
        bad = np.argwhere(i[: c.nq] != ri)[:4]
        out.append(f"ids differ from the oracle at {bad.tolist()}: got {[int(i[a, b]) for a, b in bad]}, expected {[int(ri[a, b]) for a, b in bad]}")
    if not np.array_equal(s[: c.nq].view(np.uint32), rs.view(np.uint32)):
        out.append(f"score bits differ from the oracle at {np.argwhere(s[: c.nq].view(np.uint32) != rs.view(np.uint32))[:4].tolist()}")
    if not ((s[c.nq:] == CANARY_SCORE).all() and (i[c.nq:] == CANARY_ID).all()):
        out.append("the canary rows behind the last query were written")
    got = i[: c.nq][i[: c.nq] >= 0]
    if c.api == "base":
        got = got - S.ID_BASE
    elif c.api == "map":
        got = (got - S.ID_BASE) // 3
    sh.found |= set(got.tolist())
    assert not out, "\n".join(f"{S.case_id(c)}: {m}" for m in out)


@pytest.mark.parametrize("step", STEPS, ids=_step_id)
def test_scale(step):
    """The steps of one shard in order: ingest (with the chunk checks against the numpy form), every case of the table, then the
    check that the searches between them returned every edge row; the next shard's ingest closes this one.  A search step selected
    alone builds its shard first; an edges step says something only behind its shard's searches."""
    what, key, c = step
    t0 = time.perf_counter()
    try:
        if what == "ingest":
            _ingest(key)
        elif what == "search":
            _run_case(_shard(key), c)
        else:
            sh = _shard(key)
            missing = sorted(set(S.edge_rows(sh.plan).tolist()) - sh.found)
            assert not missing, f"shard {key}: edge rows {missing} were returned by none of its searches"
            _close()
    except _lib.VragError as e:   # a call the library refused or a HIP error: nothing more is started on a device that may have faulted
        pytest.exit(f"{_step_id(step)}: {e}", returncode=3)
    print(f"{_step_id(step)}: {time.perf_counter() - t0:.2f} s")


if not NO_TILED:
    def test_pass_kernels_behind_the_tiled_search_in_a_child_process():
        """S.NO_TILED_CASES on the bf16 rows of family B, in a fresh process under VRAG_TOPK_NO_TILED=1: the ingest, the four cases
        and the edge-row check must all have passed there."""
        import subprocess
        import sys

        _close()
        steps = 2 + len(S.NO_TILED_CASES)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"],
                             env={**os.environ, "VRAG_TOPK_NO_TILED": "1"}, capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0 and f"{steps} passed" in out.stdout and "skipped" not in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
