"""The tiled batched dense search's kernels ALONE (vrag_debug_topk_run: launch_gemm(EPI_TOPK) and the launchers of
csrc/topk_kernels.h) against the numpy / integer references of tests/topk_ref.py.

Every comparison is EXACT (array_equal on key bits): the data sit on a dyadic grid on which each partial sum of a dot product, in
any order, is exact in fp32 (topk_ref.grid asserts K * max|row| * max|query| < 2^24 in grid units), so the GEMM's own accumulation
order does not matter -- and such data are full of equal scores, which is what the key test and the (score desc, row asc) order are
about.  No tolerance appears anywhere.  Every buffer goes in pre-filled with a canary and holds rows for queries behind nq:
whatever a kernel must not write must come back as it went in; the hook adds 4 KiB of device canary behind every buffer.

The score stage's tile configurations: 256 x 64 (tile 2) whatever M; tiles 0 and 1 take the small-batch 128 x 128 four-stage form
up to the small-batch row threshold (8 192 by default: every shape here), so the 256 x 128 / 256 x 256 forms and the 128 x 128
two-stage fall-through for M < 256 are reached with the threshold set to 0 for the call, as the GEMM unit test does.

CPU negative controls (unmarked): a stage result with one named defect must fail its comparison.

NOT MEASURED: no MI355X run of this module has been recorded yet.  The comparison functions, the data grids and the hook's
argument checks have run on the CPU against an emulation of the kernels built from the references; the kernels themselves have not
been compared.  test_select_fewer_than_k_keys_publishes_no_threshold is expected to fail without the `sk[k - 1] != 0` guard of
tiled_select_kernel with thr_score bits 0xffffffff (unorderable(0), read from the code, not observed)."""
import ctypes as C
import zlib

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib
import topk_ref as T

gpu = pytest.mark.gpu

U64 = np.uint64
CAN64 = U64(0x7A5C7A5C7A5C7A5C)
CAN32 = np.uint32(0x7A5C7A5C)
NEG_INF = np.float32(-np.inf)
EXTRA_Q = 2                                   # canary queries behind nq in every per-query buffer
TCAP = 2048                                   # the product's candidate buffer
PTRS = {n for n, t in _lib.DebugTopkArgs._fields_ if t is C.c_void_p}
DTYPES = {"corpus": np.uint16, "w": np.uint16, "queries": np.float32, "eps": np.float32, "src": np.uint64, "w_out": np.uint16,
          "buf": np.uint64, "cnt": np.uint32, "thr_key": np.uint64, "thr_score": np.float32, "out": np.uint64, "ovf": np.uint32,
          "done": np.uint32}
ERR_INVALID, ERR_HIP = -1, -2
CFG_TILE2 = [256, 64, 4, 1, 4, 0, 0]
CFG_TILE1 = [256, 128, 4, 2, 3, 0, 0]
CFG_TILE0 = [256, 256, 2, 4, 2, 0, 0]
CFG_SMALL = [128, 128, 2, 2, 4, 0, 0]         # M <= the small-batch threshold
CFG_FALL = [128, 128, 2, 2, 2, 0, 0]          # M < 256 above it
# (N, nq, pairs): the three tile forms at their column edges
FORMS = [(64, 1, 0), (64, 3, 0), (64, 63, 0), (64, 64, 0), (128, 65, 0), (128, 127, 0), (256, 129, 0), (256, 256, 0), (512, 300, 0),
         (64, 17, 1), (128, 33, 1)]
MS = [1, 130, 255, 256, 257, 511, 768]


# ------------------------------------------------------------------ the hook
def raw_run(op, **kw):
    a = _lib.DebugTopkArgs()
    keep = []
    for name, v in kw.items():
        if name in PTRS:
            if v is None:
                continue
            assert isinstance(v, np.ndarray) and v.flags.c_contiguous and v.dtype == DTYPES[name], name
            keep.append(v)
            setattr(a, name, v.ctypes.data)
        else:
            setattr(a, name, int(v))
    a.op = _lib.DEBUG_TOPK_OPS[op]
    if "small_rows" not in kw:
        a.small_rows = -1
    status = _lib.load_debug().vrag_debug_topk_run(C.byref(a), 0)
    del keep
    return status, a


def run(op, **kw):
    status, a = raw_run(op, **kw)
    if status == ERR_HIP:   # a failed launch or a clobbered canary: nothing more goes onto this device
        msg = _lib.load_debug().vrag_last_error()
        pytest.exit(f"vrag_debug_topk_run: {msg.decode() if msg else status}", returncode=3)
    _lib.check_debug("vrag_debug_topk_run", status)
    return a


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def can64(*shape):
    return np.full(shape, CAN64, U64)


def can32(*shape):
    return np.full(shape, CAN32, np.uint32)


def tile_of(N):
    return 2 if N == 64 else 1 if N == 128 else 0


def expected_config(N, M, small_rows):
    if N == 64:
        return CFG_TILE2
    if M <= (8192 if small_rows < 0 else small_rows):
        return CFG_SMALL
    if M < 256:
        return CFG_FALL
    return CFG_TILE1 if N == 128 else CFG_TILE0


def f32bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def pad_w(w, N):
    out = np.zeros((N, w.shape[1]), np.uint16)
    out[:w.shape[0]] = w
    return out


def stage(corpus, w, scores_src, *, M, N, nq, pairs, direct, cap, thr_score, thr_key, c0=None, row_base=0, stride=0, skip=0, tile0=0,
          small_rows=0):
    """One score-stage launch over canary-filled buffers.  Returns (buf, cnt, key_rows, scores [M, nq] of the rows the launch reads)."""
    nb = nq + EXTRA_Q
    buf, cnt = can64(nb, cap), can32(nb)
    if c0 is not None:
        cnt[:nq] = c0
    ts = np.full(nb, np.float32(np.nan), np.float32)
    tk = can64(nb)
    ts[:nq], tk[:nq] = thr_score, thr_key
    ts_in, tk_in, cnt_in = ts.copy(), tk.copy(), cnt.copy()
    a = run("score_stage", corpus=corpus, w=pad_w(w, N), buf=buf, cnt=cnt, thr_key=tk, thr_score=ts, M=M, N=N, K=corpus.shape[1],
            corpus_rows=corpus.shape[0], nq=nq, nq_buf=nb, k=1, cap=cap, pairs=pairs, direct=direct, tile=tile_of(N), row_base=row_base,
            tile_stride=stride, tile_skip=skip, tile0=tile0, small_rows=small_rows)
    assert list(a.config) == expected_config(N, M, small_rows), f"configuration {list(a.config)}"
    assert np.array_equal(f32bits(ts), f32bits(ts_in)) and np.array_equal(tk, tk_in), "the thresholds were written"
    if direct:
        assert np.array_equal(cnt, cnt_in), "direct mode touched the counters"
    src, key_rows = T.stage_rows(M, row_base, stride, skip, tile0)
    return buf, cnt, key_rows, scores_src[src]


def occurring_threshold(scores_q, key_rows, rng):
    """A real (score, row) of the data whose score is shared by rows both below and above it (falls back to any row of the most
    frequent score).  Returns (thr_score, thr_key)."""
    vals, counts = np.unique(scores_q, return_counts=True)
    tied = vals[counts >= 3]
    s = rng.choice(tied[len(tied) // 2:]) if len(tied) else vals[np.argmax(counts)]
    rows = np.sort(key_rows[scores_q == s])
    r = rows[len(rows) // 2]
    return np.float32(s), T.make_key(np.float32(s), r)


# ------------------------------------------------------------------ SCORE_STAGE
@gpu
@pytest.mark.parametrize("N,nq,pairs", FORMS)
def test_stage_direct_tile_forms(N, nq, pairs):
    """Direct mode over every tile form and row count: half of the queries with -inf (every slot [q][0, M) holds the row's key), the
    others with a threshold score that occurs in the data (rows at or above it hold their key -- equal scores included, no key test --
    the others 0).  Slots [M, cap), queries behind nq and the counters stay as they were; row_base != 0 on every second shape."""
    for i, M in enumerate(MS):
        K = 768 if (M == 257 and N in (64, 256)) else (64, 128)[i % 2]
        rng = rng_for("direct", N, nq, pairs, M)
        row_base = 0 if i % 2 else 37
        corpus, _qf, w, scores = T.grid(rng, row_base + (M + 255) // 256 * 256 + 5, K, nq, pairs)   # real rows behind M: the last tile reads them
        cap = M + 3
        thr = np.full(nq, NEG_INF, np.float32)
        for q in range(1, nq, 2):
            thr[q] = rng.choice(scores[row_base:row_base + M, q])
        for small_rows in ((0, -1) if (N != 64 and M in (130, 257, 768)) else (0,)):
            buf, _cnt, key_rows, sc = stage(corpus, w, scores, M=M, N=N, nq=nq, pairs=pairs, direct=1, cap=cap, thr_score=thr,
                                            thr_key=np.zeros(nq, U64), row_base=row_base, small_rows=small_rows)
            want = T.stage_direct_ref(sc, key_rows, thr)
            assert np.all(want[0::2] != 0) and (nq < 2 or np.any(want[1::2] == 0) or M == 1)
            T.check_direct(buf, want, M, nq, CAN64)


@gpu
@pytest.mark.parametrize("N,nq,pairs", [(64, 40, 0), (128, 100, 0), (256, 200, 0), (64, 17, 1)])
def test_stage_direct_sampled(N, nq, pairs):
    """Sampled first stage: stride 3, M = 768 over a 9-tile corpus -- launch tile t reads corpus tile 3 t, slot = launch row, the key
    carries corpus row t * 3 * 256 + r."""
    rng = rng_for("sampled", N, nq, pairs)
    corpus, _qf, w, scores = T.grid(rng, 9 * 256, 64, nq, pairs)
    thr = np.full(nq, NEG_INF, np.float32)
    buf, _cnt, key_rows, sc = stage(corpus, w, scores, M=768, N=N, nq=nq, pairs=pairs, direct=1, cap=768, thr_score=thr,
                                    thr_key=np.zeros(nq, U64), stride=3)
    assert key_rows[256] == 768 and key_rows[767] == 6 * 256 + 255
    T.check_direct(buf, T.stage_direct_ref(sc, key_rows, thr), 768, nq, CAN64)


def append_case(N, nq, pairs, M, K, k=10, cap=TCAP, row_base=0, skip=0, tile0=0, corpus_rows=None, small_rows=0, key=()):
    rng = rng_for("append", N, nq, pairs, M, K, skip, tile0, small_rows, key)
    corpus, _qf, w, scores = T.grid(rng, corpus_rows or row_base + (M + 255) // 256 * 256 + 3, K, nq, pairs)
    src, key_rows = T.stage_rows(M, row_base, 0, skip, tile0)
    sc = scores[src]
    thr_s, thr_k = np.empty(nq, np.float32), np.empty(nq, U64)
    c0 = np.array([(0, 5, k)[q % 3] for q in range(nq)], np.uint32)
    for q in range(nq):
        if q % 5 == 4:   # a threshold nothing reaches: the counter stays
            thr_s[q] = sc[:, q].max() + np.float32(1.0)
            thr_k[q] = T.make_key(thr_s[q], 0)
        else:
            thr_s[q], thr_k[q] = occurring_threshold(sc[:, q], key_rows, rng)
    buf, cnt, key_rows2, sc2 = stage(corpus, w, scores, M=M, N=N, nq=nq, pairs=pairs, direct=0, cap=cap, thr_score=thr_s, thr_key=thr_k,
                                     c0=c0, row_base=row_base, skip=skip, tile0=tile0, small_rows=small_rows)
    assert np.array_equal(key_rows, key_rows2) and np.array_equal(sc, sc2)
    ref = T.stage_append_ref(sc, key_rows, thr_s, thr_k)
    T.check_append(buf, cnt, c0, ref, nq, CAN64, CAN32)
    for q in range(4, nq, 5):
        assert ref[q][0] == 0 and cnt[q] == c0[q]
    return ref


@gpu
@pytest.mark.parametrize("N,nq,pairs", FORMS)
def test_stage_append_tile_forms(N, nq, pairs):
    """Append mode: preset counters 0 / 5 / k, (thr_key, thr_score) a real (score, row) of the data whose score other rows share on
    both sides -- "equal score, higher row" reserves a slot and writes "no key".  cnt - c0 = the reserved count, the non-zero keys of
    [c0, cnt) = the reference set, the rest of the range 0, every other slot untouched."""
    dropped = 0
    for i, M in enumerate(MS):
        K = 768 if (M == 511 and N in (64, 128, 512)) else (128, 64)[i % 2]
        for small_rows in ((0, -1) if (N != 64 and M in (130, 768)) else (0,)):
            ref = append_case(N, nq, pairs, M, K, row_base=(0, 512 + 11)[i % 2], small_rows=small_rows)
            dropped += sum(r - len(keys) for r, keys in ref)
    assert dropped > 0, "no reserved slot failed the key test: the ties at the threshold were not exercised"


@gpu
@pytest.mark.parametrize("N,nq,c0", [(64, 2, 0), (64, 5, 5), (256, 130, 0), (128, 70, 5)])
def test_stage_append_overflow(N, nq, c0):
    """cap = 64, M = 512, no threshold: the counter reaches c0 + M, slots [c0, cap) hold distinct keys of the query's own set (a
    neighbour's key has another score pattern: the membership test is per query), nothing is written at or beyond cap."""
    rng = rng_for("overflow", N, nq, c0)
    M, cap = 512, 64
    corpus, _qf, w, scores = T.grid(rng, M, 64, nq, 0, density=0.5, q_nonzero=24)
    thr_s, thr_k = np.full(nq, NEG_INF, np.float32), np.zeros(nq, U64)
    c0s = np.full(nq, c0, np.uint32)
    buf, cnt, key_rows, sc = stage(corpus, w, scores, M=M, N=N, nq=nq, pairs=0, direct=0, cap=cap, thr_score=thr_s, thr_key=thr_k, c0=c0s)
    assert np.all(cnt[:nq] == c0 + M)
    T.check_append(buf, cnt, c0s, T.stage_append_ref(sc, key_rows, thr_s, thr_k), nq, CAN64, CAN32)


@gpu
@pytest.mark.parametrize("N,nq", [(64, 30), (128, 90), (256, 140)])
def test_stage_append_skip_map(N, nq):
    """The appending stages' tile map d + d / (skip - 1) + 1 below 256 (skip - 1), d + 256 beyond: skip 2 across its boundary (tile0 =
    255, two tiles -> corpus tiles 511 and 512 of 514) and skip 3 from tile0 = 0 (three tiles -> corpus tiles 1, 2, 4)."""
    assert [T.tile_map(d, 2) for d in (255, 256)] == [511, 512] and [T.tile_map(d, 3) for d in (0, 1, 2)] == [1, 2, 4]
    append_case(N, nq, 0, 512, 64, skip=2, tile0=255, corpus_rows=514 * 256)
    append_case(N, nq, 0, 768, 64, skip=3, tile0=0, corpus_rows=5 * 256)


# ------------------------------------------------------------------ QUERIES
@gpu
@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("n_pad,nq", [(64, 1), (64, 31), (128, 50), (128, 64), (256, 97), (256, 128)])
def test_queries_operand(pairs, n_pad, nq):
    """fp32 queries -> the W operand: exact bits, bf16(q - bf16(q)) included, zero rows behind the queries."""
    if pairs:
        nq = min(nq, n_pad // 2)
    rng = rng_for("queries", pairs, n_pad, nq)
    for dim in (64, 200, 768):
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        q[0, :4] = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9]   # signed zeros, a tie to even, a round-up
        w = np.full((n_pad, dim), 0x7A5C, np.uint16)
        run("queries", queries=q, w_out=w, N=n_pad, K=dim, nq=nq, nq_buf=nq, pairs=pairs)
        want = T.queries_ref(q, nq, pairs, n_pad)
        assert np.array_equal(w, want), f"dim {dim}: {np.argwhere(w != want)[:4].tolist()}"
        assert not np.any(w[(2 if pairs else 1) * nq:])


# ------------------------------------------------------------------ SELECT
def unique_keys(rng, n, zero_every=0):
    """n unique random keys of finite scores and rows, zeros interspersed."""
    scores = rng.standard_normal(n).astype(np.float32)
    keys = T.make_key(scores, rng.permutation(n))
    assert len(np.unique(keys)) == n
    if zero_every:
        keys[rng.random(n) < 1.0 / zero_every] = 0
    return keys


SELECT_COUNTS = lambda k: [0, 1, k - 1, k, k + 1, 2047, 2048, 2049, 6000]  # noqa: E731


def select_launch(keys_per_q, counts, k, with_out, cap=TCAP):
    nq = len(counts)
    nb = nq + EXTRA_Q
    buf = can64(nb, cap)
    for q, keys in enumerate(keys_per_q):
        buf[q, :len(keys)] = keys
    before = buf.copy()
    cnt, ovf = can32(nb), np.zeros(nb, np.uint32)
    ovf[nq:] = CAN32
    cnt[:nq] = counts
    tk, ts = can64(nb), can32(nb).view(np.float32)
    out = can64(nb, k) if with_out else None
    run("select", buf=buf, cnt=cnt, thr_key=tk, thr_score=ts, out=out, ovf=ovf, nq=nq, nq_buf=nb, k=k, cap=cap)
    for q in range(nq):
        want, c, key, sbits = T.select_ref(before[q], int(counts[q]), cap, k)
        T.check_select(buf[q, :k], want)
        assert np.array_equal(buf[q, k:], before[q, k:]), "slots at or beyond k were written"
        if with_out:
            T.check_select(out[q], want)
        assert cnt[q] == c and tk[q] == key, (q, int(counts[q]), int(cnt[q]), hex(int(tk[q])), hex(int(key)))
        assert f32bits(ts)[q] == sbits, f"query {q} (count {int(counts[q])}): thr_score bits {int(f32bits(ts)[q]):#010x}, want {sbits:#010x}"
        assert ovf[q] == (1 if counts[q] > cap else 0)
    assert np.all(buf[nq:] == CAN64) and np.all(cnt[nq:] == CAN32) and np.all(tk[nq:] == CAN64) and np.all(ovf[nq:] == CAN32)
    assert np.all(f32bits(ts)[nq:] == CAN32) and (out is None or np.all(out[nq:] == CAN64))


@gpu
@pytest.mark.parametrize("k", [1, 5, 16, 17, 64])
@pytest.mark.parametrize("with_out", [True, False])
def test_select_sorts_the_stage(k, with_out):
    """One query per counter value: unique random keys with zeros interspersed; buf[:k], out, cnt = min(n, k), the thresholds, and
    ovf exactly where the counter exceeds cap."""
    rng = rng_for("select", k)
    counts = SELECT_COUNTS(k)
    select_launch([unique_keys(rng, TCAP, zero_every=7) for _ in counts], counts, k, with_out)


@gpu
@pytest.mark.parametrize("k", [2, 5, 16, 17, 64])
def test_select_fewer_than_k_keys_publishes_no_threshold(k):
    """n >= k reserved slots of which fewer than k hold a key (slots whose key failed the key test are written as 0): the selection
    must publish (0, -inf) like its first-stage sibling.  unorderable(0) has the bits 0xFFFFFFFF, a NaN: every later
    `score >= threshold` fails and the query admits nothing for the rest of the shard."""
    rng = rng_for("select-short", k)
    per_q, counts = [], []
    for n, nz in ((k, k - 1), (k + 3, 1), (300, k - 1), (TCAP, 0), (TCAP, k - 1)):
        keys = np.zeros(n, U64)
        keys[rng.choice(n, size=nz, replace=False)] = unique_keys(rng, nz)
        per_q.append(keys)
        counts.append(n)
    select_launch(per_q, counts, k, True)


# ------------------------------------------------------------------ SELECT_DIRECT
DIRECT_ORDERS = ("random", "descending", "ascending", "zeros", "short")


def direct_keys(rng, order, n, k, stride):
    keys = np.zeros(stride, U64)
    if order == "zeros":
        return keys
    if order == "short":
        nz = min(n, k - 1)
        keys[rng.choice(n, size=nz, replace=False)] = unique_keys(rng, nz)
        return keys
    body = unique_keys(rng, n, zero_every=9 if order == "random" else 0)
    keys[:n] = body if order == "random" else np.sort(body)[::-1] if order == "descending" else np.sort(body)
    keys[n:] = CAN64   # behind n: larger than any key, must never be read
    return keys


def direct_cases(k):
    for n in sorted({1, max(k - 1, 1), k, 255, 256, 257, 1024, 1025, 4096, 4097, 5000, 65536}):
        rng = rng_for("select-direct", k, n)
        stride = n + 5
        src = np.stack([direct_keys(rng, o, n, k, stride) for o in DIRECT_ORDERS])
        yield n, stride, src, [T.direct_select_overflows(src[i, :n], n, k, TCAP) for i in range(len(DIRECT_ORDERS))]


@pytest.mark.parametrize("k", [1, 10, 16, 17, 64])
def test_select_direct_only_ascending_keys_are_predicted_to_overflow(k):
    """CPU: the reference alone.  Every case but the ascending order is predicted clean, so none drops out of the GPU comparison
    unnoticed; the ascending order overflows at the large windows."""
    seen = {}
    for n, _stride, _src, pred in direct_cases(k):
        for o, p in zip(DIRECT_ORDERS, pred):
            assert not p or o == "ascending", (k, n, o)
        seen[n] = pred[DIRECT_ORDERS.index("ascending")]
    assert seen[65536] and seen[5000] and not seen[255]


@gpu
@pytest.mark.parametrize("k", [1, 10, 16, 17, 64])
def test_select_direct_windows(k):
    """One query per key order, src_stride > n.  ovf equals the reference's prediction in every case; the outputs are asserted in
    every case predicted clean (all but ascending orders: the CPU test above)."""
    nq = len(DIRECT_ORDERS)
    nb = nq + EXTRA_Q
    for n, stride, src, pred in direct_cases(k):
        buf, cnt, ovf = can64(nb, TCAP), can32(nb), np.zeros(nb, np.uint32)
        ovf[nq:] = CAN32
        tk, ts, out = can64(nb), can32(nb).view(np.float32), can64(nb, k)
        run("select_direct", src=src, buf=buf, cnt=cnt, thr_key=tk, thr_score=ts, out=out, ovf=ovf, nq=nq, nq_buf=nb, k=k, cap=TCAP, n=n,
            src_stride=stride)
        for q, order in enumerate(DIRECT_ORDERS):
            assert ovf[q] == int(pred[q]), f"n {n} {order}: ovf {int(ovf[q])}, predicted {pred[q]}"
            assert np.all(buf[q, k:] == CAN64), f"n {n} {order}: slots at or beyond k were written"
            assert cnt[q] == min(n, k)
            if pred[q]:
                continue
            want, c, key, sbits = T.select_ref(src[q], n, n, k)
            T.check_select(buf[q, :k], want)
            T.check_select(out[q], want)
            assert tk[q] == key and f32bits(ts)[q] == sbits, f"n {n} {order}: thresholds {int(tk[q]):#x} {int(f32bits(ts)[q]):#x}"
        assert np.all(buf[nq:] == CAN64) and np.all(cnt[nq:] == CAN32) and np.all(tk[nq:] == CAN64) and np.all(ovf[nq:] == CAN32)
        assert np.all(out[nq:] == CAN64)
    status, _a = raw_run("select_direct", src=src, buf=buf, cnt=cnt, thr_key=tk, thr_score=ts, out=None, ovf=ovf, nq=nq, nq_buf=nb, k=k,
                         cap=TCAP, n=n, src_stride=stride)   # out is optional
    assert status == 0


# ------------------------------------------------------------------ RESCUE
@gpu
@pytest.mark.parametrize("dim", [64, 192, 768])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 1000, 4097])
def test_rescue_flagged_queries(dim, n_rows):
    """Five queries, flags on 1 and 3: their rows of out are the brute-force best k (zero tails where n_rows < k), the others keep
    their canary, every slice counter is back at 0.  64 slices over 65 rows: slices that hold no row."""
    rng = rng_for("rescue", dim, n_rows)
    nq = 5
    corpus, qf, _w, scores = T.grid(rng, n_rows, dim, nq, 0)
    keys = T.make_key(scores, np.arange(n_rows)[:, None])
    for slices in (8, 64):
        for k in (1, 10, 64):
            out, ovf, done = can64(nq, k), np.zeros(nq, np.uint32), np.zeros(nq, np.uint32)
            ovf[[1, 3]] = (1, 7)
            run("rescue", corpus=corpus, queries=qf, ovf=ovf, done=done, out=out, K=dim, corpus_rows=n_rows, n=n_rows, nq=nq, nq_buf=nq, k=k,
                slices=slices)
            for q in range(nq):
                if q in (1, 3):
                    T.check_select(out[q], T.topk_ref(keys[:, q], k))
                else:
                    assert np.all(out[q] == CAN64)
            assert not done.any() and list(ovf) == [0, 1, 0, 7, 0]


# ------------------------------------------------------------------ MERGE
@gpu
@pytest.mark.parametrize("n_wg", [1, 2, 255, 256, 257, 1536])
@pytest.mark.parametrize("k", [1, 10, 32, 33, 64])
def test_merge_lists(n_wg, k):
    """Per-workgroup lists sorted descending with zero tails, some wholly empty, keys unique -> numpy's sort; the lists kernel up to
    k = 32, the scan kernel from 33.  One case has every list empty."""
    for nq in (1, 3):
        rng = rng_for("merge", n_wg, k, nq)
        cand = np.zeros((n_wg, nq, k), U64)
        pool = unique_keys(rng, n_wg * nq * k).reshape(n_wg, nq, k)
        for w in range(n_wg):
            for q in range(nq):
                fill = 0 if (w % 5 == 3 and n_wg > 1) else int(rng.integers(0, k + 1)) if w % 2 else k
                cand[w, q, :fill] = np.sort(pool[w, q, :fill])[::-1]
        out = can64(nq + EXTRA_Q, k)
        run("merge", src=cand, out=out, n=n_wg, nq=nq, nq_buf=nq + EXTRA_Q, k=k)
        for q in range(nq):
            T.check_select(out[q], T.topk_ref(cand[:, q].ravel(), k))
        assert np.all(out[nq:] == CAN64)
    if n_wg == 257:
        out = can64(2, k)
        run("merge", src=np.zeros((n_wg, 2, k), U64), out=out, n=n_wg, nq=2, nq_buf=2, k=k)
        assert not out.any()


# ------------------------------------------------------------------ TAU
@gpu
def test_tau_thresholds():
    nq, nb = 300, 302
    rng = rng_for("tau")
    ts = can32(nb).view(np.float32).copy()
    ts[:nq] = rng.standard_normal(nq).astype(np.float32)
    ts[:nq:7] = NEG_INF
    eps = np.abs(rng.standard_normal(nq)).astype(np.float32) * np.float32(1e-2)
    want = ts[:nq] - np.float32(2.0) * eps
    tk, cnt, flag = can64(nb), can32(nb), can32(nb)
    run("tau", thr_key=tk, thr_score=ts, eps=eps, cnt=cnt, ovf=flag, nq=nq, nq_buf=nb)
    assert np.array_equal(f32bits(ts[:nq]), f32bits(want)) and np.all(np.isneginf(ts[:nq:7]))
    assert not tk[:nq].any() and not cnt[:nq].any() and not flag[:nq].any()
    assert np.all(tk[nq:] == CAN64) and np.all(cnt[nq:] == CAN32) and np.all(flag[nq:] == CAN32) and np.all(f32bits(ts[nq:]) == CAN32)


# ------------------------------------------------------------------ the hook's refusals
@gpu
def test_hook_refuses_what_could_leave_its_buffers():
    rng = rng_for("refuse")
    corpus, _qf, w, _s = T.grid(rng, 768, 64, 4, 0)
    nb = 6
    good = dict(corpus=corpus, w=pad_w(w, 64), buf=can64(nb, 1024), cnt=np.zeros(nb, np.uint32), thr_key=np.zeros(nb, U64),
                thr_score=np.full(nb, NEG_INF, np.float32), M=512, N=64, K=64, corpus_rows=768, nq=4, nq_buf=nb, k=10, cap=1024, pairs=0,
                direct=1, tile=2, small_rows=0)
    assert raw_run("score_stage", **good)[0] == 0
    bad = [dict(corpus=None), dict(k=0), dict(k=65), dict(cap=1), dict(K=96), dict(N=192), dict(N=128), dict(nq=65, nq_buf=70),
           dict(pairs=1, nq=33, nq_buf=40), dict(M=0), dict(cap=511), dict(M=769), dict(row_base=300), dict(tile_stride=2, M=300, cap=1024),
           dict(tile_stride=2, M=768), dict(tile_stride=2, tile_skip=2), dict(direct=0, tile_skip=2, tile0=1, M=512),
           dict(direct=0, tile_skip=2, M=300), dict(direct=0, cnt=np.full(nb, 2000, np.uint32)), dict(nq_buf=3),
           dict(tile=1, N=128, w=pad_w(w, 128), tile_stride=3, M=256, small_rows=-1)]
    msgs = set()
    for change in bad:
        status, _a = raw_run("score_stage", **{**good, **change})
        assert status == ERR_INVALID, change
        msgs.add(_lib.load_debug().vrag_last_error())
    assert len(msgs) >= 15
    sel = dict(buf=can64(3, TCAP), cnt=np.zeros(3, np.uint32), thr_key=np.zeros(3, U64), thr_score=np.zeros(3, np.float32),
               ovf=np.zeros(3, np.uint32), nq=3, nq_buf=3, k=10, cap=TCAP)
    src = np.zeros((3, 600), U64)
    for op, change in (("select", dict(cap=1000)), ("select", dict(cap=8192)), ("select", dict(ovf=None)),
                       ("select_direct", dict(src=src, n=601, src_stride=600)), ("select_direct", dict(src=src, n=0, src_stride=600)),
                       ("select_direct", dict(src=src, n=600, src_stride=600, cap=128)), ("select_direct", dict(n=5, src_stride=600))):
        kw = {**sel, **change}
        if "cap" in change:
            kw["buf"] = can64(3, change["cap"])
        assert raw_run(op, **kw)[0] == ERR_INVALID, (op, change)
    q = np.zeros((2, 64), np.float32)
    res = dict(corpus=corpus[:100], queries=q, ovf=np.zeros(2, np.uint32), done=np.zeros(2, np.uint32), out=can64(2, 10), K=64,
               corpus_rows=100, n=100, nq=2, nq_buf=2, k=10, slices=8)
    for change in (dict(slices=7), dict(slices=65), dict(n=0, corpus_rows=0), dict(K=32), dict(done=None)):
        assert raw_run("rescue", **{**res, **change})[0] == ERR_INVALID, change


# ------------------------------------------------------------------ CPU negative controls
def _control_stage():
    rng = rng_for("control")
    M, nq, k = 300, 4, 10
    _corpus, _qf, _w, scores = T.grid(rng, M, 64, nq, 0)
    _src, key_rows = T.stage_rows(M)
    return M, nq, k, scores, key_rows, rng


def test_control_row_bias_off_by_one_tile():
    M, nq, _k, scores, key_rows, _rng = _control_stage()
    thr = np.full(nq, NEG_INF, np.float32)
    want = T.stage_direct_ref(scores, key_rows, thr)
    buf = can64(nq + EXTRA_Q, M + 3)
    buf[:nq, :M] = want
    T.check_direct(buf, want, M, nq, CAN64)
    buf[:nq, 256:M] = T.stage_direct_ref(scores, key_rows + 256 * (key_rows >= 256), thr)[:, 256:]   # the second tile's bias one tile off
    with pytest.raises(AssertionError, match="direct slots differ"):
        T.check_direct(buf, want, M, nq, CAN64)


def _control_append(defect):
    M, nq, k, scores, key_rows, rng = _control_stage()
    cap = 512
    thr = [occurring_threshold(scores[:, q], key_rows, rng) for q in range(nq)]
    thr_s, thr_k = np.array([t[0] for t in thr], np.float32), np.array([t[1] for t in thr], U64)
    ref = T.stage_append_ref(scores, key_rows, thr_s, thr_k)
    c0 = np.array([0, 5, k, 0], np.uint32)
    buf, cnt = can64(nq + EXTRA_Q, cap), can32(nq + EXTRA_Q)
    for q in range(nq):
        reserved, keys = ref[q]
        got = np.zeros(reserved, U64)
        got[:len(keys)] = keys
        buf[q, c0[q]:c0[q] + reserved] = rng.permutation(got)
        cnt[q] = c0[q] + reserved
    T.check_append(buf, cnt, c0, ref, nq, CAN64, CAN32)
    defect(buf, cnt, c0, ref, thr_s, cap)
    T.check_append(buf, cnt, c0, ref, nq, CAN64, CAN32)


def test_control_tie_at_the_threshold_dropped():
    def defect(buf, cnt, c0, ref, thr_s, cap):
        row = buf[1, c0[1]:cnt[1]]
        tie = np.flatnonzero((row != 0) & (T.key_score_bits(row) == thr_s[1:2].view(np.uint32)[0]))
        assert len(tie), "the control's threshold has no tie above it"
        row[tie[0]] = 0
    with pytest.raises(AssertionError, match="not the reference's"):
        _control_append(defect)


def test_control_key_written_at_slot_cap():
    def defect(buf, cnt, c0, ref, thr_s, cap):
        buf.reshape(-1)[3 * cap + cap] = ref[3][1][0]   # query 3's slot `cap` = the first slot behind its buffer
    with pytest.raises(AssertionError, match="at or beyond nq were written"):
        _control_append(defect)

    def defect_mid(buf, cnt, c0, ref, thr_s, cap):
        buf.reshape(-1)[0 * cap + cap] = ref[0][1][0]   # query 0's slot `cap` = query 1's slot 0, below its carry
    with pytest.raises(AssertionError, match="below the carry"):
        _control_append(defect_mid)


def test_control_selection_kept_the_next_key():
    rng = rng_for("control-select")
    k = 10
    keys = unique_keys(rng, 500, zero_every=7)
    want, _c, _key, _s = T.select_ref(keys, 500, TCAP, k)
    T.check_select(want.copy(), want)
    got = want.copy()
    got[k - 1] = T.topk_ref(keys, k + 1)[k]
    with pytest.raises(AssertionError, match="the selection differs"):
        T.check_select(got, want)
