"""References of the tiled search kernels (tests/test_topk_unit_gpu.py), written from csrc/common.h, csrc/gemm_bf16.h and the comments
of csrc/topk.hip in numpy and integers: nothing here runs a kernel.

Keys (common.h): [orderable(score) : 32 | 0xFFFFFFFF - row : 32], the largest key is the best hit under (score desc, row asc); 0 = no key.
Scores are exact by construction (see `grid`): rows and queries are small integers times a power of two, so a dot product is an
integer below 2^24 in grid units and every partial sum in any order is exact in fp32."""
import numpy as np

from unit16 import from16, to16

U64 = np.uint64
NEG_INF_BITS = 0xFF800000
ROW_SCALE, Q_SCALE, QP_SCALE = 2.0 ** -3, 2.0 ** -2, 2.0 ** -8
ROW_MAX, Q_MAX, QP_MAX = 4, 3, 2047


# ------------------------------------------------------------------ keys
def orderable(s):
    b = np.ascontiguousarray(s, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unorderable(k):
    k = np.ascontiguousarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def make_key(s, row):
    return (orderable(s).astype(U64) << U64(32)) | (U64(0xFFFFFFFF) - np.asarray(row).astype(U64))


def key_score_bits(key):
    return unorderable((np.asarray(key, U64) >> U64(32)).astype(np.uint32)).view(np.uint32)


# ------------------------------------------------------------------ exact data
def grid(rng, n_rows, K, nq, pairs, density=0.25, q_nonzero=6):
    """(row bits [n_rows, K], query fp32 [nq, K], W bits [(2) nq, K], scores fp32 [n_rows, nq]) on the exact grid.  Rows: integers in
    [-4, 4] / 8, a quarter of them non-zero.  Queries, plain: integers in [-3, 3] / 4 (bf16-exact) on q_nonzero coordinates; pairs:
    9- to 11-bit integers / 256 that need EXACTLY two bf16 pieces.  Few distinct products: many equal scores, on purpose."""
    R = rng.integers(-ROW_MAX, ROW_MAX + 1, (n_rows, K)) * (rng.random((n_rows, K)) < density)
    Q = np.zeros((nq, K), np.int64)
    for q in range(nq):
        cols = rng.choice(K, size=min(q_nonzero, K), replace=False)
        if pairs:
            Q[q, cols] = rng.choice([257, -257, 514, 771, -1285, 2047, -1027], size=len(cols))
        else:
            Q[q, cols] = rng.choice([-3, -2, -1, 1, 2, 3], size=len(cols))
    qmax, qscale = (QP_MAX, QP_SCALE) if pairs else (Q_MAX, Q_SCALE)
    assert K * ROW_MAX * qmax < 2 ** 24, "a partial sum could leave fp32's exact integers"
    assert np.abs(R).max(initial=0) <= ROW_MAX and np.abs(Q).max() <= qmax
    rows = R * ROW_SCALE
    row_bits = to16(rows, False)
    assert np.array_equal(from16(row_bits, False), rows), "rows are not bf16-exact"
    qf = (Q * qscale).astype(np.float32)
    w = queries_ref(qf, nq, pairs, 2 * nq if pairs else nq)
    if pairs:
        hi, lo = from16(w[0::2], False), from16(w[1::2], False)
        assert np.array_equal(hi + lo, qf.astype(np.float64)) and np.all((lo != 0) == (Q != 0)), "queries do not split into exactly two bf16 pieces"
    else:
        assert np.array_equal(from16(w, False), qf.astype(np.float64)), "queries are not bf16-exact"
    S = R @ Q.T
    assert np.abs(S).max(initial=0) < 2 ** 24
    scores = (S * (ROW_SCALE * qscale)).astype(np.float32)
    assert np.array_equal(scores.astype(np.float64), S * (ROW_SCALE * qscale))
    return row_bits, qf, w, scores


def queries_ref(q, nq, pairs, n_cols_pad):
    """tiled_queries_kernel: the GEMM's W operand [n_cols_pad, dim] bf16 bits; pairs: rows (2q, 2q + 1) = (bf16(q), bf16(q - bf16(q)))."""
    q = np.ascontiguousarray(q, np.float32)
    w = np.zeros((n_cols_pad, q.shape[1]), np.uint16)
    if pairs:
        hi = to16(q[:nq], False)
        w[0:2 * nq:2] = hi
        w[1:2 * nq:2] = to16(q[:nq] - from16(hi, False).astype(np.float32), False)   # exact in fp32 (Sterbenz-like: the remainder of a rounding)
    else:
        w[:nq] = to16(q[:nq], False)
    return w


# ------------------------------------------------------------------ the score stage
def tile_map(d, skip):
    """gemm_bf16.h, topk_tile_skip: dense tile d of the tiles the sample left -> corpus tile."""
    s1 = skip - 1
    return d + d // s1 + 1 if d < 256 * s1 else d + 256


def stage_rows(M, row_base=0, stride=0, skip=0, tile0=0):
    """(corpus row each launch row m < M reads, row its key carries)."""
    m = np.arange(M, dtype=np.int64)
    if stride > 1:
        src = (m >> 8) * stride * 256 + (m & 255)       # launch tile t = corpus tile t * stride
        return src, row_base + src
    if skip > 1:
        ct = np.array([tile_map(tile0 + int(t), skip) for t in m >> 8], np.int64)
        src = ct * 256 + (m & 255)
        return src, row_base + src
    return row_base + m, row_base + m


def stage_direct_ref(scores, key_rows, thr_score):
    """Direct mode: slot m of query q = the row's key where score >= thr_score[q], else 0; no key test.  scores [M, nq]."""
    keys = make_key(scores, key_rows[:, None])
    return np.where(scores >= thr_score[None, :], keys, U64(0)).T.copy()      # [nq, M]


def stage_append_ref(scores, key_rows, thr_score, thr_key):
    """Append mode, per query: (slots reserved = rows with score >= thr_score, sorted non-zero keys = those also above thr_key)."""
    out = []
    for q in range(scores.shape[1]):
        hit = scores[:, q] >= thr_score[q]
        keys = make_key(scores[hit, q], key_rows[hit])
        out.append((int(hit.sum()), np.sort(keys[keys > thr_key[q]])))
    return out


def check_direct(buf, want, M, nq, canary):
    """buf [nq_buf, cap] after a direct launch over a canary-filled buffer."""
    assert np.array_equal(buf[:nq, :M], want), f"direct slots differ at {np.argwhere(buf[:nq, :M] != want)[:4].tolist()}"
    assert np.all(buf[:nq, M:] == canary), "slots at or beyond M were written"
    assert np.all(buf[nq:] == canary), "queries at or beyond nq were written"


def check_append(buf, cnt, c0, ref, nq, canary, cnt_canary):
    """buf [nq_buf, cap], cnt [nq_buf] after an appending launch; c0 [nq] the preset counters; ref from stage_append_ref."""
    cap = buf.shape[1]
    for q in range(nq):
        reserved, keys = ref[q]
        assert int(cnt[q]) - int(c0[q]) == reserved, f"query {q}: {int(cnt[q]) - int(c0[q])} slots reserved, {reserved} rows reach the threshold score"
        end = min(int(cnt[q]), cap)
        got = buf[q, int(c0[q]):end]
        assert np.all(buf[q, :int(c0[q])] == canary), f"query {q}: slots below the carry were written"
        assert np.all(buf[q, end:] == canary), f"query {q}: slots at or beyond the counter were written"
        if int(cnt[q]) <= cap:
            assert np.array_equal(np.sort(got[got != 0]), keys), f"query {q}: the appended keys are not the reference's"
            assert int((got == 0).sum()) == reserved - len(keys)
        else:   # overflow: which keys found a slot depends on the order of the atomics; each slot holds a key of the set, once
            assert np.all(got != 0) and len(np.unique(got)) == len(got) and np.all(np.isin(got, keys)), f"query {q}: overflowed slots hold foreign keys"
    assert np.all(buf[nq:] == canary), "queries at or beyond nq were written"
    assert np.all(cnt[nq:] == cnt_canary), "counters at or beyond nq were written"


# ------------------------------------------------------------------ selections, rescue, merge
def topk_ref(keys, k):
    """Brute force: the k largest non-zero keys, descending, zero tail."""
    keys = np.asarray(keys, U64)
    best = np.sort(keys[keys != 0])[::-1][:k]
    return np.concatenate([best, np.zeros(k - len(best), U64)])


def select_ref(keys, n, cap, k):
    """tiled_select_kernel / tiled_select_direct_kernel without overflow: (best k of the first min(n, cap) keys, cnt, thr_key, thr_score bits)."""
    m = min(n, cap)
    best = topk_ref(keys[:m], k)
    full = m >= k and best[k - 1] != 0
    return best, min(m, k), (best[k - 1] if full else U64(0)), (int(key_score_bits(best[k - 1:k])[0]) if full else NEG_INF_BITS)


def check_select(buf_k, want):
    assert np.array_equal(buf_k, want), f"the selection differs at {np.argwhere(buf_k != want)[:4].ravel().tolist()}"


def direct_select_overflows(keys, n, k, cap):
    """The windows of tiled_select_direct_kernel restated: True iff some window has more than cap - k keys above the cut (the k-th best
    of everything before it, 0 while fewer than k slots are sorted).  Deterministic; which survivors are then kept is not."""
    growth = 4 if k > 16 else 16
    seen = min(n, 1024 if k > 16 else 256)
    top = topk_ref(keys[:seen], k)
    P = 2
    while P < seen:
        P <<= 1
    while seen < n:
        chunk = min(n - seen, seen * (growth - 1))
        cut = top[k - 1] if P >= k else U64(0)
        win = keys[seen:seen + chunk]
        surv = win[win > cut]
        if len(surv) > cap - k:
            return True
        top = topk_ref(np.concatenate([top, surv]), k)
        P = 2
        while P < k + len(surv):
            P <<= 1
        seen += chunk
    return False
