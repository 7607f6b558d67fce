"""numpy restatement of the PQ contract (include/vrag_amd.h, "PQ dense rows"): codebook half norms, the encoding rule, the
look-up table, the j-ordered score, the (score desc, id asc) ranking and the deterministic training.  Every chain is the CPU
oracle's (`oracle.topk_ref.dense_topk`: acc = fmaf(x[c], q[c], acc) for c ascending, one fp32 rounding per step -- a float64
product-and-round would round twice), every other operation one IEEE fp32 operation on float32 arrays, so the GPU tests compare
bits."""
import numpy as np

from oracle import topk_ref as T
from sq8_ref import topk  # noqa: F401  (the ranking is the SQ8 reference's)

KSUB = 256


def chains(U, V):
    """float32 `[len(U), len(V)]`: chain(U[a], V[b]) for every pair, from the oracle's top-len(V) lists (every row of V is in
    the list of every query, so the lists are the whole matrix in another order)."""
    U, V = np.ascontiguousarray(U, dtype=np.float32), np.ascontiguousarray(V, dtype=np.float32)
    out = np.empty((len(U), len(V)), np.float32)
    if len(U):
        s, i = T.dense_topk(V, U, len(V))
        assert (np.sort(i, axis=1) == np.arange(len(V))).all()
        np.put_along_axis(out, i, s, axis=1)
    return out


def split(x, m):
    """`[n, dim]` -> `[m, n, dsub]` contiguous."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x = x.reshape(-1, x.shape[-1])
    return np.ascontiguousarray(x.reshape(len(x), m, -1).transpose(1, 0, 2))


def half_norms(cb):
    """h[j][c] = 0.5f * chain(cb[j][c], cb[j][c])."""
    cb = np.ascontiguousarray(cb, dtype=np.float32)
    return np.stack([np.float32(0.5) * np.diagonal(chains(cb[j], cb[j])) for j in range(len(cb))]).astype(np.float32)


def encode(x, cb):
    """codes uint8 `[n, m]`: argmax_c (chain(x_j, cb[j][c]) - h[j][c]), the lowest c on ties (np.argmax returns the first)."""
    cb = np.ascontiguousarray(cb, dtype=np.float32)
    m, h, xs = len(cb), half_norms(cb), split(x, len(cb))
    codes = np.empty((xs.shape[1], m), np.uint8)
    for j in range(m):
        a = chains(xs[j], cb[j]) - h[j][None, :]
        assert a.dtype == np.float32
        codes[:, j] = np.argmax(a, axis=1)
    return codes


def lut(queries, cb):
    """LUT float32 `[nq, m, 256]`."""
    cb = np.ascontiguousarray(cb, dtype=np.float32)
    qs = split(queries, len(cb))
    return np.ascontiguousarray(np.stack([chains(qs[j], cb[j]) for j in range(len(cb))], axis=1))


def scores(table, codes):
    """`[nq, n]` float32: (((0 + LUT[0][code[0]]) + LUT[1][code[1]]) + ...), one fp32 addition per sub-space, j ascending."""
    S = np.zeros((table.shape[0], len(codes)), np.float32)
    for j in range(table.shape[1]):
        S = S + table[:, j, :][:, codes[:, j]]
    assert S.dtype == np.float32
    return S


def search(cb, codes, queries, k, passing=None):
    return topk(scores(lut(queries, cb), codes), k, passing)


def decode(codes, cb):
    """The vectors the codes stand for, float32 `[n, dim]`."""
    return np.concatenate([cb[j][codes[:, j]] for j in range(len(cb))], axis=1)


def train(rows, m, iters):
    """The deterministic training: initial centroid c of every sub-space = sample row c * n // 256; per round every row is
    assigned by `encode`, then a centroid is the sequential fp32 sum of its members' sub-vectors in ascending row order divided
    once by float32(count); an empty cluster keeps its centroid."""
    xs = split(rows, m)
    n = xs.shape[1]
    cb = np.ascontiguousarray(xs[:, (np.arange(KSUB, dtype=np.int64) * n) // KSUB, :])
    for _ in range(iters):
        codes = encode(rows, cb)
        for j in range(m):
            sums, counts = np.zeros((KSUB, xs.shape[2]), np.float32), np.zeros(KSUB, np.int64)
            for r in range(n):                       # ascending rows: the order of the contract's sum
                c = codes[r, j]
                sums[c] = sums[c] + xs[j, r]
                counts[c] += 1
            hit = counts > 0
            cb[j][hit] = sums[hit] / counts[hit].astype(np.float32)[:, None]
        assert cb.dtype == np.float32
    return cb
