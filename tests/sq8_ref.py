"""numpy restatement of the SQ8 contract (include/vrag_amd.h, "SQ8 dense rows"): the quantisation rule, the three-rounding
score and the (score desc, id asc) ranking with -1 / -inf tails.  Everything here is exact, so the GPU tests compare bits."""
import numpy as np


def quantize(x):
    """fp32 `[n, dim]` (or `[dim]`) -> (codes int8 `[n, dim]`, scales float32 `[n]`):
    m = max |x|, s = m / 127 in fp32, code = clamp(rint(x / s), -127, 127) with the division in fp32 and halves to even;
    a zero row has scale 0 and zero codes."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x = x.reshape(-1, x.shape[-1])
    m = np.abs(x).max(axis=1)
    s = (m / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.rint(x / s[:, None])
    assert r.dtype == np.float32
    r = np.where((m > 0)[:, None], r, np.float32(0))
    return np.clip(r, -127, 127).astype(np.int8), np.where(m > 0, s, np.float32(0)).astype(np.float32)


def scores(cq, sq, cr, sr):
    """`[nq, n]` float32: (float)idot * (s_q * s_r).  The integer dot is a float64 matmul of the codes (exact: |idot| <=
    4096 * 127^2 < 2^53), its conversion to fp32 rounds to nearest even like the device's int -> float conversion."""
    idot = cq.astype(np.float64) @ cr.astype(np.float64).T
    return idot.astype(np.float32) * (sq.astype(np.float32)[:, None] * sr.astype(np.float32)[None, :])


def topk(S, k, passing=None):
    """(scores `[nq, k]` float32, ids `[nq, k]` int64) by (score desc, id asc) over the columns `passing` (ascending ids; None =
    all), missing hits -1 / -inf."""
    nq = S.shape[0]
    ids = np.arange(S.shape[1], dtype=np.int64) if passing is None else np.asarray(passing, dtype=np.int64)
    sub = S if passing is None else S[:, ids]
    out_s, out_i = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)
    kk = min(k, len(ids))
    if kk:
        order = np.argsort(-sub, axis=1, kind="stable")[:, :kk]     # stable: equal scores keep ascending ids
        out_s[:, :kk] = np.take_along_axis(sub, order, axis=1)
        out_i[:, :kk] = ids[order]
    return out_s, out_i


def search(rows, queries, k, passing=None):
    """The whole contract: quantise both sides, score, rank."""
    cr, sr = quantize(rows)
    cq, sq = quantize(queries)
    return topk(scores(cq, sq, cr, sr), k, passing)
