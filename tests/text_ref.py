"""Host references of the full-text index build and BM25 scoring stages of csrc/fulltext.hip, one per op of vrag_debug_text_run
(include/vrag_amd_debug.h).  Plain numpy: integers as integers, fp32 one rounded operation at a time (the file compiles with fp
contraction off), so every result is the device's bits.  Nothing here touches a device.

A segment is a dict: keys u64 [n_keys] ascending, pstart u32 [n_keys + 1], prow / ptf u32 [n_post] (rows ascending within a key),
row_lo, n_rows (the row range it covers), and df u32 [n_keys] once stats_ref has run."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from topk_ref import make_key

U64 = np.uint64
U32 = np.uint32
F32 = np.float32
FT_MAXSEG = 4
FT_ROWS = 4096      # rows per scoring workgroup
TILE = 4096         # elements per scan / sort tile


# ------------------------------------------------------------------ scan, sort
def scan_ref(x: np.ndarray) -> np.ndarray:
    """Exclusive scan modulo 2^32, out[n] = the total."""
    x = np.asarray(x, U32)
    out = np.zeros(len(x) + 1, U32)
    np.cumsum(x, dtype=U32, out=out[1:])
    return out


def sort_ref(key, row, tf, by_row: int = 0, row_bits: int = 0):
    """Stable sort of the three arrays by the key, or by the row's bits below 2^row_bits."""
    key, row, tf = np.asarray(key, U64), np.asarray(row, U32), np.asarray(tf, U32)
    if by_row:
        order = np.argsort(row & U32((1 << row_bits) - 1), kind="stable")
    else:
        order = np.argsort(key, kind="stable")
    return key[order], row[order], tf[order]


def query_sort_ref(key, row, tf, nq: int):
    """The two sorts of vrag_text_index_query_terms: by key, then stably by query number over whole bytes."""
    row_bits = 0
    while (1 << row_bits) < nq:
        row_bits += 8
    return sort_ref(*sort_ref(key, row, tf), by_row=1, row_bits=row_bits)


# ------------------------------------------------------------------ run-length encoding
def rle_ref(key, row, tf, unit: int) -> Dict[str, np.ndarray]:
    """Runs of equal (key, row) = postings, runs of equal key = keys; boundaries by comparison with the record before.  tf of a
    posting: the run length (unit) or the tf of the run's first record."""
    key, row, tf = np.asarray(key, U64), np.asarray(row, U32), np.asarray(tf, U32)
    n = len(key)
    kflag = np.ones(n, bool)
    kflag[1:] = key[1:] != key[:-1]
    pflag = kflag.copy()
    pflag[1:] |= row[1:] != row[:-1]
    ppos = np.nonzero(pflag)[0]
    pscan = np.cumsum(pflag) - pflag            # posting number of every record's run
    ptf = np.diff(np.append(ppos, n)).astype(U32) if unit else tf[ppos]
    return {"n_post": len(ppos), "n_keys": int(kflag.sum()), "ukeys": key[kflag], "pstart": np.append(pscan[kflag], len(ppos)).astype(U32),
            "prow": row[ppos], "ptf": ptf.astype(U32), "pkey": key[ppos]}


def segment_of(r: Dict[str, np.ndarray], row_lo: int, n_rows: int) -> dict:
    return {"keys": r["ukeys"], "pstart": r["pstart"], "prow": r["prow"], "ptf": r["ptf"], "row_lo": row_lo, "n_rows": n_rows}


def build_segment_ref(key, row, tf, unit: int, row_lo: int, n_rows: int) -> dict:
    """build_segment: records in row order -> stable sort by key -> RLE."""
    return segment_of(rle_ref(*sort_ref(key, row, tf), unit), row_lo, n_rows)


# ------------------------------------------------------------------ fold
def expand_ref(seg: dict):
    """A segment's postings back into (key, row, tf) records, in posting order."""
    counts = np.diff(seg["pstart"].astype(np.int64))
    return np.repeat(np.asarray(seg["keys"], U64), counts), np.asarray(seg["prow"], U32), np.asarray(seg["ptf"], U32)


def fold_ref(parts: Sequence[dict]) -> dict:
    """RLE (tf carried) of the stably key-sorted concatenation of the parts' expanded records."""
    recs = [expand_ref(p) for p in parts]
    key, row, tf = (np.concatenate([r[i] for r in recs]) for i in range(3))
    row_lo = parts[0]["row_lo"]
    return build_segment_ref(key, row, tf, 0, row_lo, parts[-1]["row_lo"] + parts[-1]["n_rows"] - row_lo)


# ------------------------------------------------------------------ statistics
def bits_of(words: np.ndarray, n: int) -> np.ndarray:
    """Bitmap words -> bool [n]."""
    words = np.asarray(words, U32)
    r = np.arange(n, dtype=np.int64)
    return ((words[r >> 5] >> (r & 31).astype(U32)) & U32(1)).astype(bool)


def words_of(bits: np.ndarray) -> np.ndarray:
    bits = np.asarray(bits, bool)
    out = np.zeros((len(bits) + 31) // 32, U32)
    r = np.nonzero(bits)[0]
    np.bitwise_or.at(out, r >> 5, (U32(1) << (r & 31).astype(U32)))
    return out


def kd_ref(dl: np.ndarray, n_live: int, sum_dl: int, k1: float, b: float) -> np.ndarray:
    """kd_kernel: avgdl = fp32(sum dl / N) from a float64 division, K_d = k1 * ((1 - b) + b * (dl / avgdl)), every operation
    rounded in fp32; k1 where avgdl is not above 0."""
    k1, b = F32(k1), F32(b)
    avgdl = F32(float(sum_dl) / float(n_live)) if n_live else F32(0)
    if not avgdl > 0:
        return np.full(len(dl), k1, F32)
    t = np.asarray(dl, U32).astype(F32) / avgdl
    return (k1 * ((F32(1) - b) + b * t)).astype(F32)


def stats_ref(dl, live_words, segs: Sequence[dict], k1: float, b: float, corpus: Optional[Tuple[int, int]] = None):
    """(N, sum dl) of the live rows as Python integers, K_d per row (from the corpus pair when given), df per segment = live rows
    among every key's postings."""
    dl = np.asarray(dl, U32)
    live = bits_of(live_words, len(dl))
    n_live, sum_dl = int(live.sum()), int(dl[live].astype(np.int64).sum())
    pair = corpus if corpus and corpus[0] else (n_live, sum_dl)
    dfs = []
    for g in segs:
        hit = live[g["prow"].astype(np.int64)].astype(np.int64)
        c = np.concatenate([[0], np.cumsum(hit)])
        ps = g["pstart"].astype(np.int64)
        dfs.append((c[ps[1:]] - c[ps[:-1]]).astype(U32))
    return (n_live, sum_dl), kd_ref(dl, pair[0], pair[1], k1, b), dfs


# ------------------------------------------------------------------ search
def lookup_ref(segs: Sequence[dict], qkeys) -> Tuple[np.ndarray, np.ndarray]:
    """tu [n_terms, 4]: the key's index in every segment, -1 = absent (and for the segments that are not there); df summed over
    the segments that hold it."""
    qkeys = np.asarray(qkeys, U64)
    tu = np.full((len(qkeys), FT_MAXSEG), -1, np.int32)
    df = np.zeros(len(qkeys), np.int64)
    for s, g in enumerate(segs):
        keys = np.asarray(g["keys"], U64)
        if len(keys) == 0:
            continue
        i = np.searchsorted(keys, qkeys)
        found = (i < len(keys)) & (keys[np.minimum(i, len(keys) - 1)] == qkeys)
        tu[found, s] = i[found]
        if "df" in g:
            df[found] += g["df"][i[found]].astype(np.int64)
    return tu, df


def scores_ref(segs: Sequence[dict], tu_q: np.ndarray, w_q: np.ndarray, kd: np.ndarray, n_rows: int, k1p1) -> np.ndarray:
    """One fp32 accumulator per row: terms in the order given, segments in order, c = w * ((tf * k1p1) / (tf + kd)), each
    operation rounded on its own."""
    acc = np.zeros(n_rows, F32)
    k1p1 = F32(k1p1)
    for u4, wt in zip(tu_q, np.asarray(w_q, F32)):
        for s, g in enumerate(segs):
            u = int(u4[s])
            if u < 0:
                continue
            a, e = int(g["pstart"][u]), int(g["pstart"][u + 1])
            rows = g["prow"][a:e].astype(np.int64)
            tf = g["ptf"][a:e].astype(F32)
            c = wt * ((tf * k1p1) / (tf + kd[rows]))
            acc[rows] = acc[rows] + c
    return acc


def score_ref(segs: Sequence[dict], q_indptr, tu, w, kd, live_words, allow_words, allow_rows: int, n_rows: int, k1p1, kk: int,
              bound=None) -> np.ndarray:
    """cand [blocks, nq, kk]: per block of 4 096 rows the keys of the hits (score > 0, live, allowed and below allow_rows, key
    below the query's bound), descending, the first kk, zero-filled."""
    nq = len(q_indptr) - 1
    n_blocks = (n_rows + FT_ROWS - 1) // FT_ROWS
    ok = bits_of(live_words, n_rows)
    if allow_words is not None:
        allowed = np.zeros(n_rows, bool)
        allowed[:allow_rows] = bits_of(allow_words, allow_rows)
        ok &= allowed
    rows = np.arange(n_rows, dtype=np.int64)
    cand = np.zeros((n_blocks, nq, kk), U64)
    tu = np.asarray(tu, np.int32).reshape(-1, FT_MAXSEG)
    for q in range(nq):
        j0, j1 = int(q_indptr[q]), int(q_indptr[q + 1])
        if j0 == j1:
            continue
        acc = scores_ref(segs, tu[j0:j1], w[j0:j1], kd, n_rows, k1p1)
        hit = (acc > 0) & ok
        keys = make_key(acc[hit], rows[hit])
        if bound is not None:
            keep = keys < U64(bound[q])
            keys, hit_rows = keys[keep], rows[hit][keep]
        else:
            hit_rows = rows[hit]
        blk = hit_rows // FT_ROWS
        for bi in np.unique(blk):
            best = np.sort(keys[blk == bi])[::-1][:kk]
            cand[bi, q, :len(best)] = best
    return cand
