"""The full-text index build and BM25 scoring stages of csrc/fulltext.hip ALONE (vrag_debug_text_run: the product's own host
launchers, one stage per call) against the numpy references of tests/text_ref.py, then a whole index through the harness
library's vrag_text_index_* functions read back with vrag_debug_text_index_read.

Every comparison is EXACT: integers as integers, fp32 by bit pattern (the file compiles with fp contraction off and the references
round every operation on its own).  No tolerance appears anywhere.  Output buffers go in pre-filled with a canary and hold more
elements than the launch covers: whatever a kernel must not write must come back as it went in; the hook adds 4 KiB of device
canary behind every buffer.  The shapes are the smallest at which each kernel can still go wrong: the 4 096-element scan / sort
tile and the 4 096-row scoring block at their edges, more than 256 scan tiles (the tile sums carry across chunks), a wave of 64
equal digits, more than 16 384 keys (the df grid wraps), 257 and 65 537 queries (two and three digit passes of the by-row sort,
gridDim.y above 256).

CPU negative controls (unmarked): an expected value with one named defect must fail its comparison."""
import ctypes as C
import zlib

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib
import full_text_oracle as O
import text_ref as R
from topk_ref import make_key

gpu = pytest.mark.gpu

U64, U32, F32 = np.uint64, np.uint32, np.float32
CAN64 = U64(0x7A5C7A5C7A5C7A5C)
CAN32 = U32(0x7A5C7A5C)
ERR_INVALID, ERR_HIP = -1, -2
TILE = R.TILE
EXTRA = 5                                     # canary elements behind the launch's count in every output buffer
SEG_FIELDS = {"keys": ("seg_keys", U64), "pstart": ("seg_pstart", U32), "prow": ("seg_prow", U32), "ptf": ("seg_ptf", U32),
              "df": ("seg_df", U32)}
PTRS = {n for n, t in _lib.DebugTextArgs._fields_ if t is C.c_void_p}
DTYPES = {"in": U32, "out": U32, "key": U64, "row": U32, "tf": U32, "ukeys": U64, "pstart": U32, "prow": U32, "ptf": U32, "pkey": U64,
          "dl": U32, "live": U32, "allow": U32, "acc": U64, "kd": F32, "qkeys": U64, "tu": np.int32, "df_out": np.int64,
          "q_indptr": np.int64, "w": F32, "bound": U64, "cand": U64}


# ------------------------------------------------------------------ the hook
def raw_run(op, segs=None, **kw):
    a = _lib.DebugTextArgs()
    keep = []
    for name, v in kw.items():
        if name in PTRS:
            if v is None:
                continue
            assert isinstance(v, np.ndarray) and v.flags.c_contiguous and v.dtype == DTYPES[name], name
            keep.append(v)
            setattr(a, name, v.ctypes.data)
        elif name in ("k1", "b", "k1p1"):
            setattr(a, name, float(v))
        else:
            setattr(a, name, int(v))
    if segs is not None:
        a.n_segs = len(segs)
        for s, g in enumerate(segs[:4]):
            for key, (field, dt) in SEG_FIELDS.items():
                v = g.get(key)
                if v is None:
                    continue
                v = np.ascontiguousarray(v, dt)
                keep.append(v)
                g["_" + key] = v                                  # what the hook writes (df) is read from here
                getattr(a, field)[s] = v.ctypes.data
            a.seg_n_keys[s] = g.get("n_keys", len(g["keys"]))
            a.seg_n_post[s] = g.get("n_post", len(g["prow"]))
            a.seg_row_lo[s], a.seg_n_rows[s] = g["row_lo"], g["n_rows"]
    a.op = _lib.DEBUG_TEXT_OPS[op]
    status = _lib.load_debug().vrag_debug_text_run(C.byref(a), 0)
    del keep
    return status, a


def run(op, segs=None, **kw):
    status, a = raw_run(op, segs, **kw)
    if status == ERR_HIP:   # a failed launch or a clobbered canary: nothing more goes onto this device
        msg = _lib.load_debug().vrag_last_error()
        pytest.exit(f"vrag_debug_text_run: {msg.decode() if msg else status}", returncode=3)
    _lib.check_debug("vrag_debug_text_run", status)
    return a


def refused(match, op, segs=None, **kw):
    status, _a = raw_run(op, segs, **kw)
    msg = (_lib.load_debug().vrag_last_error() or b"").decode()
    assert status == ERR_INVALID and match in msg, (status, msg)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def can(n, dtype):
    dt = np.dtype(dtype)
    return np.full(n, CAN64 if dt.itemsize == 8 else CAN32).view(dt)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(U32) if x.dtype == F32 else x


def same(got, want):
    """Exact: same shape, same dtype width, same bits."""
    got, want = bits(np.asarray(got)), bits(np.asarray(want))
    return got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize and np.array_equal(got, want)


def is_canary(x):
    x = np.ascontiguousarray(x)
    return bool((x.view(U64 if x.dtype.itemsize == 8 else U32) == (CAN64 if x.dtype.itemsize == 8 else CAN32)).all())


# ------------------------------------------------------------------ SCAN
SCAN_NS = [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 256 * TILE - 1, 256 * TILE, 256 * TILE + 1, 2 * 256 * TILE + 5]


def scan_values(n):
    yield "random", rng_for("scan", n).integers(0, 1 << 16, n).astype(U32)
    yield "ones", np.ones(n, U32)
    yield "wrap", np.full(n, 0xFFFFFFFF, U32)


def scan_matches(out, x, n):
    return same(out[:n + 1], R.scan_ref(x)) and is_canary(out[n + 1:])


@gpu
@pytest.mark.parametrize("n", SCAN_NS)
def test_scan(n):
    for kind, x in scan_values(n):
        out = can(n + EXTRA + 1, U32)
        run("scan", **{"in": x}, out=out, n=n, n_buf=n + EXTRA)
        assert scan_matches(out, x, n), kind


# ------------------------------------------------------------------ SORT
SORT_NS = [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]


def sort_keys(n):
    rng = rng_for("sort", n)
    base = U64(0x0123456789ABCD00)
    yield "random", rng.integers(0, 1 << 64, n, dtype=np.uint64)
    yield "equal", np.full(n, base, U64)
    yield "two", np.where(rng.random(n) < 0.5, base, U64(0xFEDCBA9876543210)).astype(U64)
    yield "low byte", base | rng.integers(0, 256, n, dtype=np.uint64)
    yield "high byte", (rng.integers(0, 256, n, dtype=np.uint64) << U64(56)) | U64(0x00ABCDEF01234567)
    by = rng.integers(0, 2, (n, 8), dtype=np.uint64) * U64(255)
    yield "digits 0 and 255", (by << (U64(8) * np.arange(8, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def sort_run(key, row, tf, by_row=0, row_bits=0):
    key, row, tf = key.copy(), row.copy(), tf.copy()
    run("sort", key=key, row=row, tf=tf, n=len(key), by_row=by_row, row_bits=row_bits)
    return key, row, tf


def records_match(got, want):
    return all(same(g, w) for g, w in zip(got, want))


@gpu
@pytest.mark.parametrize("n", SORT_NS)
def test_sort_by_key(n):
    """tf = the arrival index: equal keys must come out in arrival order."""
    rng = rng_for("rows", n)
    row, tf = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32), np.arange(n, dtype=U32)
    for kind, key in sort_keys(n):
        assert records_match(sort_run(key, row, tf), R.sort_ref(key, row, tf)), kind


@gpu
@pytest.mark.parametrize("n", SORT_NS)
def test_sort_by_row(n):
    rng = rng_for("by row", n)
    key, tf = rng.integers(0, 1 << 64, n, dtype=np.uint64), np.arange(n, dtype=U32)
    for row_bits in (0, 8, 16, 24, 32):
        for hi in sorted({1 << row_bits, min(3, 1 << row_bits)}):              # the whole range, and few distinct rows: long equal runs
            row = rng.integers(0, hi, n, dtype=np.uint64).astype(U32)
            assert records_match(sort_run(key, row, tf, 1, row_bits), R.sort_ref(key, row, tf, 1, row_bits)), (row_bits, hi)


@gpu
@pytest.mark.parametrize("n,nq", [(257, 2), (TILE + 1, 256), (TILE + 1, 257), (3 * TILE + 1, 65537)])
def test_sort_key_then_row_as_query_terms_does(n, nq):
    rng = rng_for("two sorts", n, nq)
    key = rng.integers(0, 1 << 64, 40, dtype=np.uint64)[rng.integers(0, 40, n)]
    row, tf = rng.integers(0, nq, n).astype(U32), np.arange(n, dtype=U32)
    row[:2] = (0, nq - 1)
    row_bits = 0
    while (1 << row_bits) < nq:
        row_bits += 8
    got = sort_run(*sort_run(key, row, tf), 1, row_bits)
    assert records_match(got, R.query_sort_ref(key, row, tf, nq))
    assert np.array_equal(np.lexsort((got[2], got[0], got[1])), np.arange(n))          # (query, key, arrival) order


# ------------------------------------------------------------------ RLE
RLE_NS = [0, 1, 255, 256, 257, TILE + 1]
RLE_OUT = {"ukeys": U64, "pstart": U32, "prow": U32, "ptf": U32, "pkey": U64}


def rle_records(kind, n):
    """Sorted (key, row) records: all one posting, every record a posting of its own, or runs of 11 records, offset so that one
    straddles record 256 and one record 4 096.  Three postings per key at rows 5k, 5k + 2, 5k + 5: an equal key with different
    rows, and the first posting of a key repeats the row of the posting before it (an equal row under adjacent different keys)."""
    rng = rng_for("rle", kind, n)
    i = np.arange(n, dtype=np.int64)
    if kind == "identical":
        post = np.zeros(n, np.int64)
    elif kind == "distinct":
        post = i
    else:
        post = (i + 5) // 11
    key = (U64(1) << U64(40)) * (post // 3).astype(U64) + U64(7)
    row = (5 * (post // 3) + np.array([0, 2, 5])[post % 3]).astype(U32)
    return key, row, rng.integers(1, 9, n).astype(U32)


def rle_run(key, row, tf, unit, form):
    n = len(key)
    out = {name: can(n + EXTRA + (name == "pstart"), dt) for name, dt in RLE_OUT.items()}
    if form == "segment":
        out["pkey"] = None
    if form == "query":
        out["ukeys"] = out["pstart"] = None
    a = run("rle", key=key, row=row, tf=tf, n=n, unit=unit, post_buf=n + EXTRA, keys_buf=n + EXTRA, **out)
    return a.n_post, a.n_keys, out


def rle_matches(n_post, n_keys, out, want):
    if (n_post, n_keys) != (want["n_post"], want["n_keys"]):
        return False
    for name, v in out.items():
        if v is None:
            continue
        m = n_keys if name == "ukeys" else n_keys + 1 if name == "pstart" else n_post
        if not (same(v[:m], want[name]) and is_canary(v[m:])):
            return False
    return True


@gpu
@pytest.mark.parametrize("n", RLE_NS)
@pytest.mark.parametrize("unit", [0, 1])
def test_rle(n, unit):
    for kind in ("identical", "distinct", "runs"):
        key, row, tf = rle_records(kind, n)
        want = R.rle_ref(key, row, tf, unit)
        for form in ("segment", "query", "both"):
            n_post, n_keys, out = rle_run(key, row, tf, unit, form)
            assert rle_matches(n_post, n_keys, out, want), (kind, form)
            if form != "query":
                assert out["pstart"][n_keys] == n_post
        if kind == "identical" and n:
            assert want["n_post"] == 1 and want["ptf"][0] == (n if unit else tf[0])
        if kind == "runs" and n > TILE and unit:
            assert want["ptf"][(256 + 5) // 11] == 11 and want["ptf"][-1] == n - (TILE - 9)     # the run over record 256; the last run is cut short


# ------------------------------------------------------------------ FOLD
def part(rng, keys, row_lo, n_rows, n_tokens):
    """A segment over rows [row_lo, row_lo + n_rows) built by the reference from n_tokens random tokens (repeats: tf > 1)."""
    key = keys[rng.integers(0, len(keys), n_tokens)] if n_rows else np.zeros(0, U64)
    row = np.sort(rng.integers(row_lo, row_lo + max(n_rows, 1), len(key))).astype(U32)
    return R.build_segment_ref(key, row, np.ones(len(key), U32), 1, row_lo, n_rows)


def fold_parts(layout):
    """layout: tokens per part (0 = a part without postings).  Keys: a shared pool, and a private pool per part."""
    rng = rng_for("fold", layout)
    shared = rng.integers(1, 1 << 64, 30, dtype=np.uint64)
    parts, row_lo = [], 0
    for i, t in enumerate(layout):
        own = rng.integers(1, 1 << 64, 10, dtype=np.uint64)
        n_rows = 0 if t == 0 and i % 2 else max(8, t // 4)       # an empty part with and without rows of its own
        parts.append(part(rng, np.concatenate([shared, own]), row_lo, n_rows, t))
        row_lo += n_rows
    return parts


def fold_run(parts):
    total = sum(len(p["prow"]) for p in parts)
    out = {"ukeys": can(total + EXTRA, U64), "pstart": can(total + EXTRA + 1, U32), "prow": can(total + EXTRA, U32),
           "ptf": can(total + EXTRA, U32)}
    a = run("fold", segs=parts, post_buf=total + EXTRA, keys_buf=total + EXTRA, **out)
    return a.n_post, a.n_keys, out


def fold_matches(n_post, n_keys, out, want):
    return rle_matches(n_post, n_keys, out, {"n_post": len(want["prow"]), "n_keys": len(want["keys"]), "ukeys": want["keys"],
                                            "pstart": want["pstart"], "prow": want["prow"], "ptf": want["ptf"]})


FOLD_LAYOUTS = [(300, 200), (300, 200, 100), (0, 300), (300, 0, 200), (300, 200, 0), (0, 0), (2700, 1900), (1500, 1400, 1300, 1200)]


@gpu
@pytest.mark.parametrize("layout", FOLD_LAYOUTS, ids=str)
def test_fold(layout):
    parts = fold_parts(layout)
    want = R.fold_ref(parts)
    if sum(layout) > 4000:
        assert sum(len(p["prow"]) for p in parts) > TILE                               # more than one sort tile
    if sum(layout):
        assert want["ptf"].max() > 1 and len(want["keys"]) > 30                         # tf carried; shared and private keys
    n_post, n_keys, out = fold_run(parts)
    assert fold_matches(n_post, n_keys, out, want)


# ------------------------------------------------------------------ STATS
STATS_ROWS = [1, 63, 64, 65, 256, 257, TILE + 1]
POSTING_COUNTS = [0, 1, 63, 64, 65, 1000]


def stats_segments(rng, n_rows, n_segs, n_single=0):
    """Segments over consecutive halves of the rows.  Keys with 0, 1, 63, 64, 65 and 1 000 postings (as many as the segment has
    rows), then n_single keys of one posting."""
    edges = [0, n_rows] if n_segs == 1 else [0, n_rows // 2, n_rows]
    segs = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        counts = [min(c, hi - lo) for c in POSTING_COUNTS]
        rows = [np.sort(rng.choice(hi - lo, c, replace=False)) + lo for c in counts]
        if n_single and hi > lo:
            counts += [1] * n_single
            rows.append(rng.integers(lo, hi, n_single))
        segs.append({"keys": np.arange(1, len(counts) + 1, dtype=U64) * U64(1000003),
                     "pstart": np.concatenate([[0], np.cumsum(counts)]).astype(U32),
                     "prow": (np.concatenate(rows) if rows else np.zeros(0)).astype(U32), "row_lo": lo, "n_rows": hi - lo})
        segs[-1]["ptf"] = np.ones(len(segs[-1]["prow"]), U32)
    return segs


def live_words(kind, rng, n):
    b = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "one": np.arange(n) == n // 2, "random": rng.random(n) < 0.5}[kind]
    return R.words_of(b)


def stats_run(dl, live, segs, k1, b, corpus=None):
    n = len(dl)
    acc, kd = np.zeros(2, U64), can(n + EXTRA, F32)
    for g in segs:
        g["df"] = can(len(g["keys"]), U32)
    run("stats", segs=segs, dl=dl, live=live, acc=acc, kd=kd, n_rows=n, rows_buf=n + EXTRA, k1=k1, b=b,
        corpus_n=corpus[0] if corpus else 0, corpus_sum_dl=corpus[1] if corpus else 0)
    return acc, kd, [g["_df"] for g in segs]


def stats_match(got, want, n):
    acc, kd, dfs = got
    (n_live, sum_dl), kd_w, dfs_w = want
    return (int(acc[0]), int(acc[1])) == (n_live, sum_dl) and same(kd[:n], kd_w) and is_canary(kd[n:]) and \
        len(dfs) == len(dfs_w) and all(same(a, b) for a, b in zip(dfs, dfs_w))


@gpu
@pytest.mark.parametrize("n_rows", STATS_ROWS)
@pytest.mark.parametrize("live_kind", ["all", "none", "one", "random"])
def test_stats(n_rows, live_kind):
    rng = rng_for("stats", n_rows, live_kind)
    live = live_words(live_kind, rng, n_rows)
    small = rng.integers(0, 40, n_rows).astype(U32)                       # zeros among them
    large = rng.integers(1 << 30, 1 << 32, n_rows, dtype=np.uint64).astype(U32)
    cases = [(small, None, 1), (large, None, 2), (small, (1000, 23456), 2), (large, (3, 1 << 34), 1), (np.zeros(n_rows, U32), None, 1)]
    for i, (dl, corpus, n_segs) in enumerate(cases):
        segs = stats_segments(rng, n_rows, n_segs)
        want = R.stats_ref(dl, live, segs, 1.2, 0.75, corpus)
        assert stats_match(stats_run(dl, live, segs, 1.2, 0.75, corpus), want, n_rows), i
    if live_kind == "all" and n_rows >= 8:
        assert int(large.astype(np.int64).sum()) > 1 << 32


@gpu
def test_stats_more_keys_than_the_df_grid_has_waves():
    """16 385 single-posting keys behind the six others: df_kernel's grid stops at 4 096 workgroups of 4 waves and wraps."""
    rng = rng_for("df wrap")
    n_rows = TILE + 1
    live = live_words("random", rng, n_rows)
    dl = rng.integers(0, 40, n_rows).astype(U32)
    segs = stats_segments(rng, n_rows, 1, n_single=16385)
    assert len(segs[0]["keys"]) > 4 * 4096
    assert stats_match(stats_run(dl, live, segs, 0.9, 0.4), R.stats_ref(dl, live, segs, 0.9, 0.4), n_rows)


# ------------------------------------------------------------------ LOOKUP
def lookup_segments(n_segs):
    """Segments of 50, 1, 0 and 20 keys (in that order, the first n_segs): even keys in segment 0, multiples of 3 in segment 3."""
    all_keys = [np.arange(100, 200, 2), np.array([150]), np.zeros(0), np.arange(99, 159, 3)]
    segs, lo = [], 0
    for s in range(n_segs):
        keys = all_keys[s].astype(U64) << U64(33)
        segs.append({"keys": keys, "pstart": np.arange(len(keys) + 1, dtype=U32), "prow": (np.arange(len(keys)) + lo).astype(U32),
                     "ptf": np.ones(len(keys), U32), "df": (np.arange(len(keys)) * 7 + s + 1).astype(U32), "row_lo": lo, "n_rows": len(keys)})
        lo += len(keys)
    return segs


def lookup_run(segs, qkeys, with_df):
    n = len(qkeys)
    tu, df = can((n + EXTRA) * 4, np.int32), can(n + EXTRA, np.int64) if with_df else None
    run("lookup", segs=segs, qkeys=qkeys, tu=tu, df_out=df, n_terms=n, terms_buf=n + EXTRA)
    return tu.reshape(-1, 4), df


def lookup_matches(tu, df, want_tu, want_df, n):
    return same(tu[:n], want_tu) and is_canary(tu[n:]) and (df is None or (same(df[:n], want_df) and is_canary(df[n:])))


@gpu
@pytest.mark.parametrize("n_segs", [1, 2, 3, 4])
@pytest.mark.parametrize("with_df", [False, True])
def test_lookup(n_segs, with_df):
    segs = lookup_segments(n_segs)
    q = np.array([0, 99, 100, 101, 102, 150, 156, 198, 199, 200, (1 << 31) - 1], U64) << U64(33)   # below, first, between, shared, last, above
    q = np.concatenate([q, np.array([1, (1 << 64) - 1], U64), np.arange(90, 210, dtype=U64) << U64(33)])   # 133 terms
    want_tu, want_df = R.lookup_ref(segs, q)
    assert (want_tu >= 0).any(axis=0).tolist() == [True, n_segs > 1, False, n_segs > 3]
    tu, df = lookup_run(segs, q, with_df)
    assert lookup_matches(tu, df, want_tu, want_df, len(q))


# ------------------------------------------------------------------ SCORE
def split_segments(postings, edges):
    """postings: {key: (rows ascending, tf)} over the whole row range -> one segment per [edges[i], edges[i + 1])."""
    segs = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        keys, pstart, prow, ptf = [], [0], [], []
        for key in sorted(postings):
            rows, tf = postings[key]
            m = (rows >= lo) & (rows < hi)
            if m.any():
                keys.append(key)
                prow.append(rows[m])
                ptf.append(tf[m])
                pstart.append(pstart[-1] + int(m.sum()))
        segs.append({"keys": np.array(keys, U64), "pstart": np.array(pstart, U32), "prow": np.concatenate(prow + [np.zeros(0)]).astype(U32),
                     "ptf": np.concatenate(ptf + [np.zeros(0)]).astype(U32), "row_lo": lo, "n_rows": hi - lo})
    return segs


def layouts(n_rows):
    """One segment; main + tail with the boundary inside a block and on a block edge; four segments."""
    out = {"one": [0, n_rows]}
    if n_rows >= 2:
        out["inside"] = [0, n_rows - max(1, n_rows // 3), n_rows]
    if n_rows > R.FT_ROWS:
        out["edge"] = [0, R.FT_ROWS, n_rows]
    if n_rows >= 4:
        out["four"] = [0, n_rows // 5, n_rows // 2, n_rows - 1, n_rows]
    return out


def score_corpus(rng, n_rows, kk):
    """Keys by the rows they hit in block 0 (and every other block gets far fewer): 1 = every row, 2..8 = 1, 2, 3, kk - 1, kk, kk + 1
    and 100 rows of block 0 only, 9 = a random third of all rows, 10 = every 7th row.  tf in {1, 2}; K_d takes three values: equal
    scores by the hundred."""
    first = min(n_rows, R.FT_ROWS)
    post = {1: np.arange(n_rows)}
    for key, c in zip(range(2, 9), (1, 2, 3, kk - 1, kk, kk + 1, 100)):
        post[key] = np.sort(rng.choice(first, min(c, first), replace=False))
    post[9] = np.nonzero(rng.random(n_rows) < 0.33)[0]
    post[10] = np.arange(0, n_rows, 7)
    post = {U64(k) << U64(40): (r.astype(np.int64), rng.integers(1, 3, len(r)).astype(U32)) for k, r in post.items() if len(r)}
    kd = np.array([0.5, 1.25, 2.0], F32)[rng.integers(0, 3, n_rows)]
    return post, kd


DESIGNED = [[1], [], [2], [3], [4], [5], [6], [7], [8], [1, 9], [9, 10], [(10, 0.0), 3], [(1, 0.0)], [2, 3, 4, 8, 9, 10], [11], [11, 6]]


def score_batch(rng, nq):
    """nq queries as lists of (key number, weight): the designed ones first (nq = 1: every row; nq = 3: every row, no term,
    kk + 1 rows), then random mixes.  Key 11 is in no segment; a weight of 0 contributes nothing."""
    qs = {1: [[1]], 3: [[1], [], [7]]}.get(nq) or (DESIGNED + [sorted(rng.choice(np.arange(1, 12), int(rng.integers(1, 5)), replace=False).tolist())
                                                             for _ in range(nq - len(DESIGNED))])[:nq]
    out = []
    for q in qs:
        out.append([(t, float(F32(rng.uniform(0.1, 4.0)))) if not isinstance(t, tuple) else t for t in q])
    return out


def score_inputs(segs, batch):
    q_indptr = np.concatenate([[0], np.cumsum([len(q) for q in batch])]).astype(np.int64)
    qk = np.array([U64(t) << U64(40) for q in batch for t, _w in q], U64)
    w = np.array([wt for q in batch for _t, wt in q], F32)
    tu, _df = R.lookup_ref(segs, qk)
    return q_indptr, np.ascontiguousarray(tu.reshape(-1)), w


def score_run(segs, q_indptr, tu, w, kd, live, allow, allow_rows, n_rows, kk, bound=None):
    nq = len(q_indptr) - 1
    n_blocks = (n_rows + R.FT_ROWS - 1) // R.FT_ROWS
    cand = can(n_blocks * nq * kk + EXTRA, U64)
    run("score", segs=segs, q_indptr=q_indptr, tu=tu, w=w, kd=kd, live=live, allow=allow, allow_rows=allow_rows, n_rows=n_rows,
        n_terms=len(w), nq=nq, kk=kk, k1p1=F32(1.2) + F32(1), bound=bound, cand=cand, cand_buf=len(cand))
    return cand


def score_matches(cand, want):
    return same(cand[:want.size].reshape(want.shape), want) and is_canary(cand[want.size:])


K1P1 = F32(1.2) + F32(1)


@gpu
@pytest.mark.parametrize("n_rows", [1, R.FT_ROWS - 1, R.FT_ROWS, R.FT_ROWS + 1, 2 * R.FT_ROWS + 1])
@pytest.mark.parametrize("nq", [1, 3, 257])
@pytest.mark.parametrize("kk", [1, 5, 64])
def test_score(n_rows, nq, kk):
    rng = rng_for("score", n_rows, nq, kk)
    post, kd = score_corpus(rng, n_rows, kk)
    batch = score_batch(rng, nq)
    live = R.words_of(rng.random(n_rows) < 0.9)
    allow = R.words_of(rng.random(n_rows) < 0.8)
    allow_rows = max(1, n_rows - 37)                                     # below the row count and no multiple of 32
    for i, (name, edges) in enumerate(layouts(n_rows).items()):
        segs = split_segments(post, edges)
        q_indptr, tu, w = score_inputs(segs, batch)
        filt = (allow[:(allow_rows + 31) // 32].copy(), allow_rows) if (i + nq) % 2 else (None, 0)
        want = R.score_ref(segs, q_indptr, tu, w, kd, live, filt[0], filt[1], n_rows, K1P1, kk)
        cand = score_run(segs, q_indptr, tu, w, kd, live, filt[0], filt[1], n_rows, kk)
        assert score_matches(cand, want), name


def hit_case(kk):
    """8 193 rows, every row live, one K_d and tf = 1 everywhere: the hits of a query tie and come out by row."""
    rng = rng_for("hits", kk)
    n_rows = 2 * R.FT_ROWS + 1
    post, _kd = score_corpus(rng, n_rows, kk)
    post = {k: (r, np.ones(len(r), U32)) for k, (r, _tf) in post.items()}
    batch = [[(t, 1.5) for t in q] for q in ([1], [2], [3], [4], [5], [6], [7], [], [11])]
    segs = split_segments(post, [0, 5000, n_rows])
    return n_rows, segs, batch, np.full(n_rows, 1.25, F32), R.words_of(np.ones(n_rows, bool))


@gpu
@pytest.mark.parametrize("kk", [5, 64])
def test_score_hit_counts_and_ties(kk):
    """0, 1, 2, 3, kk - 1, kk, kk + 1 and 4 096 hits in a block, all of one score."""
    n_rows, segs, batch, kd, live = hit_case(kk)
    q_indptr, tu, w = score_inputs(segs, batch)
    want = R.score_ref(segs, q_indptr, tu, w, kd, live, None, 0, n_rows, K1P1, kk)
    assert [(want[0, q] != 0).sum() for q in range(9)] == [kk, 1, 2, 3, kk - 1, kk, kk, 0, 0] and not want[1:, 1:].any()
    assert len({int(k) >> 32 for k in want[:, 0].ravel() if k}) == 1                  # one score: the order is by row
    rows = (0xFFFFFFFF - (want[0, 0] & U64(0xFFFFFFFF))).tolist()
    assert rows == list(range(kk))
    assert score_matches(score_run(segs, q_indptr, tu, w, kd, live, None, 0, n_rows, kk), want)


@gpu
def test_score_page_bound():
    """The paging case: the bound is a key from the middle of a block's hits (equal scores on both sides of it); a bound of 0
    admits nothing; no bound array = every hit."""
    kk = 5
    n_rows, segs, batch, kd, live = hit_case(kk)
    q_indptr, tu, w = score_inputs(segs, batch)
    nq = len(batch)
    full = R.score_ref(segs, q_indptr, tu, w, kd, live, None, 0, n_rows, K1P1, 64)
    bound = np.zeros(nq, U64)
    bound[0] = full[0, 0, 30]                       # 30 hits of block 0 are above it
    bound[1] = full[0, 1, 0]                        # the only hit is the bound itself: not below it
    bound[6] = full[0, 6, 2]
    bound[2] = U64((1 << 64) - 1)
    want = R.score_ref(segs, q_indptr, tu, w, kd, live, None, 0, n_rows, K1P1, kk, bound=bound)
    assert same(want[0, 0], full[0, 0, 31:36]) and not want[0, 1].any() and same(want[0, 6, :3], full[0, 6, 3:6]) and not want[:, 3:6].any()
    assert score_matches(score_run(segs, q_indptr, tu, w, kd, live, None, 0, n_rows, kk, bound=bound), want)


# ------------------------------------------------------------------ a whole index through the API
def dbg_text_lib():
    lib = _lib.load_debug()
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith("vrag_text_index_"):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def pack(texts):
    enc = [t.encode("utf-8") for t in texts]
    off = np.zeros(len(enc) + 1, np.int64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    return np.frombuffer(b"".join(enc) or b"\0", np.uint8), off


class Index:
    def __init__(self, k1=1.2, b=0.75):
        self.lib = dbg_text_lib()
        self.h = C.c_void_p()
        _lib.check_debug("vrag_text_index_create", self.lib.vrag_text_index_create(k1, b, 0, C.byref(self.h)))

    def close(self):
        self.lib.vrag_text_index_destroy(self.h)

    def add(self, texts, fold_all):
        buf, off = pack(texts)
        _lib.check_debug("vrag_text_index_add", self.lib.vrag_text_index_add(self.h, buf.ctypes.data, off.ctypes.data_as(_lib._LP), len(texts), fold_all))

    def read(self):
        s = _lib.DebugTextIndexState()
        _lib.check_debug("vrag_debug_text_index_read", self.lib.vrag_debug_text_index_read(self.h, C.byref(s)))
        n = s.n_rows
        out = {"n_live": s.n_live, "sum_dl": s.sum_dl, "dl": np.zeros(n, U32), "kd": np.zeros(n, F32), "live": np.zeros((n + 31) // 32, U32), "segs": []}
        for g in range(s.n_segs):
            seg = {"keys": np.zeros(s.n_keys[g], U64), "pstart": np.zeros(s.n_keys[g] + 1, U32), "prow": np.zeros(s.n_post[g], U32),
                   "ptf": np.zeros(s.n_post[g], U32), "df": np.zeros(s.n_keys[g], U32)}
            for name, v in seg.items():
                getattr(s, name)[g] = v.ctypes.data
            seg["row_lo"], seg["n_rows"] = s.row_lo[g], s.seg_rows[g]
            out["segs"].append(seg)
        s.dl, s.kd, s.live, s.with_data = out["dl"].ctypes.data, out["kd"].ctypes.data, out["live"].ctypes.data, 1
        _lib.check_debug("vrag_debug_text_index_read", self.lib.vrag_debug_text_index_read(self.h, C.byref(s)))
        return out

    def query_terms(self, texts, cap):
        buf, off = pack(texts)
        nq = len(texts)
        q_indptr, keys, counts, df = np.zeros(nq + 1, np.int64), np.zeros(cap, U64), np.zeros(cap, np.int32), np.zeros(cap, np.int64)
        n_live = C.c_int64()
        _lib.check_debug("vrag_text_index_query_terms", self.lib.vrag_text_index_query_terms(
            self.h, buf.ctypes.data, off.ctypes.data_as(_lib._LP), nq, cap, q_indptr.ctypes.data_as(_lib._LP), keys.ctypes.data,
            counts.ctypes.data_as(_lib._IP), df.ctypes.data_as(_lib._LP), C.byref(n_live)))
        n = int(q_indptr[nq])
        return q_indptr, keys[:n], counts[:n], df[:n], n_live.value

    def search(self, q_indptr, keys, w, k):
        nq = len(q_indptr) - 1
        scores, ids = np.zeros((nq, k), F32), np.zeros((nq, k), np.int64)
        _lib.check_debug("vrag_text_index_search", self.lib.vrag_text_index_search(
            self.h, q_indptr.ctypes.data_as(_lib._LP), keys.ctypes.data, w.ctypes.data_as(_lib._FP), nq, k, None, 0,
            scores.ctypes.data_as(_lib._FP), ids.ctypes.data_as(_lib._LP)))
        return scores, ids


def expected_state(row_keys, edges, live, k1, b, corpus=None):
    """The index's state from the term keys of its rows: one reference segment per [edges[i], edges[i + 1])."""
    dl = np.array([len(r) for r in row_keys], U32)
    segs = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        key = np.array([k for r in row_keys[lo:hi] for k in r], U64)
        row = np.repeat(np.arange(lo, hi), dl[lo:hi]).astype(U32)
        segs.append(R.build_segment_ref(key, row, np.ones(len(key), U32), 1, lo, hi - lo))
    words = R.words_of(live)
    (n_live, sum_dl), kd, dfs = R.stats_ref(dl, words, segs, k1, b, corpus)
    for g, df in zip(segs, dfs):
        g["df"] = df
    return {"n_live": n_live, "sum_dl": sum_dl, "dl": dl, "kd": kd, "live": words, "segs": segs}


def state_matches(got, want):
    if (got["n_live"], got["sum_dl"], len(got["segs"])) != (want["n_live"], want["sum_dl"], len(want["segs"])):
        return False
    if not all(same(got[n], want[n]) for n in ("dl", "kd", "live")):
        return False
    return all((g["row_lo"], g["n_rows"]) == (w["row_lo"], w["n_rows"]) and all(same(g[n], w[n]) for n in ("keys", "pstart", "prow", "ptf", "df"))
               for g, w in zip(got["segs"], want["segs"]))


@pytest.fixture(scope="module")
def small_corpus():
    texts, words, _flat, _lens = O.zipf_corpus(3000, vocab=150, mean_len=8, seed=11)
    texts[5] = ""                                                         # a row without a token
    return texts, words, [O.term_keys(t) for t in texts]


@gpu
def test_whole_index_state_after_every_kind_of_change(small_corpus):
    texts, _words, row_keys = small_corpus
    ix = Index()
    try:
        live = np.ones(0, bool)

        def step(a, b, fold_all, edges):
            nonlocal live
            ix.add(texts[a:b], fold_all)
            live = np.concatenate([live, np.ones(b - a, bool)])
            assert state_matches(ix.read(), expected_state(row_keys[:b], edges, live, 1.2, 0.75)), (a, b)

        step(0, 1200, 1, [0, 1200])                                        # one add, folded: the main segment
        step(1200, 1900, 0, [0, 1200, 1900])                               # no fold: a tail segment appears
        step(1900, 2300, 0, [0, 1200, 2300])                               # the second add joins the tail (fold of two parts)
        step(2300, 3000, 1, [0, 3000])                                     # fold_all: main + tail + new rows, three parts
        live = rng_for("live").random(3000) < 0.7
        words = R.words_of(live)
        _lib.check_debug("vrag_text_index_set_live", ix.lib.vrag_text_index_set_live(ix.h, words.ctypes.data, 3000))
        assert state_matches(ix.read(), expected_state(row_keys, [0, 3000], live, 1.2, 0.75))
        _lib.check_debug("vrag_text_index_set_corpus_stats", ix.lib.vrag_text_index_set_corpus_stats(ix.h, 123456, 1500000))
        assert state_matches(ix.read(), expected_state(row_keys, [0, 3000], live, 1.2, 0.75, corpus=(123456, 1500000)))
    finally:
        ix.close()


@pytest.fixture(scope="module")
def small_index(small_corpus):
    texts, words, row_keys = small_corpus
    ix = Index()
    ix.add(texts[:2000], 1)
    ix.add(texts[2000:], 0)
    yield ix, O.Bm25Oracle(row_keys), words
    ix.close()


def query_texts(words, nq, rng):
    """One- to three-word queries from the whole vocabulary, a word now and then twice, and unknown words."""
    out = []
    for _ in range(nq):
        ws = [words[int(i)] for i in rng.integers(0, len(words), int(rng.integers(1, 4)))]
        if rng.random() < 0.3:
            ws.append(ws[0].upper())
        if rng.random() < 0.1:
            ws.append("zzzunknownzzz")
        out.append(" ".join(ws))
    return out


def terms_match(got, oracle, queries):
    q_indptr, keys, counts, df, n_live = got
    if n_live != oracle.N:
        return False
    for q, text in enumerate(queries):
        k, c, _w = oracle.query_terms(O.term_keys(text))
        a, e = int(q_indptr[q]), int(q_indptr[q + 1])
        if not (same(keys[a:e], k) and counts[a:e].tolist() == c.tolist() and df[a:e].tolist() == [oracle.df(int(x)) for x in k]):
            return False
    return True


@gpu
@pytest.mark.parametrize("nq", [1, 2, 256, 257, 65537])
def test_query_terms_one_two_and_three_digit_passes(small_index, nq):
    ix, oracle, words = small_index
    rng = rng_for("query terms", nq)
    base = query_texts(words, min(nq, 300), rng)
    queries = [base[i % len(base)] for i in range(nq)]                      # 65 537 queries: 300 distinct texts, cycled
    got = ix.query_terms(queries, 5 * nq)
    if nq <= 300:
        assert terms_match(got, oracle, queries)
    else:
        first = terms_match((got[0][:301], got[1], got[2], got[3], got[4]), oracle, queries[:300])
        assert first and got[4] == oracle.N
        q_indptr, keys, counts, df, _n = got
        lens = np.diff(q_indptr)
        assert np.array_equal(lens, np.tile(lens[:300], nq // 300 + 1)[:nq])
        for q in (300, 65535, 65536):                                       # and the queries behind every 2^8 / 2^16 boundary
            a, e, a0 = int(q_indptr[q]), int(q_indptr[q + 1]), int(q_indptr[q % 300])
            assert same(keys[a:e], keys[a0:a0 + e - a]) and same(counts[a:e], counts[a0:a0 + e - a]) and same(df[a:e], df[a0:a0 + e - a])
        n300 = int(q_indptr[300])
        reps = np.concatenate([keys[:n300]] * (nq // 300 + 1))[:len(keys)]
        assert same(keys, reps)


def search_matches(scores, ids, oracle, queries, k):
    for q, text in enumerate(queries):
        rows, sc = oracle.search(O.term_keys(text), k)
        m = len(rows)
        if not (ids[q, :m].tolist() == rows.tolist() and same(scores[q, :m], sc.astype(F32)) and (ids[q, m:] == -1).all()
                and np.isneginf(scores[q, m:]).all()):
            return False
    return True


@gpu
def test_search_257_queries(small_index):
    ix, oracle, words = small_index
    queries = query_texts(words, 257, rng_for("search"))
    q_indptr, keys, counts, df, n_live = ix.query_terms(queries, 2000)
    idf = np.log(1.0 + (float(n_live) - df + 0.5) / (df + 0.5))
    w = (counts.astype(np.float64) * idf).astype(F32)
    scores, ids = ix.search(q_indptr, np.ascontiguousarray(keys), w, 10)
    assert search_matches(scores, ids, oracle, queries, 10)


# ------------------------------------------------------------------ refusals (nothing is launched)
@gpu
def test_refusals():
    x, out = np.ones(8, U32), can(20, U32)
    refused("n (", "scan", **{"in": x}, out=out, n=-1, n_buf=8)
    refused("n (", "scan", **{"in": x}, out=out, n=(1 << 22) + 1, n_buf=(1 << 22) + 1)
    refused("n_buf", "scan", **{"in": x}, out=out, n=8, n_buf=7)
    refused("scan needs", "scan", **{"in": x}, out=None, n=8, n_buf=8)
    key, row, tf = np.arange(8, dtype=U64), np.arange(8, dtype=U32), np.ones(8, U32)
    refused("sort needs", "sort", key=key, row=None, tf=tf, n=8)
    refused("row_bits", "sort", key=key, row=row, tf=tf, n=8, by_row=1, row_bits=12)
    refused("row_bits", "sort", key=key, row=row, tf=tf, n=8, by_row=1, row_bits=40)
    o = {"prow": can(16, U32), "ptf": can(16, U32)}
    refused("neither", "rle", key=key, row=row, tf=tf, n=8, post_buf=16, keys_buf=16, **o)
    refused("rle needs key", "rle", key=None, row=row, tf=tf, n=8, post_buf=16, keys_buf=16, pkey=can(16, U64), **o)
    refused("rle needs prow", "rle", key=key, row=row, tf=tf, n=8, post_buf=16, keys_buf=16, pkey=can(16, U64), prow=o["prow"])
    refused("come together", "rle", key=key, row=row, tf=tf, n=8, post_buf=16, keys_buf=16, ukeys=can(16, U64), **o)
    refused("post_buf", "rle", key=key, row=row, tf=tf, n=8, post_buf=7, keys_buf=16, pkey=can(16, U64), **o)
    refused("keys_buf", "rle", key=key, row=row, tf=tf, n=8, post_buf=16, keys_buf=7, pkey=can(16, U64), **o)
    assert all(is_canary(v) for v in o.values()) and is_canary(out)

    def seg(**kw):
        g = {"keys": np.array([5, 9], U64), "pstart": np.array([0, 2, 3], U32), "prow": np.array([0, 2, 1], U32), "ptf": np.ones(3, U32),
             "df": np.zeros(2, U32), "row_lo": 0, "n_rows": 3}
        g.update(kw)
        return g

    fo = {"ukeys": can(16, U64), "pstart": can(17, U32), "prow": can(16, U32), "ptf": can(16, U32), "post_buf": 16, "keys_buf": 16}
    refused("n_segs", "fold", segs=[], **fo)
    refused("fold needs", "fold", segs=[seg()], **dict(fo, ukeys=None))
    refused("count is negative", "fold", segs=[seg(n_rows=-1)], **fo)
    refused("pstart[0]", "fold", segs=[seg(pstart=np.array([1, 2, 3], U32))], **fo)
    refused("pstart[n_keys]", "fold", segs=[seg(pstart=np.array([0, 2, 2], U32))], **fo)
    refused("pstart decreases", "fold", segs=[seg(pstart=np.array([0, 4, 3], U32))], **fo)
    refused("outside", "fold", segs=[seg(prow=np.array([0, 3, 1], U32))], **fo)
    refused("strictly ascending", "fold", segs=[seg(prow=np.array([2, 2, 1], U32))], **fo)
    refused("does not follow", "fold", segs=[seg(), seg(row_lo=4)], **fo)
    refused("without a key", "fold", segs=[seg(n_keys=0, pstart=np.array([3], U32))], **fo)
    refused("post_buf", "fold", segs=[seg()], **dict(fo, post_buf=2))
    assert all(is_canary(v) for v in fo.values() if isinstance(v, np.ndarray))
    st = {"dl": np.ones(3, U32), "live": np.ones(1, U32), "acc": np.zeros(2, U64), "kd": can(8, F32), "n_rows": 3, "rows_buf": 8, "k1": 1.2, "b": 0.75}
    refused("reaches row", "stats", segs=[seg()], **dict(st, n_rows=2))
    refused("rows_buf", "stats", segs=[seg()], **dict(st, rows_buf=2))
    refused("n_rows", "stats", segs=[seg()], **dict(st, n_rows=0))
    refused("k1 >= 0", "stats", segs=[seg()], **dict(st, b=1.5))
    refused("k1 >= 0", "stats", segs=[seg()], **dict(st, k1=-1.0))
    refused("corpus pair", "stats", segs=[seg()], corpus_n=0, corpus_sum_dl=5, **st)
    refused("stats needs", "stats", segs=[seg()], **dict(st, dl=None))
    assert is_canary(st["kd"])
    lk = {"qkeys": np.array([5], U64), "tu": can(8, np.int32), "n_terms": 1, "terms_buf": 2}
    refused("n_terms", "lookup", segs=[seg()], **dict(lk, n_terms=0))
    refused("terms_buf", "lookup", segs=[seg()], **dict(lk, terms_buf=0))
    refused("null array", "lookup", segs=[seg(df=None)], **lk)
    refused("lookup needs", "lookup", segs=[seg()], **dict(lk, qkeys=None))
    refused("n_segs", "lookup", segs=[seg(row_lo=3 * i) for i in range(5)], **lk)
    assert is_canary(lk["tu"])
    sc = {"q_indptr": np.array([0, 1], np.int64), "tu": np.array([1, -1, -1, -1], np.int32), "w": np.ones(1, F32), "kd": np.ones(3, F32),
          "live": np.ones(1, U32), "n_rows": 3, "n_terms": 1, "nq": 1, "kk": 2, "k1p1": 2.2, "cand": can(4, U64), "cand_buf": 4}
    refused("nq (", "score", segs=[seg()], **dict(sc, nq=0))
    refused("nq (", "score", segs=[seg()], **dict(sc, nq=65536))
    refused("kk (", "score", segs=[seg()], **dict(sc, kk=65))
    refused("kk (", "score", segs=[seg()], **dict(sc, kk=0))
    refused("score needs q_indptr", "score", segs=[seg()], **dict(sc, cand=None))
    refused("score needs tu and w", "score", segs=[seg()], **dict(sc, w=None))
    refused("score: n_terms", "score", segs=[seg()], **dict(sc, n_terms=-1))
    refused("n_rows", "score", segs=[seg()], **dict(sc, n_rows=(1 << 22) + 1))
    refused("q_indptr[0]", "score", segs=[seg()], **dict(sc, q_indptr=np.array([1, 1], np.int64)))
    refused("q_indptr ends", "score", segs=[seg()], **dict(sc, q_indptr=np.array([0, 2], np.int64)))
    refused("q_indptr decreases", "score", segs=[seg()], **dict(sc, nq=2, q_indptr=np.array([0, 2, 1], np.int64)))
    refused("no key of that segment", "score", segs=[seg()], **dict(sc, tu=np.array([2, -1, -1, -1], np.int32)))
    refused("no key of that segment", "score", segs=[seg()], **dict(sc, tu=np.array([1, 0, -1, -1], np.int32)))
    refused("allow_rows", "score", segs=[seg()], allow=np.ones(1, U32), allow_rows=4, **sc)
    refused("cand_buf", "score", segs=[seg()], **dict(sc, cand_buf=1))
    refused("reaches row", "score", segs=[seg()], **dict(sc, n_rows=2))
    assert is_canary(sc["cand"])
    assert _lib.load_debug().vrag_debug_text_run(None, 0) == ERR_INVALID
    a = _lib.DebugTextArgs()
    a.op = 7
    assert _lib.load_debug().vrag_debug_text_run(C.byref(a), 0) == ERR_INVALID
    assert b"not a full-text stage" in _lib.load_debug().vrag_last_error()


# ------------------------------------------------------------------ CPU negative controls
def test_control_scan_rejects_a_lost_tile_carry():
    x = np.ones(TILE + 3, U32)
    out = np.concatenate([R.scan_ref(x), can(EXTRA, U32)])
    assert scan_matches(out, x, len(x))
    bad = out.copy()
    bad[TILE:len(x) + 1] -= U32(TILE)                                  # the second tile starts from 0 again
    assert not scan_matches(bad, x, len(x))
    bad = out.copy()
    bad[len(x) + 1] = 0                                                # one element behind the total
    assert not scan_matches(bad, x, len(x))


def test_control_sort_rejects_two_equal_key_records_swapped():
    key, row, tf = np.array([3, 1, 3, 2], U64), np.array([9, 8, 7, 6], U32), np.arange(4, dtype=U32)
    want = R.sort_ref(key, row, tf)
    assert records_match(want, R.sort_ref(key, row, tf))
    bad = [v.copy() for v in want]
    for v in bad:
        v[[2, 3]] = v[[3, 2]]                                          # both have key 3: sorted all the same, not stable
    assert np.array_equal(bad[0], want[0]) and not records_match(bad, want)


def test_control_rle_rejects_an_off_by_one_range_and_a_short_tf():
    key, row, tf = rle_records("runs", 300)
    want = R.rle_ref(key, row, tf, 1)

    def outs():
        return {n: np.concatenate([want[n], can(EXTRA, dt)]) for n, dt in RLE_OUT.items()}

    assert rle_matches(want["n_post"], want["n_keys"], outs(), want)
    bad = outs()
    bad["pstart"][3] += 1
    assert not rle_matches(want["n_post"], want["n_keys"], bad, want)
    bad = outs()
    bad["ptf"][want["n_post"] - 1] -= 1                                # the last run, short by one
    assert not rle_matches(want["n_post"], want["n_keys"], bad, want)
    assert not rle_matches(want["n_post"] - 1, want["n_keys"], outs(), want)


def test_control_fold_rejects_postings_left_in_part_order():
    parts = fold_parts((300, 200))
    want = R.fold_ref(parts)

    def outs(g):
        return {"ukeys": np.concatenate([g["keys"], can(EXTRA, U64)]), "pstart": np.concatenate([g["pstart"], can(EXTRA, U32)]),
                "prow": np.concatenate([g["prow"], can(EXTRA, U32)]), "ptf": np.concatenate([g["ptf"], can(EXTRA, U32)])}

    assert fold_matches(len(want["prow"]), len(want["keys"]), outs(want), want)
    bad = dict(want, ptf=np.ones_like(want["ptf"]))                    # tf not carried
    assert not fold_matches(len(want["prow"]), len(want["keys"]), outs(bad), want)
    u = int(np.nonzero(np.diff(want["pstart"].astype(int)) > 1)[0][0])
    bad = dict(want, prow=want["prow"].copy())
    a = int(want["pstart"][u])
    bad["prow"][[a, a + 1]] = bad["prow"][[a + 1, a]]                  # rows of one key out of order
    assert not fold_matches(len(want["prow"]), len(want["keys"]), outs(bad), want)


def test_control_stats_rejects_df_that_counts_dead_rows():
    rng = rng_for("control stats")
    n = 257
    dl, live = rng.integers(0, 40, n).astype(U32), live_words("random", rng, n)
    segs = stats_segments(rng, n, 2)
    want = R.stats_ref(dl, live, segs, 1.2, 0.75)

    def got(acc=None, kd=None, dfs=None):
        return (np.array(acc or want[0], U64), np.concatenate([want[1] if kd is None else kd, can(EXTRA, F32)]), dfs or want[2])

    assert stats_match(got(), want, n)
    assert not stats_match(got(dfs=[np.diff(g["pstart"]).astype(U32) for g in segs]), want, n)      # every posting counted
    assert not stats_match(got(acc=(want[0][0], want[0][1])), ((want[0][0], want[0][1] + (1 << 32)), want[1], want[2]), n)   # a 32-bit sum
    fused = want[1].copy()
    fused[3] = np.nextafter(fused[3], F32(np.inf))                                                   # one ulp: what an FMA would give
    assert not stats_match(got(kd=fused), want, n)


def test_control_lookup_rejects_the_insertion_point_for_an_absent_key():
    segs = lookup_segments(2)
    q = np.array([101, 150], U64) << U64(33)
    tu, df = R.lookup_ref(segs, q)
    assert tu[0].tolist() == [-1, -1, -1, -1] and tu[1].tolist() == [25, 0, -1, -1]
    pad_tu, pad_df = np.concatenate([tu, can(EXTRA * 4, np.int32).reshape(-1, 4)]), np.concatenate([df, can(EXTRA, np.int64)])
    assert lookup_matches(pad_tu, pad_df, tu, df, 2)
    bad = pad_tu.copy()
    bad[0, 0] = 1                                                      # where 101 would be inserted
    assert not lookup_matches(bad, pad_df, tu, df, 2)
    bad_df = pad_df.copy()
    bad_df[1] -= segs[1]["df"][0]                                      # the second segment's share left out
    assert not lookup_matches(pad_tu, bad_df, tu, df, 2)


def test_control_score_rejects_a_4095_row_block_and_ties_by_descending_row():
    kk = 5
    n_rows, segs, batch, kd, live = hit_case(kk)
    q_indptr, tu, w = score_inputs(segs, batch)
    want = R.score_ref(segs, q_indptr, tu, w, kd, live, None, 0, n_rows, K1P1, kk)
    pad = np.concatenate([want.ravel(), can(EXTRA, U64)])
    assert score_matches(pad, want)
    rows = np.arange(n_rows)
    keys = make_key(R.scores_ref(segs, tu.reshape(-1, 4)[:1], w[:1], kd, n_rows, K1P1), rows)
    bad = want.copy()
    bad[1, 0] = np.sort(keys[4095:8190])[::-1][:kk]                    # blocks of 4 095 rows: block 1 starts one row early
    assert not score_matches(np.concatenate([bad.ravel(), can(EXTRA, U64)]), want)
    bad = want.copy()
    bad[0, 0] = make_key(R.scores_ref(segs, tu.reshape(-1, 4)[:1], w[:1], kd, n_rows, K1P1)[:kk], rows[4095:4095 - kk:-1])   # highest rows first
    assert not score_matches(np.concatenate([bad.ravel(), can(EXTRA, U64)]), want)
    bad = want.copy()
    bad[0, 5, kk - 1] = 0                                              # kk hits, the last one dropped
    assert not score_matches(np.concatenate([bad.ravel(), can(EXTRA, U64)]), want)
