"""The references of tests/text_ref.py (what tests/test_text_unit_gpu.py compares the kernels of csrc/fulltext.hip with) against
brute force in Python integers and against Bm25Oracle (tests/full_text_oracle.py), on small random inputs.  No device."""
import itertools

import numpy as np
import pytest

import text_ref as R
from full_text_oracle import Bm25Oracle
from topk_ref import make_key

U64, U32, F32 = np.uint64, np.uint32, np.float32


def records(rng, n, n_keys, n_rows):
    key = rng.integers(0, 1 << 63, n_keys, dtype=np.uint64)[rng.integers(0, n_keys, n)] if n else np.zeros(0, U64)
    return key, rng.integers(0, n_rows, n).astype(U32), np.arange(n, dtype=U32)


@pytest.mark.parametrize("n", [0, 1, 2, 17, 300])
def test_scan_ref_is_the_running_sum_modulo_2_32(n):
    rng = np.random.default_rng(n)
    for x in (rng.integers(0, 1 << 16, n).astype(U32), np.full(n, 0xFFFFFFFF, U32)):
        want, s = [], 0
        for v in x.tolist():
            want.append(s)
            s = (s + v) & 0xFFFFFFFF
        assert R.scan_ref(x).tolist() == want + [s]


@pytest.mark.parametrize("n", [0, 1, 2, 65, 500])
def test_sort_ref_is_python_sorted(n):
    rng = np.random.default_rng(n)
    key, row, tf = records(rng, n, 7, 1 << 20)
    got = R.sort_ref(key, row, tf)
    want = sorted(zip(key.tolist(), row.tolist(), tf.tolist()), key=lambda r: r[0])      # sorted() is stable
    assert list(zip(*(g.tolist() for g in got))) == want
    for bits in (0, 8, 16, 24, 32):
        got = R.sort_ref(key, row, tf, 1, bits)
        want = sorted(zip(key.tolist(), row.tolist(), tf.tolist()), key=lambda r: r[1] & ((1 << bits) - 1))
        assert list(zip(*(g.tolist() for g in got))) == want
    got = R.query_sort_ref(key, row % U32(300), tf, 300)
    want = sorted(zip(key.tolist(), (row % U32(300)).tolist(), tf.tolist()), key=lambda r: (r[1], r[0]))
    assert list(zip(*(g.tolist() for g in got))) == want


@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 2, 40, 400])
def test_rle_ref_is_groupby(n, unit):
    rng = np.random.default_rng(n)
    key, row, _ = records(rng, n, 5, 6)
    order = np.lexsort((row, key))
    key, row = key[order], row[order]
    tf = rng.integers(1, 9, n).astype(U32)
    r = R.rle_ref(key, row, tf, unit)
    posts = [(k, rw, list(g)) for (k, rw), g in itertools.groupby(range(n), key=lambda i: (int(key[i]), int(row[i])))]
    assert r["n_post"] == len(posts) and r["pkey"].tolist() == [p[0] for p in posts] and r["prow"].tolist() == [p[1] for p in posts]
    assert r["ptf"].tolist() == [len(p[2]) if unit else int(tf[p[2][0]]) for p in posts]
    ukeys = [k for k, _g in itertools.groupby(p[0] for p in posts)]
    assert r["n_keys"] == len(ukeys) and r["ukeys"].tolist() == ukeys
    assert r["pstart"].tolist() == [[p[0] for p in posts].index(k) for k in ukeys] + [len(posts)]


def corpus(rng, n_rows, vocab=40, max_len=12):
    keys = np.sort(rng.integers(1, 1 << 63, vocab, dtype=np.uint64))
    return [keys[rng.integers(0, vocab, int(rng.integers(0, max_len)))].tolist() for _ in range(n_rows)], keys


def segment(row_keys, row_lo):
    dl = [len(r) for r in row_keys]
    key = np.array([k for r in row_keys for k in r], U64)
    row = np.repeat(np.arange(row_lo, row_lo + len(row_keys)), dl).astype(U32)
    return R.build_segment_ref(key, row, np.ones(len(key), U32), 1, row_lo, len(row_keys))


def assert_segment_is_oracle(seg, o):
    assert np.array_equal(seg["keys"], o.keys) and np.array_equal(seg["pstart"], np.append(o.start, len(o.p_row)))
    assert np.array_equal(seg["prow"], o.p_row) and np.array_equal(seg["ptf"], o.p_tf)


def test_build_and_fold_ref_give_the_oracles_postings():
    rng = np.random.default_rng(1)
    rows, _keys = corpus(rng, 90)
    o = Bm25Oracle(rows)
    assert_segment_is_oracle(segment(rows, 0), o)
    for cuts in ([30], [30, 60], [0, 30], [30, 30], [30, 90]):      # two and three parts, an empty one first / middle / last
        edges = [0] + cuts + [90]
        parts = [segment(rows[a:b], a) for a, b in zip(edges[:-1], edges[1:])]
        f = R.fold_ref(parts)
        assert_segment_is_oracle(f, o)
        assert (f["row_lo"], f["n_rows"]) == (0, 90)
    for p in parts:
        k, r, t = R.expand_ref(p)
        assert np.array_equal(R.rle_ref(k, r, t, 0)["ptf"], p["ptf"]) and len(k) == len(p["prow"])


@pytest.mark.parametrize("live_kind", ["all", "none", "random"])
def test_stats_and_lookup_ref_against_the_oracle(live_kind):
    rng = np.random.default_rng(2)
    rows, keys = corpus(rng, 70)
    o = Bm25Oracle(rows, 1.2, 0.75)
    live = {"all": np.ones(70, bool), "none": np.zeros(70, bool), "random": rng.random(70) < 0.6}[live_kind]
    o.set_live(live)
    segs = [segment(rows[:40], 0), segment(rows[40:], 40)]
    dl = np.array([len(r) for r in rows], U32)
    (n_live, sum_dl), kd, dfs = R.stats_ref(dl, R.words_of(live), segs, 1.2, 0.75)
    assert (n_live, sum_dl) == (o.N, int(o.dl[live].sum()))
    assert np.array_equal(kd.view(U32), o.kd.astype(F32).view(U32))
    for g, df in zip(segs, dfs):
        g["df"] = df
        assert df.tolist() == [int(live[g["prow"][a:e].astype(int)].sum()) for a, e in zip(g["pstart"][:-1], g["pstart"][1:])]
    q = np.concatenate([keys[:5], [U64(0), U64((1 << 64) - 1)], keys[-3:] + U64(1)])
    tu, df = R.lookup_ref(segs, q)
    assert df.tolist() == [o.df(int(k)) for k in q]
    for j, k in enumerate(q.tolist()):
        for s in range(4):
            want = segs[s]["keys"].tolist().index(k) if s < 2 and k in segs[s]["keys"].tolist() else -1
            assert tu[j, s] == want
    # the corpus-wide pair replaces the index's own in K_d only
    (n2, s2), kd2, _ = R.stats_ref(dl, R.words_of(live), segs, 1.2, 0.75, corpus=(1000, 7000))
    assert (n2, s2) == (n_live, sum_dl)
    assert np.array_equal(kd2.view(U32), (F32(1.2) * ((F32(1) - F32(0.75)) + F32(0.75) * (dl.astype(F32) / F32(7.0)))).view(U32))


def test_bits_round_trip():
    rng = np.random.default_rng(3)
    for n in (1, 31, 32, 33, 100):
        bits = rng.random(n) < 0.5
        assert np.array_equal(R.bits_of(R.words_of(bits), n), bits)


@pytest.mark.parametrize("segments", [1, 2, 4])
def test_score_ref_against_the_oracle(segments):
    """Blocks of one query merged = the oracle's search; the scores are its bits.  9 000 rows: three blocks."""
    rng = np.random.default_rng(4)
    n = 9000
    rows, keys = corpus(rng, n, vocab=30, max_len=6)
    o = Bm25Oracle(rows)
    live = rng.random(n) < 0.9
    o.set_live(live)
    allow = rng.random(n) < 0.7
    edges = np.linspace(0, n, segments + 1).astype(int)
    segs = [segment(rows[a:b], int(a)) for a, b in zip(edges[:-1], edges[1:])]
    dl = np.array([len(r) for r in rows], U32)
    _acc, kd, dfs = R.stats_ref(dl, R.words_of(live), segs, 1.2, 0.75)
    for g, df in zip(segs, dfs):
        g["df"] = df
    queries = [keys[[0, 3]].tolist(), [], [int(keys[5])] * 2 + [12345], keys[[7, 1, 2]].tolist()]
    terms = [o.query_terms(q) if q else (np.zeros(0, U64), None, np.zeros(0, F32)) for q in queries]
    q_indptr = np.concatenate([[0], np.cumsum([len(t[0]) for t in terms])]).astype(np.int64)
    qk = np.concatenate([t[0] for t in terms])
    w = np.concatenate([t[2] for t in terms]).astype(F32)
    tu, df = R.lookup_ref(segs, qk)
    assert df.tolist() == [o.df(int(k)) for k in qk]
    k = 20
    for allow_rows in (n, 5003):
        cand = R.score_ref(segs, q_indptr, tu, w, kd, R.words_of(live), R.words_of(allow), allow_rows, n, F32(1.2) + F32(1), k)
        mask = allow & (np.arange(n) < allow_rows)
        for qi, q in enumerate(queries):
            merged = np.sort(cand[:, qi].ravel())[::-1][:k]
            merged = merged[merged != 0]
            want_rows, want_scores = o.search(q, k, mask) if q else (np.zeros(0, int), np.zeros(0, F32))
            assert np.array_equal(merged, make_key(want_scores, want_rows))
    # the page bound: the second page of a query is what follows its first
    cand = R.score_ref(segs, q_indptr, tu, w, kd, R.words_of(live), None, 0, n, F32(2.2), 5)
    first = np.sort(cand[:, 0].ravel())[::-1][:5]
    bound = np.array([first[-1], 0, 0, 0], U64)
    page2 = R.score_ref(segs, q_indptr, tu, w, kd, R.words_of(live), None, 0, n, F32(2.2), 5, bound=bound)
    want_rows, want_scores = o.search(queries[0], 10)
    assert np.array_equal(np.sort(page2[:, 0].ravel())[::-1][:5], make_key(want_scores, want_rows)[5:])
    assert not page2[:, 1:].any()
