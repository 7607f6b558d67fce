"""`GpuVectorStore(filter_route="bitmap")` on CPU: the store's part of the filtered route -- the mask cut and packed again per
resident segment, rows beyond the mask, which queries take the second pass, the `want = min(k, n_pass)` tail, the option's
validation and the `comm.on_gpu` fallback -- against stand-in shard classes whose `search_filtered` answers from the exact
CPU oracle over the passing rows (tests/test_filter_route_gpu.py runs the same comparison through the C ABI)."""
import logging

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from oracle import topk_ref as T
from tests.sharded_store_cases import CpuDense, CpuSparse
from verbatim_rag_amd import vector_stores as vs

CALLS = []          # (kind, shard, number of queries, k, words, n_allow) of every search_filtered call


def _passing(words, n_allow, n_rows):
    """Rows r < min(n_allow, n_rows) whose bit is set, from the words alone (the contract of include/vrag_amd.h)."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    n = min(int(n_allow), n_rows)
    assert len(words) * 32 >= n_allow
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)
    return np.nonzero(bits)[0]


def _pad(s, i, k):
    pad = k - s.shape[1]
    return np.pad(s, ((0, 0), (0, pad)), constant_values=-np.inf), np.pad(i, ((0, 0), (0, pad)), constant_values=-1)


class FDense(CpuDense):
    def __len__(self):
        return len(self.rows)

    def search_filtered(self, queries, k, allow_words, n_allow, stream=None):
        q = np.asarray(queries, np.float32)
        CALLS.append(("dense", self, len(q), k, np.array(allow_words), int(n_allow)))
        rows = _passing(allow_words, n_allow, len(self.rows))
        kk = min(k, len(rows))
        if kk == 0:
            return np.full((len(q), k), -np.inf, np.float32), np.full((len(q), k), -1, np.int64)
        s, i = T.dense_topk(self.rows[rows], q, kk)
        return _pad(s, np.where(i >= 0, rows[np.where(i >= 0, i, 0)], -1), k)


class FSparse(CpuSparse):
    def __init__(self, vocab, indptr, indices, values, device=0):
        super().__init__(vocab, np.array(indptr), np.array(indices), np.array(values), device)
        self.n_docs = len(indptr) - 1

    def search_filtered(self, queries, k, allow_words, n_allow, stream=None):
        queries = list(queries)
        CALLS.append(("sparse", self, len(queries), k, np.array(allow_words), int(n_allow)))
        rows = _passing(allow_words, n_allow, self.n_docs)
        kk = min(k, len(rows))
        if kk == 0:
            return np.full((len(queries), k), -np.inf, np.float32), np.full((len(queries), k), -1, np.int64)
        s, i = T.sparse_topk(*vs.csr_take_rows(*self.csr, rows), self.vocab, *vs.dicts_to_csr(queries), kk)
        return _pad(s, np.where(i >= 0, rows[np.where(i >= 0, i, 0)], -1), k)


N, DIM, VOCAB = 403, 64, 300


def _data(seed=5, n=N):
    rng = np.random.default_rng(seed)
    dense = (rng.integers(0, 2, (n, DIM)) * 2 - 1).astype(np.float32) / np.float32(8.0)      # unit rows stay dyadic: exact ties
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 9, replace=False), rng.integers(1, 64, 9) / 64)} for _ in range(n)]
    return dense, sparse


def _add(st, dense, sparse, a, b):
    st.add_vectors([f"id{i}" for i in range(a, b)], dense[a:b].tolist(), sparse[a:b], [f"text {i}" for i in range(a, b)],
                   [f"enh {i}" for i in range(a, b)], [{"document_id": f"d{i % 50}", "half": i % 2, "n": i} for i in range(a, b)])


@pytest.fixture()
def stand_ins(monkeypatch):
    from verbatim_rag_amd.distributed import merge_topk

    monkeypatch.setattr(vs._lib, "load", lambda: None)
    monkeypatch.setattr(vs._lib, "require_gpu", lambda: None)
    monkeypatch.setattr(vs, "DenseShard", FDense)
    monkeypatch.setattr(vs, "SparseShard", FSparse)
    monkeypatch.setattr(vs, "_merge_parts", lambda scores, rows, k, device: merge_topk(scores, rows, k))
    CALLS.clear()
    yield
    CALLS.clear()


def _pair(**kw):
    dense, sparse = _data()
    stores = []
    for route in ("subset", "bitmap"):
        st = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_route=route, **kw)
        _add(st, dense, sparse, 0, N - 40)
        st.query(dense_query=dense[0].tolist(), top_k=1, search_type="dense")        # flush: the main segments
        st.query(sparse_query=sparse[0], top_k=1, search_type="sparse")
        _add(st, dense, sparse, N - 40, N)                                             # a sparse tail segment at row 363
        stores.append(st)
    return stores[0], stores[1], dense, sparse


def _dump(per_q):
    return [[(r.id, r.score, r.text, sorted(r.metadata.items())) for r in rs] for rs in per_q]


FILTERS = ['metadata["document_id"] == "d7"', 'metadata["n"] in [0, 1, 2, 3, 5, 8, 362, 363, 364, 402]', 'metadata["half"] == 1', None]


@pytest.mark.parametrize("length", [0, 1, 31, 32, 33, 1000])
def test_bitmap_words_agree_with_the_mask(length):
    rng = np.random.default_rng(length)
    for mask in (rng.random(length) < 0.5, np.ones(length, bool), np.zeros(length, bool)):
        words = vs._bitmap(mask)
        assert words.dtype == np.uint32 and len(words) == (length + 31) // 32
        for r in range(length):
            assert bool((int(words[r // 32]) >> (r % 32)) & 1) == bool(mask[r])
        assert sum(bin(int(w)).count("1") for w in words) == int(mask.sum())          # no bit behind the last row
        assert _passing(words, length, length).tolist() == np.nonzero(mask)[0].tolist()


def test_filter_route_is_validated(stand_ins, tmp_path):
    for bad in ("bitmaps", "", None, 1):
        with pytest.raises(ValueError, match="filter_route"):
            vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_route=bad)
    st = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB)
    assert st.filter_route == "subset" and st._filter_route == "subset"
    dense, sparse = _data(n=20)
    _add(st, dense, sparse, 0, 20)
    st.save(str(tmp_path / "s"))
    assert "filter_route" not in open(tmp_path / "s" / "store.json").read()        # a run-time choice, not part of a saved store
    with pytest.raises(ValueError, match="filter_route"):
        vs.GpuVectorStore.load(str(tmp_path / "s"), filter_route="nope")
    assert vs.GpuVectorStore.load(str(tmp_path / "s")).filter_route == "subset"
    assert vs.GpuVectorStore.load(str(tmp_path / "s"), filter_route="bitmap")._filter_route == "bitmap"


class _FakeComm:
    def __init__(self, on_gpu):
        self.rank, self.world, self.on_gpu = 0, 1, on_gpu


def test_a_gpu_exchange_keeps_the_subset_route(stand_ins, caplog):
    with caplog.at_level(logging.INFO, logger=vs.logger.name):
        st = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, comm=_FakeComm(True), filter_route="bitmap")
    assert st.filter_route == "bitmap" and st._filter_route == "subset"
    said = [r for r in caplog.records if "filter_route" in r.getMessage()]
    assert len(said) == 1 and said[0].levelno == logging.INFO
    caplog.clear()
    with caplog.at_level(logging.INFO, logger=vs.logger.name):
        host = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, comm=_FakeComm(False), filter_route="bitmap")
        plain = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, comm=_FakeComm(True))
    assert host._filter_route == "bitmap" and plain._filter_route == "subset"
    assert not [r for r in caplog.records if "filter_route" in r.getMessage()]


def test_default_mode_never_calls_search_filtered(stand_ins):
    sub, _bm, dense, sparse = _pair()
    CALLS.clear()
    for flt in FILTERS:
        sub.query(dense_query=dense[3].tolist(), sparse_query=sparse[3], top_k=5, search_type="hybrid", filter=flt)
    sub.delete(["id3"])
    sub.query_batch(dense_queries=[dense[3].tolist()] * 2, top_k=5, search_type="dense")
    assert not CALLS and sub._subsets


def test_bitmap_route_equals_subset_route_and_builds_no_subset(stand_ins):
    sub, bm, dense, sparse = _pair()
    rng = np.random.default_rng(8)
    picks = [3, 362, 363, 402, 17, 200, 100]
    dq = [dense[i].tolist() for i in picks]
    sq = [sparse[i] for i in picks]
    for round_ in range(3):
        for flt in FILTERS:
            for kw in (dict(dense_queries=dq, search_type="dense", top_k=5), dict(sparse_queries=sq, search_type="sparse", top_k=7),
                       dict(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=4),
                       dict(dense_queries=dq, search_type="dense", top_k=70)):
                a, b = sub.query_batch(filter=flt, **kw), bm.query_batch(filter=flt, **kw)
                assert _dump(a) == _dump(b), (round_, flt, kw["search_type"], kw["top_k"])
                rest = {k: v for k, v in kw.items() if not k.endswith("_queries")}
                one = bm.query(dense_query=kw.get("dense_queries", [None])[0], sparse_query=kw.get("sparse_queries", [None])[0],
                               filter=flt, **rest)
                assert _dump([one]) == _dump(b[:1])
            assert not bm._subsets
        if round_ == 0:      # rows of the unfiltered top-k: the next unfiltered query is short as well
            gone = [r.id for r in bm.query(dense_query=dq[0], top_k=3, search_type="dense")] + ["id363", "id0"]
            sub.delete(gone), bm.delete(gone)
        if round_ == 1:
            more, more_sp = _data(seed=int(rng.integers(100)), n=30)
            for st in (sub, bm):
                st.add_vectors([f"new{i}" for i in range(30)], more.tolist(), more_sp, [f"t{i}" for i in range(30)], [""] * 30,
                               [{"document_id": "d7", "half": 1, "n": 1000 + i} for i in range(30)])
    assert any(c[0] == "dense" for c in CALLS) and any(c[0] == "sparse" for c in CALLS)
    assert len(bm._sparse_parts) == 2 and bm._sparse_parts[1][1] % 32 != 0             # the tail segment starts inside a word


def test_mask_is_cut_and_packed_again_at_every_segment_base(stand_ins):
    _sub, bm, dense, sparse = _pair()
    flt = 'metadata["n"] in [0, 1, 2, 3, 5, 8, 362, 363, 364, 402]'
    mask = bm._mask(flt)
    CALLS.clear()
    got = bm.query(sparse_query=sparse[363], top_k=10, search_type="sparse", filter=flt)
    assert {r.metadata["n"] for r in got} <= {0, 1, 2, 3, 5, 8, 362, 363, 364, 402} and got[0].id == "id363"
    assert [(sh, base) for sh, base, _n in bm._sparse_parts] == [(c[1], b) for c, b in zip(CALLS, (0, 363))]
    for (kind, shard, nq, k, words, n_allow), (_sh, base, n) in zip(CALLS, bm._sparse_parts):
        assert kind == "sparse" and n_allow == n == shard.n_docs
        assert np.array_equal(words, vs._bitmap(mask[base:base + n]))                   # bit 0 of word 0 = the segment's first row
        assert _passing(words, n_allow, n).tolist() == (np.nonzero(mask[base:base + n])[0]).tolist()
    CALLS.clear()
    bm.query(dense_query=dense[5].tolist(), top_k=10, search_type="dense", filter=flt)
    (kind, shard, nq, k, words, n_allow), = CALLS
    assert kind == "dense" and n_allow == N and np.array_equal(words, vs._bitmap(mask))


def test_rows_beyond_the_mask_do_not_pass(stand_ins):
    _sub, bm, dense, sparse = _pair()
    parts, _dev, n = bm._main_parts("sparse")
    assert n == N and len(parts) == 2
    short_mask = np.ones(370, dtype=bool)                  # built before rows 370 .. 402 were inserted: ends inside the tail segment
    CALLS.clear()
    scores, rows = bm._filtered_topk("sparse", parts, [sparse[400], sparse[365]], 5, short_mask)
    assert rows.max() < 370 and (rows[1] == 365).any() and not (rows == 400).any()
    assert [c[5] for c in CALLS] == [363, 40] and _passing(CALLS[1][4], 40, 40).tolist() == list(range(7))
    parts, _dev, n = bm._main_parts("dense")
    scores, rows = bm._filtered_topk("dense", parts, [dense[400].tolist()], N, short_mask)
    assert sorted(rows[0][rows[0] >= 0].tolist()) == list(range(370)) and (rows[0][370:] == -1).all()
    # and through the public path: a mask that is shorter than the store is padded with rows that do not pass
    r, _s = bm._topk_rows("dense", [dense[400].tolist()], 400, short_mask)
    assert sorted(r[0][r[0] >= 0].tolist()) == list(range(370))


def test_only_short_queries_take_the_second_pass(stand_ins):
    _sub, bm, dense, sparse = _pair()
    flt, k = 'metadata["half"] == 1', 2
    mask = bm._mask(flt)
    assert mask.sum() * 8 >= N                                               # the first pass is the full unfiltered one
    picks = list(range(0, 60))
    unit = bm._unit_queries([dense[i].tolist() for i in picks])
    _s, ids = T.dense_topk(bm._dense_rows.data, unit, k)
    short = [j for j in range(len(picks)) if mask[ids[j]].sum() < k]
    assert 0 < len(short) < len(picks)
    CALLS.clear()
    got = bm.query_batch(dense_queries=[dense[i].tolist() for i in picks], top_k=k, search_type="dense", filter=flt)
    (kind, shard, nq, kk, words, n_allow), = CALLS
    assert (kind, nq, kk) == ("dense", len(short), k)
    assert all(len(g) == k and all(r.metadata["half"] == 1 for r in g) for g in got)
    # a query that is not short keeps the first pass's rows: the passing prefix of the unfiltered ranking
    j = next(j for j in range(len(picks)) if j not in short)
    assert [r.id for r in got[j]] == [f"id{i}" for i in ids[j] if mask[i]][:k]


def test_the_second_pass_asks_for_min_k_and_passing_rows(stand_ins):
    _sub, bm, dense, sparse = _pair()
    flt = 'metadata["n"] in [4, 44, 363, 401]'
    CALLS.clear()
    got = bm.query(dense_query=dense[9].tolist(), top_k=10, search_type="dense", filter=flt)
    assert sorted(r.metadata["n"] for r in got) == [4, 44, 363, 401]
    assert [(c[0], c[2], c[3]) for c in CALLS] == [("dense", 1, 4)]           # k = want = min(10, 4 passing rows), no first pass
    rows, scores = bm._topk_rows("dense", [dense[9].tolist()], 10, bm._mask(flt))
    assert (rows[0, :4] >= 0).all() and (rows[0, 4:] == -1).all() and (scores[0, 4:] == 0).all()
    CALLS.clear()
    assert bm.query(dense_query=dense[9].tolist(), top_k=10, search_type="dense", filter='metadata["n"] == -1') == []
    assert not CALLS                                                           # nothing passes: no search at all


def test_the_filtered_and_the_unfiltered_route_are_one_loop(stand_ins):
    _sub, bm, dense, sparse = _pair()
    parts, _dev, n = bm._main_parts("sparse")
    assert n == N and len(parts) == 2                                          # main segment + the tail at row 363
    queries = [sparse[i] for i in (3, 362, 363, 402, 17)]
    for k in (1, 7, 70):
        plain_s, plain_r = bm._device_topk("sparse", parts, None, queries, k)
        CALLS.clear()
        filt_s, filt_r = bm._filtered_topk("sparse", parts, queries, k, np.ones(N, dtype=bool))
        assert len(CALLS) == 2 and plain_r.shape == (len(queries), k)
        assert np.array_equal(plain_r, filt_r) and (plain_r >= 363).any() and (plain_r < 363).any()
        assert plain_s.dtype == filt_s.dtype == np.float32 and plain_s.tobytes() == filt_s.tobytes()
