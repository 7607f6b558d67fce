"""index_type="PQ" on the host: the constructor's refusals and acceptances (checked before any device is touched), the store's
part with stand-in shards -- exact rows under `PQ_MIN_ROWS`, one training at it, frozen codebooks in every shard built afterwards,
the manifest -- and self-checks of tests/pq_ref.py, the reference the GPU tests compare bits with."""
import json
import os

import numpy as np
import pytest

import pq_ref as R
import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import vector_stores as VS


# ---------------------------------------------------------------------------------------------------------------- the constructor
def test_constructor_refusals_and_acceptances_need_no_device():
    with pytest.raises(ValueError, match="needs m"):
        VS.GpuVectorStore(dense_dim=64, index_type="PQ")
    with pytest.raises(ValueError, match="m must divide dense_dim"):
        VS.GpuVectorStore(dense_dim=64, index_type="PQ", m=24)
    with pytest.raises(ValueError, match="m must divide dense_dim"):
        VS.GpuVectorStore(dense_dim=None, index_type="PQ", m=8)
    for bad in (0, -4, 129, 8.0, True, "8"):
        with pytest.raises(ValueError, match="m must be an integer"):
            VS.GpuVectorStore(dense_dim=1032, index_type="PQ", m=bad)
    with pytest.raises(ValueError, match="at most 64 components"):
        VS.GpuVectorStore(dense_dim=1040, index_type="PQ", m=16)
    for bad in (4, 16, None, True):
        with pytest.raises(ValueError, match="nbits must be 8"):
            VS.GpuVectorStore(dense_dim=64, index_type="PQ", m=8, nbits=bad)
    for dtype in ("bf16", "int8"):
        with pytest.raises(ValueError, match="PQ.*dense_dtype='f32'"):
            VS.GpuVectorStore(dense_dim=64, index_type="PQ", m=8, dense_dtype=dtype)
    with pytest.raises(ValueError, match="PQ.*single-GPU.*keep FLAT"):
        VS.GpuVectorStore(dense_dim=64, index_type="PQ", m=8, distributed=True)
    with pytest.raises(ValueError, match="PQ.*single-GPU.*keep FLAT"):
        VS.GpuVectorStore(dense_dim=64, index_type="PQ", m=8, comm=object())
    with pytest.raises(ValueError, match="index_type must be .*'PQ'"):
        VS.GpuVectorStore(dense_dim=64, index_type="pq", m=8)
    with pytest.raises(ValueError, match="index_type must be .*'PQ'"):
        VS.GpuVectorStore(dense_dim=64, index_type="IVF_PQ", m=8)            # the follow-up, not this store
    with pytest.raises(ValueError, match="m is the number of sub-vectors of index_type='PQ'"):
        VS.GpuVectorStore(dense_dim=64, index_type="FLAT", m=8)
    VS.check_index_config("PQ", 8192, 16, False, 8, 8, 64)
    VS.check_index_config("PQ", 8192, 16, False, 128, 8, 4096)
    VS.check_index_config("PQ", 8192, 16, False, np.int64(96), np.int64(8), 768)
    VS.check_index_config("FLAT", 8192, 16, True)                            # the four-argument form of the other index types
    VS.check_dense_dtype("f32", "PQ", False)
    assert VS.IVF_INDEX_TYPES == ("IVF_FLAT", "IVF_SQ8") and VS.DENSE_DTYPES == ("f32", "bf16", "int8")
    assert VS.PQ_MIN_ROWS == 256 * VS.IVF_MIN_LIST_ROWS == 9984 and VS.PqShard.__name__ == "PqShard"


# ---------------------------------------------------------------------------------------------------------------- the store
def _dump(per_q):
    return [[(r.id, r.score) for r in rs] for rs in per_q]


def test_store_trains_once_and_hands_the_frozen_codebooks_to_every_shard(monkeypatch, tmp_path):
    from tests.sharded_store_cases import CpuDense
    from verbatim_rag_amd.distributed import merge_topk

    made = []

    class CpuPq(CpuDense):
        """Stand-in for `PqShard`: its constructor and codebook calls, exact fp32 answers (the route is what this test is about)."""
        ivf = None

        def __init__(self, dim, m, capacity, device=0):
            super().__init__(dim, capacity)
            self.dim, self.m, self.capacity, self.cb, self.calls = dim, m, capacity, None, []
            made.append(self)

        def train(self, rows, iters=10):
            rows = np.asarray(rows, np.float32)
            self.calls.append(("train", len(rows), iters))
            self.sample = rows.copy()
            self.cb = np.full((self.m, 256, self.dim // self.m), np.float32(len(rows)))

        def set_codebooks(self, cb):
            self.calls.append(("set_codebooks",))
            self.cb = np.array(cb, np.float32)

        def codebooks(self):
            return self.cb.copy()

        def add(self, rows):
            assert self.cb is not None, "rows before codebooks"
            super().add(rows)

        def __len__(self):
            return len(self.rows)

        def compact(self, keep):
            self.calls.append(("compact", len(keep)))
            self.rows = self.rows[np.asarray(keep, bool)]
            return len(self.rows)

    class CpuFlat(CpuDense):
        def __len__(self):
            return len(self.rows)

        def compact(self, keep):
            self.rows = self.rows[np.asarray(keep, bool)]
            return len(self.rows)

    monkeypatch.setattr(VS._lib, "load", lambda: None)
    monkeypatch.setattr(VS._lib, "require_gpu", lambda: None)
    monkeypatch.setattr(VS, "DenseShard", CpuFlat)
    monkeypatch.setattr(VS, "PqShard", CpuPq)
    monkeypatch.setattr(VS, "_merge_parts", lambda scores, rows, k, device: merge_topk(scores, rows, k))
    monkeypatch.setattr(VS, "PQ_MIN_ROWS", 300)
    monkeypatch.setattr(VS, "PQ_TRAIN_ROWS_MAX", 128)
    rng = np.random.default_rng(5)
    dim = 32

    def rows(a, b):
        dense = (rng.integers(0, 2, (b - a, dim)) * 2 - 1).astype(np.float32) / np.float32(8.0)
        return ([f"id{i}" for i in range(a, b)], dense, [None] * (b - a), [f"t{i}" for i in range(a, b)], [""] * (b - a),
                [{"document_id": f"d{i % 20}"} for i in range(a, b)])

    st = VS.GpuVectorStore(dense_dim=dim, enable_sparse=False, index_type="PQ", m=8)
    flat = VS.GpuVectorStore(dense_dim=dim, enable_sparse=False)
    assert (st.m, st.nbits) == (8, 8) and (flat.m, flat.nbits) == (None, None) and st._use_prefilter() == flat._use_prefilter()
    first = rows(0, 200)
    for s_ in (st, flat):
        s_.add_vectors(*first)
    dq = [first[1][i].tolist() for i in (3, 77)]
    # under the threshold: the exact shard, the FLAT store's answers, nothing trained
    assert st.pq_stats() is None and flat.pq_stats() is None and isinstance(st._dense, CpuFlat) and not made
    assert _dump(st.query_batch(dense_queries=dq, search_type="dense", top_k=5)) == _dump(flat.query_batch(dense_queries=dq, search_type="dense", top_k=5))
    flt = 'metadata["document_id"] == "d3"'
    st.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter=flt)
    assert not made                                                        # a subset of an untrained store is exact rows too
    # the flush that reaches it: one training on evenly strided host rows, the shard built from the host rows, swapped in
    batch = rows(200, 500)
    for s_ in (st, flat):
        s_.add_vectors(*batch)
    assert st.pq_stats() == {"m": 8, "rows": 500, "trained_rows": 128} and flat.pq_stats() is None
    trainer, shard = made
    assert trainer.calls == [("train", 128, VS.PQ_TRAIN_ITERS)] and VS.PQ_TRAIN_ITERS == 10 and len(trainer.rows) == 0
    unit = st._dense_rows.data[:500]
    assert np.array_equal(trainer.sample, unit[(np.arange(128) * 500) // 128])
    assert shard is st._dense and shard.calls == [("set_codebooks",)] and np.array_equal(shard.cb, trainer.cb) and len(shard) == 500
    assert np.array_equal(shard.rows, unit)
    frozen = st._pq_codebooks.copy()
    # later inserts are encoded by the resident shard; a rebuild for capacity and a filter subset get the frozen codebooks
    batch = rows(500, 600)
    for s_ in (st, flat):
        s_.add_vectors(*batch)
    assert st.pq_stats()["rows"] == 600 and st._dense is shard and len(made) == 2
    got = st.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter=flt)
    assert _dump(got) == _dump(flat.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter=flt))
    subset = made[2]
    assert len(made) == 3 and subset.calls == [("set_codebooks",)] and np.array_equal(subset.cb, frozen) and len(subset) == 30
    batch = rows(600, 1200)
    for s_ in (st, flat):
        s_.add_vectors(*batch)                                   # past 500 * dense_headroom: rebuilt
    assert st.pq_stats() == {"m": 8, "rows": 1200, "trained_rows": 128}
    rebuilt = made[3]
    assert len(made) == 4 and rebuilt is st._dense and rebuilt.calls == [("set_codebooks",)] and np.array_equal(rebuilt.cb, frozen)
    with pytest.raises(ValueError, match="grouping search .*index_type='PQ'"):
        st.query(dense_query=dq[0], search_type="dense", top_k=3, search_params={"group_by_field": "document_id"})
    # compact() goes to the shard
    for s_ in (st, flat):
        s_.delete([f"id{i}" for i in range(0, 1200, 4)])
        assert s_.compact() == 300
    assert rebuilt.calls[-1] == ("compact", 1200) and len(rebuilt) == 900 and st.pq_stats()["rows"] == 900
    # save / load: the manifest gains m / nbits for PQ alone, the codebooks come back and nothing trains again
    st.save(str(tmp_path / "pq"))
    flat.save(str(tmp_path / "flat"))
    head = json.load(open(os.path.join(tmp_path, "pq", "store.json")))
    assert (head["index_type"], head["m"], head["nbits"]) == ("PQ", 8, 8)
    flat_text = open(os.path.join(tmp_path, "flat", "store.json"), encoding="utf-8").read()
    assert list(json.loads(flat_text)) == ["format", "world", "dense_dim", "sparse_vocab", "enable_dense", "enable_sparse", "dense_dtype",
                                           "dense_prefilter", "enable_full_text", "bm25_k1", "bm25_b", "rows", "documents"]
    assert "pq_codebooks" not in np.load(os.path.join(tmp_path, "flat", "vectors.rank0.npz")).files
    ivf = VS.GpuVectorStore(dense_dim=dim, enable_sparse=False, index_type="IVF_FLAT")
    ivf.save(str(tmp_path / "ivf"))
    assert list(json.load(open(os.path.join(tmp_path, "ivf", "store.json"))))[-3:] == ["index_type", "nlist", "nprobe"]
    n_made = len(made)
    back = VS.GpuVectorStore.load(str(tmp_path / "pq"))
    assert back.index_type == "PQ" and (back.m, back.nbits) == (8, 8) and np.array_equal(back._pq_codebooks, frozen)
    assert back.pq_stats() == {"m": 8, "rows": 900, "trained_rows": 128}
    assert len(made) == n_made + 1 and made[-1].calls == [("set_codebooks",)] and np.array_equal(made[-1].cb, frozen)
    assert _dump(back.query_batch(dense_queries=dq, search_type="dense", top_k=5)) == _dump(st.query_batch(dense_queries=dq, search_type="dense", top_k=5))
    # an untrained PQ store saves no codebooks and comes back untrained
    young = VS.GpuVectorStore(dense_dim=dim, enable_sparse=False, index_type="PQ", m=4)
    young.add_vectors(*rows(0, 50))
    young.save(str(tmp_path / "young"))
    again = VS.GpuVectorStore.load(str(tmp_path / "young"))
    assert again.m == 4 and again._pq_codebooks is None and again.pq_stats() is None and isinstance(again._dense, CpuFlat)


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_reference_scores_are_the_dot_with_the_decoded_row_to_rounding():
    rng = np.random.default_rng(2)
    dim, m, n = 136, 17, 300
    cb = rng.standard_normal((m, 256, dim // m)).astype(np.float32)
    X, Q = rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((9, dim)).astype(np.float32)
    codes = R.encode(X, cb)
    assert codes.dtype == np.uint8 and codes.shape == (n, m)
    table = R.lut(Q, cb)
    S = R.scores(table, codes)
    assert table.dtype == np.float32 and table.shape == (9, m, 256) and S.dtype == np.float32 and S.shape == (9, n)
    dec = R.decode(codes, cb)
    exact = Q.astype(np.float64) @ dec.astype(np.float64).T
    # dim fp32 roundings of partial sums no larger than sum |q||d|: the error is under dim * 2^-24 of that
    bound = dim * 2.0 ** -24 * (np.abs(Q).astype(np.float64) @ np.abs(dec).astype(np.float64).T)
    assert (np.abs(S - exact) <= bound).all()
    # the rule picks the nearest centroid: no other centroid is closer than rounding allows
    xs = R.split(X, m)
    for j in (0, m - 1):
        d2 = ((xs[j][:, None, :].astype(np.float64) - cb[j][None].astype(np.float64)) ** 2).sum(axis=2)
        assert (d2[np.arange(n), codes[:, j]] <= d2.min(axis=1) + 1e-4).all()
    # one chain against a by-hand fmaf-free case: dyadic values are exact in any order
    u, v = np.array([[0.5, 0.25, -2.0]], np.float32), np.array([[4.0, 8.0, 1.5], [1.0, 1.0, 1.0]], np.float32)
    assert R.chains(u, v).tolist() == [[1.0, -1.25]]
    s, i = R.search(cb, codes, Q[:2], 4, passing=[5, 6, 7])
    assert set(i.ravel().tolist()) == {5, 6, 7, -1} and np.isneginf(s[:, 3]).all()


def test_identical_centroids_resolve_to_the_lower_code_and_ties_rank_by_id():
    rng = np.random.default_rng(3)
    cb = rng.standard_normal((3, 256, 8)).astype(np.float32)
    cb[1, 200] = cb[1, 7]
    X = rng.standard_normal((40, 24)).astype(np.float32)
    X[10:14, 8:16] = cb[1, 200]
    X[20:23] = X[3]                                   # equal rows -> equal codes -> equal scores
    codes = R.encode(X, cb)
    assert (codes[10:14, 1] == 7).all() and not (codes[:, 1] == 200).any()
    assert (codes[20:23] == codes[3]).all()
    s, i = R.search(cb, codes, X[3:4] * np.float32(3.0), 40)
    at = [i[0].tolist().index(r) for r in (3, 20, 21, 22)]
    assert at == list(range(at[0], at[0] + 4)) and len(set(s[0, at].view(np.uint32).tolist())) == 1


def test_reference_training_is_deterministic_and_keeps_empty_clusters():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((300, 8)).astype(np.float32)
    X[100:] = X[:200]                                # repeated rows: some initial centroids coincide, the higher one stays empty
    a, b = R.train(X, 2, 2), R.train(X, 2, 2)
    assert a.dtype == np.float32 and a.shape == (2, 256, 4) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    init = R.train(X, 2, 0)
    assert np.array_equal(init, R.split(X, 2)[:, (np.arange(256) * 300) // 256, :])
    codes = R.encode(X, init)
    empty = [c for c in range(256) if not (codes[:, 0] == c).any()]
    assert empty and np.array_equal(R.train(X, 2, 1)[0, empty], init[0, empty])
