"""`GpuVectorStore(rrf_route="device")` on CPU: the store's part of the device fusion -- which batches reach
`rrf_fuse_rows_device`, with which lists, and which never do -- against the stand-in shard classes of
tests/sharded_store_cases.py, with the device routine replaced by a recorder that answers from `rrf_merge_rows`
(tests/test_rrf_fuse_gpu.py compares the real routine with it bit for bit)."""
import ctypes

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from tests.sharded_store_cases import CpuDense, CpuSparse
from verbatim_rag_amd import _lib
from verbatim_rag_amd import vector_stores as vs

N, DIM, VOCAB, NQ = 203, 64, 300, 6
CALLS = []          # (methods in the order given, columns per method, top_k, weights, rrf_k, device) of every device fusion


@pytest.fixture()
def stand_ins(monkeypatch):
    from verbatim_rag_amd.distributed import merge_topk

    def recorder(rows_by_method, top_k, weights, rrf_k=60, device=0):
        CALLS.append((list(rows_by_method), [np.asarray(r).shape for r in rows_by_method.values()], top_k, dict(weights), rrf_k, device))
        return vs.rrf_merge_rows(rows_by_method, top_k, weights, rrf_k)

    monkeypatch.setattr(vs._lib, "load", lambda: None)
    monkeypatch.setattr(vs._lib, "require_gpu", lambda: None)
    monkeypatch.setattr(vs, "DenseShard", CpuDense)
    monkeypatch.setattr(vs, "SparseShard", CpuSparse)
    monkeypatch.setattr(vs, "_merge_parts", lambda scores, rows, k, device: merge_topk(scores, rows, k))
    monkeypatch.setattr(vs, "rrf_fuse_rows_device", recorder)
    monkeypatch.setattr(vs.GpuVectorStore, "RRF_DEVICE_MIN_QUERIES", 1)      # the routing is under test here, not the batch size
    CALLS.clear()
    yield
    CALLS.clear()


def _data(seed=5):
    rng = np.random.default_rng(seed)
    dense = (rng.integers(0, 2, (N, DIM)) * 2 - 1).astype(np.float32) / np.float32(8.0)      # unit rows stay dyadic: exact ties
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 9, replace=False), rng.integers(1, 64, 9) / 64)} for _ in range(N)]
    return dense, sparse


def _store(route=None, ids=None):
    dense, sparse = _data()
    st = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, **({} if route is None else {"rrf_route": route}))
    ids = ids or [f"id{i}" for i in range(N)]
    st.add_vectors(ids, dense.tolist(), sparse, [f"text {i}" for i in range(N)], [f"enh {i}" for i in range(N)],
                   [{"document_id": f"d{i % 20}", "half": i % 2, "n": i} for i in range(N)])
    picks = [3, 17, 100, 101, 202, 55][:NQ]
    return st, [dense[i].tolist() for i in picks], [sparse[i] for i in picks]


def _dump(per_q):
    return [[(r.id, r.score, r.text, sorted(r.metadata.items())) for r in rs] for rs in per_q]


def test_rrf_route_is_validated_and_not_saved(stand_ins, tmp_path):
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError, match="rrf_route"):
            vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, rrf_route=bad)
    st, _dq, _sq = _store()
    assert st.rrf_route == "host"
    st.save(str(tmp_path / "s"))
    assert "rrf_route" not in open(tmp_path / "s" / "store.json").read()           # a run-time choice, not part of a saved store
    with pytest.raises(ValueError, match="rrf_route"):
        vs.GpuVectorStore.load(str(tmp_path / "s"), rrf_route="nope")
    assert vs.GpuVectorStore.load(str(tmp_path / "s")).rrf_route == "host"
    assert vs.GpuVectorStore.load(str(tmp_path / "s"), rrf_route="device").rrf_route == "device"


def test_device_route_fuses_each_hybrid_batch_once(stand_ins):
    host, dq, sq = _store("host")
    dev, _dq, _sq = _store("device")
    for kw, weights, rrf_k in (
            (dict(search_type="hybrid", top_k=5), {"dense": 0.5, "sparse": 0.5}, 60),
            (dict(top_k=4, hybrid_weights={"sparse": 0.3, "dense": 0.7}, rrf_k=30), {"sparse": 0.3, "dense": 0.7}, 30),
            (dict(search_type="hybrid", top_k=3, filter='metadata["half"] == 1'), {"dense": 0.5, "sparse": 0.5}, 60)):
        want = host.query_batch(dense_queries=dq, sparse_queries=sq, **kw)
        assert not CALLS                                                                # "host" never calls it
        got = dev.query_batch(dense_queries=dq, sparse_queries=sq, **kw)
        k = kw["top_k"]
        assert CALLS == [(["dense", "sparse"], [(NQ, 2 * k), (NQ, 2 * k)], k, weights, rrf_k, 0)]      # fusion order, 2 * top_k columns
        CALLS.clear()
        assert _dump(got) == _dump(want)
        assert _dump([dev.query(dense_query=dq[0], sparse_query=sq[0], **kw)]) == _dump(got[:1])
        assert not CALLS                                                                # `query` fuses on the host


def test_other_branches_never_reach_the_device_fusion(stand_ins):
    dev, dq, sq = _store("device")
    dev.query_batch(dense_queries=dq, sparse_queries=sq, top_k=4, hybrid_weights={"dense": 1.0})     # one method left: its first top_k
    dev.query_batch(dense_queries=dq, top_k=4, search_type="dense")
    dev.query_batch(sparse_queries=sq, top_k=4, search_type="sparse")
    assert not CALLS
    falsy, dq, sq = _store("device", ids=[f"id{i}" if i != 17 else "" for i in range(N)])
    host, _dq, _sq = _store("host", ids=[f"id{i}" if i != 17 else "" for i in range(N)])
    assert not falsy._all_ids_truthy
    kw = dict(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=5)
    assert _dump(falsy.query_batch(**kw)) == _dump(host.query_batch(**kw))
    assert not CALLS                                                                    # a falsy id: the per-query dict path


def test_batches_below_the_measured_crossover_stay_on_the_host(stand_ins, monkeypatch):
    dev, dq, sq = _store("device")
    host, _dq, _sq = _store("host")
    monkeypatch.setattr(vs.GpuVectorStore, "RRF_DEVICE_MIN_QUERIES", NQ + 1)
    kw = dict(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=5)
    got = dev.query_batch(**kw)
    assert not CALLS
    monkeypatch.setattr(vs.GpuVectorStore, "RRF_DEVICE_MIN_QUERIES", NQ)
    assert _dump(dev.query_batch(**kw)) == _dump(got) == _dump(host.query_batch(**kw))      # same output on both sides of it
    assert len(CALLS) == 1


def test_binding_and_no_device_status():
    assert "vrag_rrf_fuse" in _lib.SIGNATURES and len(_lib.SIGNATURES["vrag_rrf_fuse"][1]) == 10
    lib = _lib.load()
    assert lib.vrag_abi_version() == 6                                                  # added without an ABI bump
    if lib.vrag_device_count() > 0:
        pytest.skip("GPU present")
    rows, gains = np.arange(8, dtype=np.int64), np.full(8, 0.01)
    out_r, out_d = np.full(4, -7, np.int64), np.full(4, -7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.vrag_rrf_fuse(p(rows), p(gains), 1, 8, 4, p(out_r), p(out_d), 0, 0, None) == -4
    assert "no HIP device" in _lib.last_error()
    assert lib.vrag_rrf_fuse(p(rows), p(gains), 1, 8, 9, p(out_r), p(out_d), 0, 0, None) == -1     # bad geometry: the argument status
    assert "top_k" in _lib.last_error()
    assert (out_r == -7).all() and (out_d == -7.0).all()                                # and nothing computed on the host
    with pytest.raises(_lib.VragError, match="no HIP device"):
        vs.rrf_fuse_rows_device({"dense": rows[None], "sparse": rows[None]}, 3, {"dense": 0.5, "sparse": 0.5})
