"""IVF_FLAT on the host: the pure helpers of vector_stores.py, the constructor's refusals (checked before any device is touched),
the float64 properties the GPU tests' data must have (tests/ivf_cases.py), and the scan kernel's register budget."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ivf_cases as V
import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import vector_stores as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_rows,nlist,want", [
    (0, 8192, 0), (4095, 8192, 0), (4095, 1, 0),                 # under IVF_MIN_ROWS: FLAT
    (4096, 8192, 105), (4096, 32, 32), (4096, 105, 105), (4096, 106, 105),
    (6000, 32, 32), (100_000, 8192, 2564), (1_250_000, 4096, 4096), (1_250_000, 16384, 16384),
    (10_000_000, 16384, 16384), (10_000_000, 100_000, 16384), (4096, 1, 1),
])
def test_ivf_effective_nlist(n_rows, nlist, want):
    assert VS.IVF_MIN_ROWS == 4096
    assert VS.ivf_effective_nlist(n_rows, nlist) == want == (0 if n_rows < 4096 else min(nlist, 16384, n_rows // 39))


@pytest.mark.parametrize("params,want", [
    (None, 16), ({}, 16), ({"nprobe": 3}, 3), ({"params": {"nprobe": 128}}, 128), ({"nprobe": np.int64(7)}, 7),
    ({"metric_type": "COSINE", "ef": 64}, 16), ({"params": {"ef": 10}}, 16), ({"params": None}, 16),
    ({"nprobe": 5, "params": {"nprobe": 9}}, 5), ({"nprobe": 1 << 20}, 1 << 20),
])
def test_parse_nprobe(params, want):
    assert VS.parse_nprobe(params, 16) == want


@pytest.mark.parametrize("bad", [0, -1, 2.0, "8", True, None])
def test_parse_nprobe_refuses(bad):
    if bad is None:
        assert VS.parse_nprobe({"nprobe": None}, 4) == 4        # an explicit None is "not given"
        return
    for params in ({"nprobe": bad}, {"params": {"nprobe": bad}}):
        with pytest.raises(ValueError, match="nprobe"):
            VS.parse_nprobe(params, 16)


def test_constructor_refusals_need_no_device():
    """The index arguments are checked before the library is asked for a device, so these hold on a CPU box too."""
    with pytest.raises(ValueError, match="index_type"):
        VS.GpuVectorStore(index_type="HNSW")
    with pytest.raises(ValueError, match="index_type"):
        VS.GpuVectorStore(index_type="ivf_flat")
    for kw in ({"nlist": 0}, {"nlist": 2.5}, {"nprobe": 0}, {"nprobe": "4"}, {"nlist": True}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            VS.GpuVectorStore(index_type="IVF_FLAT", **kw)
    with pytest.raises(ValueError, match="sharded stores .*keep FLAT"):
        VS.GpuVectorStore(index_type="IVF_FLAT", comm=object())
    with pytest.raises(ValueError, match="sharded stores .*keep FLAT"):
        VS.GpuVectorStore(index_type="IVF_FLAT", distributed=True)
    VS.check_index_config("FLAT", 8192, 16, True)                # a sharded FLAT store is what it always was
    VS.check_index_config("IVF_FLAT", 16384, 1, False)


class _Overlay:
    """Stand-in for `IvfOverlay` on a CPU box: records what the store asks of it and answers from the shard it lies over."""
    made = []

    def __init__(self, shard, nlist):
        self.shard, self.nlist, self.calls, self.rows = shard, nlist, [], 0
        _Overlay.made.append(self)

    def train(self, iters, max_train_rows):
        self.calls.append(("train", iters, max_train_rows))

    def sync(self):
        self.rows = len(self.shard.rows)
        self.calls.append(("sync", self.rows))

    def stats(self):
        return {"nlist": self.nlist, "rows": self.rows, "largest_list": self.rows}

    def search(self, queries, k, nprobe, stream=None):
        self.calls.append(("search", len(queries), k, nprobe))
        return self.shard.search(queries, k)

    def close(self):
        pass


def _dump(per_q):
    return [[(r.id, r.score) for r in rs] for rs in per_q]


def test_store_routes_search_params_to_the_overlay(monkeypatch, tmp_path):
    """The store's part on CPU (stand-in shards of tests/sharded_store_cases.py, a recording overlay): when it trains and syncs,
    which searches reach the overlay with which nprobe, which never do, and what `save` writes."""
    import json

    from tests.sharded_store_cases import CpuDense, CpuSparse
    from verbatim_rag_amd.distributed import merge_topk

    monkeypatch.setattr(VS._lib, "load", lambda: None)
    monkeypatch.setattr(VS._lib, "require_gpu", lambda: None)
    monkeypatch.setattr(VS, "DenseShard", CpuDense)
    monkeypatch.setattr(VS, "SparseShard", CpuSparse)
    monkeypatch.setattr(VS, "IvfOverlay", _Overlay)
    monkeypatch.setattr(VS, "_merge_parts", lambda scores, rows, k, device: merge_topk(scores, rows, k))
    monkeypatch.setattr(VS, "IVF_MIN_ROWS", 200)
    _Overlay.made.clear()
    rng = np.random.default_rng(9)
    n, dim, vocab = 640, 64, 300

    def rows(a, b):
        dense = (rng.integers(0, 2, (b - a, dim)) * 2 - 1).astype(np.float32) / np.float32(8.0)
        sparse = [{int(t): float(v) for t, v in zip(rng.choice(vocab, 9, replace=False), rng.integers(1, 64, 9) / 64)} for _ in range(a, b)]
        return ([f"id{i}" for i in range(a, b)], dense, sparse, [f"t{i}" for i in range(a, b)], [""] * (b - a),
                [{"document_id": f"d{i % 20}", "half": i % 2} for i in range(a, b)])

    first = rows(0, 150)
    st = VS.GpuVectorStore(dense_dim=dim, sparse_vocab=vocab, index_type="IVF_FLAT", nlist=8192, nprobe=6)
    flat = VS.GpuVectorStore(dense_dim=dim, sparse_vocab=vocab)
    for s_ in (st, flat):
        s_.add_vectors(*first)
    dq, sq = [first[1][i].tolist() for i in (3, 77)], [first[2][i] for i in (3, 77)]
    assert st.ivf_stats() is None and not _Overlay.made               # 150 rows: FLAT
    more = rows(150, 400)
    for s_ in (st, flat):
        s_.add_vectors(*more)
    assert st.ivf_stats() == {"nlist": 400 // 39, "rows": 400, "largest_list": 400, "trained_rows": 400}
    ov, = _Overlay.made
    assert ov.calls == [("train", 10, 64 * (400 // 39)), ("sync", 400)]
    del ov.calls[:]
    want = _dump(flat.query_batch(dense_queries=dq, search_type="dense", top_k=5))
    assert _dump(st.query_batch(dense_queries=dq, search_type="dense", top_k=5)) == want and ov.calls == [("search", 2, 5, 6)]
    del ov.calls[:]
    st.query_batch(dense_queries=dq, search_type="dense", top_k=5, search_params={"nprobe": 3, "ef": 9})
    st.query(dense_query=dq[0], search_type="dense", top_k=4, search_params={"params": {"nprobe": 5}})
    st.query_batch(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=5, search_params={"nprobe": 2})
    st.query(dense_query=dq[0], sparse_query=sq[0], top_k=3, search_params={"nprobe": 7})
    st.query(dense_query=dq[0], sparse_query=sq[0], top_k=3, hybrid_weights={"dense": 0.5, "sparse": 0.5}, search_params={"nprobe": 8})
    st.query_batch(dense_queries=dq, sparse_queries=sq, top_k=3, hybrid_weights={"dense": 0.5, "sparse": 0.5}, search_params={"nprobe": 9})
    assert ov.calls == [("search", 2, 5, 3), ("search", 1, 4, 5), ("search", 2, 10, 2), ("search", 1, 6, 7), ("search", 1, 6, 8), ("search", 2, 6, 9)]
    del ov.calls[:]
    st.query_batch(dense_queries=dq, search_type="dense", top_k=65, search_params={"nprobe": 3})         # over 64 rows: FLAT
    st.query_batch(sparse_queries=sq, search_type="sparse", top_k=5, search_params={"nprobe": 3})       # not the dense leg
    got = st.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter='metadata["document_id"] == "d3"', search_params={"nprobe": 1})
    assert ov.calls == []                                             # a filter 1/20 of the rows pass goes straight to the exact route
    assert _dump(got) == _dump(flat.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter='metadata["document_id"] == "d3"'))
    with pytest.raises(ValueError, match="nprobe"):
        st.query(dense_query=dq[0], search_type="dense", search_params={"nprobe": -2})
    for s_ in (st, flat):
        s_.add_vectors(*rows(400, 640))
    assert st.ivf_stats()["rows"] == 640 and st.ivf_stats()["trained_rows"] == 400 and ov.calls == [("sync", 640)]     # appended: synced only
    for s_ in (st, flat):
        s_.save(str(tmp_path / s_.index_type))
    head = json.load(open(tmp_path / "IVF_FLAT" / "store.json"))
    assert (head["index_type"], head["nlist"], head["nprobe"]) == ("IVF_FLAT", 8192, 6)
    assert not {"index_type", "nlist", "nprobe"} & set(json.load(open(tmp_path / "FLAT" / "store.json")))
    back = VS.GpuVectorStore.load(str(tmp_path / "IVF_FLAT"))
    assert (back.index_type, back.nlist, back.nprobe) == ("IVF_FLAT", 8192, 6) and VS.GpuVectorStore.load(str(tmp_path / "FLAT")).index_type == "FLAT"
    assert back.ivf_stats()["trained_rows"] == 640 and len(_Overlay.made) == 2
    st.add_vectors(*rows(640, 900))                                   # 900 rows >= 2 x 400: trained again, on a new overlay
    assert st.ivf_stats()["trained_rows"] == 900 and len(_Overlay.made) == 3 and _Overlay.made[-1].calls[0] == ("train", 10, 64 * (900 // 39))


@pytest.mark.parametrize("case", V.CASES, ids=lambda c: "d%d-n%d-t%d-l%d-%s" % c)
def test_gpu_test_data_has_the_properties_the_gpu_tests_rely_on(case):
    """float64 alone: an empty list, a list of one row, a size that is no multiple of 16; queries 1 and 2 probe those two lists first;
    and at most 10 % of the queries have a probe set the fp32 scores may legitimately decide otherwise (gap < 1e-5)."""
    dim, n, dtype, nlist, kind = case
    X, Q, Cn = V.data(kind, dim, n, nlist)
    rows = V.stored(X, dtype)[:n]
    sizes = np.bincount(V.assign64(rows, Cn), minlength=nlist)
    assert sizes.sum() == n
    if nlist >= 7:
        assert sizes[0] == 0 and sizes[1] == 1 and (sizes % 16 != 0).any()
        first, gap = V.probes64(Q[1:3], Cn, 1)
        assert first.ravel().tolist() == [0, 1] and (gap > 0.1).all()
    for nprobe in (1, 3):
        if nprobe < nlist and kind != "grid":
            _p, gap = V.probes64(Q, Cn, nprobe)
            assert (gap < V.GAP).mean() <= V.LEFT_OUT_MAX
    off, lrows = V.lists_of(V.assign64(rows, Cn), nlist)
    assert off[-1] == n and np.array_equal(np.sort(lrows), np.arange(n))


@pytest.mark.parametrize("dim,n,dtype,nlist,max_rows", V.TRAIN_CASES)
def test_training_data_starts_with_a_centroid_in_every_cluster(dim, n, dtype, nlist, max_rows):
    """The purity test's premise: the fixed start (evenly strided rows) puts a centroid into each of the 16 clusters, exactly one
    where there are 16 lists, and the sample holds rows of every cluster."""
    _X, label = V.clusters(dim, n)
    sample, first = V.training_rows(n, max_rows, nlist)
    assert len(np.unique(first)) == nlist and (np.diff(sample) > 0).all() and sample[-1] < n
    assert np.array_equal(np.unique(label[first]), np.arange(16)) and np.array_equal(np.unique(label[sample]), np.arange(16))
    if nlist == 16:
        assert np.array_equal(label[first], np.arange(16))


@pytest.mark.skipif(not (shutil.which("hipcc") and shutil.which("c++filt")), reason="hipcc / c++filt not on PATH")
def test_scan_kernel_spills_nothing():
    """tools/kernel_resources.py over csrc/ivf.hip: both instantiations of the scan kernel (fp32 and bf16 rows), no VGPR spill, no scratch."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "verbatim-rag_amd", "csrc", "ivf.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    scan = [line.split() for line in out.stdout.splitlines() if "ivf_scan_kernel" in line]
    assert len(scan) == 2, out.stdout
    for vgpr, _agpr, _sgpr, spill, scratch, occ, *_name in scan:
        assert int(spill) == 0 and int(scratch) == 0 and int(vgpr) <= 128 and int(occ) >= 2, (vgpr, spill, scratch, occ)
