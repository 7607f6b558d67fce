"""`GpuVectorStore(index_type="IVF_FLAT")` through `query` / `query_batch`: with nprobe = nlist it returns the FLAT store's results
exactly (dense, hybrid, weighted hybrid, host and device RRF); with a small nprobe every hit carries its row's exact score in
(score desc, row asc) order; small stores stay FLAT; appended rows are found; deletes and filters are honoured; save / load keeps
the index settings and the results; a FLAT store's manifest has no new keys.

Data: 6000 x 64 rows in 32 clusters, every entry +-1/8 (a cluster's sign pattern with a tenth of the signs flipped): unit length in
fp32, bf16-exact, every dot product a multiple of 1/64 -- every score is exact in any summation order, so two routes that look at
the same rows must agree to the bit, and ties are frequent."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, VOCAB, NLIST, CLUSTERS = 6000, 64, 2000, 32, 32
ALL = ({"nprobe": NLIST}, {"params": {"nprobe": NLIST}})


def _rows(rng, n, first, centres):
    flip = rng.random((n, DIM)) < 0.1
    dense = (centres[rng.integers(0, CLUSTERS, n)] * np.where(flip, -1, 1)).astype(np.float32) / np.float32(np.sqrt(DIM))
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 12, replace=False), rng.integers(1, 64, 12) / 64)} for _ in range(n)]
    ids = [f"id{i}" for i in range(first, first + n)]
    texts = [f"row {i}" for i in range(first, first + n)]
    metas = [{"document_id": f"d{i % 500}", "half": i % 2, "n": i} for i in range(first, first + n)]
    return ids, dense, sparse, texts, metas


def _close(st):
    if st is None:
        return
    if st._dense is not None:
        st._dense.close()
    for shard, _base, _n in st._sparse_parts:
        shard.close()
    for parts, _rows_, _dev in list(st._subsets.values()):
        for shard, _base in parts:
            shard.close()


def _dump(per_q):
    return [[(r.id, r.score, r.text, sorted(r.metadata.items())) for r in rs] for rs in per_q]


def _check_exact_and_sorted(results, queries, dense_all):
    """Every hit's score is its row's exact score against the (unit) query; lists are in (score desc, row asc) order."""
    for rs, q in zip(results, queries):
        rows = np.array([int(r.id[2:]) for r in rs])
        scores = np.array([r.score for r in rs], np.float32)
        want = (dense_all[rows].astype(np.float64) @ np.asarray(q, np.float64)).astype(np.float32)
        assert np.array_equal(scores, want)
        assert all((scores[j] > scores[j + 1]) or (scores[j] == scores[j + 1] and rows[j] < rows[j + 1]) for j in range(len(rs) - 1))


def test_ivf_store(tmp_path, caplog):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    rng = np.random.default_rng(23)
    centres = rng.integers(0, 2, (CLUSTERS, DIM)) * 2 - 1
    ids, dense, sparse, texts, metas = _rows(rng, N, 0, centres)
    kw = dict(dense_dim=DIM, sparse_vocab=VOCAB, rrf_route="device")
    flat = GpuVectorStore(**kw)
    ivf = GpuVectorStore(index_type="IVF_FLAT", nlist=NLIST, nprobe=4, **kw)
    small = GpuVectorStore(index_type="IVF_FLAT", nlist=NLIST, **kw)
    loaded = None
    try:
        for st in (flat, ivf):
            st.add_vectors(ids, dense, sparse, texts, [""] * N, metas)
        small.add_vectors(ids[:4000], dense[:4000], sparse[:4000], texts[:4000], [""] * 4000, metas[:4000])
        picks = list(rng.choice(N, 70, replace=False))           # >= RRF_DEVICE_MIN_QUERIES: the batch fuses on the device
        dq, sq = [dense[i].tolist() for i in picks], [sparse[i] for i in picks]
        assert flat.ivf_stats() is None
        assert ivf.ivf_stats() == {"nlist": NLIST, "rows": N, "trained_rows": N, "largest_list": ivf.ivf_stats()["largest_list"]}
        assert 0 < ivf.ivf_stats()["largest_list"] < N

        # nprobe = nlist, both spellings: the FLAT store's results, whole
        cases = [dict(dense_queries=dq, search_type="dense", top_k=5), dict(dense_queries=dq, search_type="dense", top_k=64),
                 dict(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=5),
                 dict(dense_queries=dq, sparse_queries=sq, top_k=7, hybrid_weights={"dense": 0.7, "sparse": 0.3}),
                 dict(dense_queries=dq[:9], sparse_queries=sq[:9], search_type="hybrid", top_k=5)]       # under 64 queries: fused on the host
        for case in cases:
            want = _dump(flat.query_batch(**case))
            for params in ALL:
                assert _dump(ivf.query_batch(search_params=params, **case)) == want, (case["top_k"], params)
        for i in (0, 69):
            for one in (dict(dense_query=dq[i], search_type="dense", top_k=5), dict(dense_query=dq[i], sparse_query=sq[i], top_k=5),
                        dict(dense_query=dq[i], sparse_query=sq[i], top_k=5, hybrid_weights={"dense": 0.6, "sparse": 0.4})):
                for params in ALL:
                    assert _dump([ivf.query(search_params=params, **one)]) == _dump([flat.query(**one)]), (i, params)
        assert _dump(ivf.query_batch(dense_queries=dq, search_type="dense", top_k=70, search_params={"nprobe": 1})) == \
            _dump(flat.query_batch(dense_queries=dq, search_type="dense", top_k=70))                     # lists over 64 rows search FLAT

        # small nprobe: exact scores of the rows it found, sorted; the row a query was taken from is found
        for params in ({"nprobe": 2}, None):                      # None: the store's own nprobe = 4
            got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params=params)
            _check_exact_and_sorted(got, dq, dense)
            assert all(len(rs) == 10 and rs[0].score == 1.0 for rs in got)
        two = _dump(ivf.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params={"nprobe": 2}))
        # nprobe does reach the overlay: the store's lists are IvfOverlay.search's, and one probed list is not the whole shard
        overlay, unit = ivf._dense.ivf, np.asarray(dq, np.float32)
        for nprobe in (1, 2):
            sc, rows_ = overlay.search(unit, 10, nprobe)
            got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params={"nprobe": nprobe})
            assert [[(r.id, r.score) for r in rs] for rs in got] == \
                [[(f"id{r}", float(v)) for r, v in zip(rr, ss) if r >= 0] for rr, ss in zip(rows_.tolist(), sc.tolist())]
        cent, off, lrows = overlay.read()
        nearest = np.argmax(unit.astype(np.float64) @ cent.astype(np.float64).T - 0.5 * (cent.astype(np.float64) ** 2).sum(axis=1), axis=1)
        one = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=64, search_params={"nprobe": 1})
        whole = flat.query_batch(dense_queries=dq, search_type="dense", top_k=64)
        outside = [q for q in range(len(dq)) if not {int(r.id[2:]) for r in whole[q]} <= set(lrows[off[nearest[q]]:off[nearest[q] + 1]].tolist())]
        assert outside, "no query's FLAT top-64 leaves its nearest list: the data cannot tell IVF from FLAT"
        for q in outside:
            assert [r.id for r in one[q]] != [r.id for r in whole[q]], "nprobe = 1 answered like FLAT"
        with caplog.at_level("WARNING"):
            with pytest.raises(ValueError, match="nprobe"):
                ivf.query_batch(dense_queries=dq, sparse_queries=sq, search_type="hybrid", search_params={"nprobe": -1})
        assert not [r for r in caplog.records if "failed" in r.getMessage()]
        for bad in ({"nprobe": 0}, {"params": {"nprobe": 1.5}}):
            with pytest.raises(ValueError, match="nprobe"):
                ivf.query(dense_query=dq[0], search_type="dense", search_params=bad)
        flat.query(dense_query=dq[0], search_type="dense", search_params={"nprobe": 0})      # a FLAT store never looked at it

        # under IVF_MIN_ROWS rows: FLAT
        assert small.ivf_stats() is None
        assert _dump(small.query_batch(dense_queries=dq, search_type="dense", top_k=5, search_params={"nprobe": 1})) == \
            _dump(small.query_batch(dense_queries=dq, search_type="dense", top_k=5))

        # save / load keeps the settings and, training being deterministic, the results
        ivf.save(str(tmp_path / "ivf"))
        flat.save(str(tmp_path / "flat"))
        head = json.load(open(os.path.join(tmp_path, "ivf", "store.json")))
        assert (head["index_type"], head["nlist"], head["nprobe"]) == ("IVF_FLAT", NLIST, 4)
        assert not {"index_type", "nlist", "nprobe"} & set(json.load(open(os.path.join(tmp_path, "flat", "store.json"))))
        loaded = GpuVectorStore.load(str(tmp_path / "ivf"), rrf_route="device")
        assert (loaded.index_type, loaded.nlist, loaded.nprobe) == ("IVF_FLAT", NLIST, 4)
        assert loaded.ivf_stats() == ivf.ivf_stats()
        assert _dump(loaded.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params={"nprobe": 2})) == two
        assert GpuVectorStore.load(str(tmp_path / "flat")).index_type == "FLAT"

        # 1000 rows appended after the first query are searchable at once (synced, not retrained)
        ids2, dense2, sparse2, texts2, metas2 = _rows(rng, 1000, N, centres)
        for st in (flat, ivf):
            st.add_vectors(ids2, dense2, sparse2, texts2, [""] * 1000, metas2)
        dense_all = np.concatenate([dense, dense2])
        dq2 = [dense2[i].tolist() for i in (0, 499, 999)]
        stats = ivf.ivf_stats()
        assert stats["rows"] == N + 1000 and stats["trained_rows"] == N
        for params in ({"nprobe": 1}, {"nprobe": NLIST}):
            got = ivf.query_batch(dense_queries=dq2, search_type="dense", top_k=10, search_params=params)
            _check_exact_and_sorted(got, dq2, dense_all)
            for rs, i in zip(got, (0, 499, 999)):
                assert f"id{N + i}" in [r.id for r in rs if r.score == 1.0]
        assert _dump(ivf.query_batch(dense_queries=dq2, search_type="dense", top_k=10, search_params=ALL[0])) == \
            _dump(flat.query_batch(dense_queries=dq2, search_type="dense", top_k=10))

        # a delete and a document_id filter under a small nprobe
        gone = sorted({r.id for rs in ivf.query_batch(dense_queries=dq, search_type="dense", top_k=3, search_params={"nprobe": 2}) for r in rs})
        for st in (flat, ivf):
            st.delete(gone)
        got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params={"nprobe": 2})
        _check_exact_and_sorted(got, dq, dense_all)
        assert all(len(rs) == 10 for rs in got) and not {r.id for rs in got for r in rs} & set(gone)
        flt = 'metadata["document_id"] == "d41"'                  # 14 rows pass: answered exactly, whatever nprobe says
        got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter=flt, search_params={"nprobe": 2})
        assert _dump(got) == _dump(flat.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter=flt))
        assert all(len(rs) == 5 and all(r.metadata["document_id"] == "d41" for r in rs) for rs in got)
        got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter='metadata["half"] == 1', search_params={"nprobe": 2})
        _check_exact_and_sorted(got, dq, dense_all)
        assert all(len(rs) == 5 and all(r.metadata["half"] == 1 and r.id not in gone for r in rs) for rs in got)
    finally:
        for st in (flat, ivf, small, loaded):
            _close(st)
