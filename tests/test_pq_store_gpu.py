"""`GpuVectorStore(index_type="PQ", m=8)` through `query` / `query_batch` (dim 32, 12 000 rows): under `PQ_MIN_ROWS` the answers are
a FLAT store's; from the flush that reaches it every dense list is the ranking of tests/pq_ref.py applied to the store's own unit
rows and unit queries with the codebooks read back from the shard -- for `query`, `query_batch` and the dense leg of a hybrid batch,
under a metadata filter and after a delete on both filter routes, for a row inserted after the training, after `compact()` and
after save / load (which never retrains).  A grouping request raises."""
import json
import os

import numpy as np
import pytest

import pq_ref as R

pytestmark = pytest.mark.gpu

DIM, M, VOCAB = 32, 8, 500


def _rows(rng, n, first):
    dense = rng.standard_normal((n, DIM)).astype(np.float32)
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 6, replace=False), rng.integers(1, 64, 6) / 64)} for _ in range(n)]
    ids = [f"id{i}" for i in range(first, first + n)]
    texts = [f"row {i}" for i in range(first, first + n)]
    metas = [{"document_id": f"d{i % 40}", "half": i % 2} for i in range(first, first + n)]
    return ids, dense, sparse, texts, metas


def _add(st, batch):
    ids, dense, sp, texts, metas = batch
    st.add_vectors(ids, dense, sp, texts, [""] * len(ids), metas)


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


def _pairs(per_q):
    return [[(r.id, np.float32(r.score).view(np.uint32).item()) for r in rs] for rs in per_q]


def _lists(ids, s, i):
    return [[(ids[r], v.view(np.uint32).item()) for r, v in zip(rr, ss) if r >= 0] for rr, ss in zip(i, s)]


def test_pq_store(tmp_path):
    from verbatim_rag_amd.vector_stores import PQ_MIN_ROWS, DenseShard, GpuVectorStore, PqShard, rrf_merge_rows

    rng = np.random.default_rng(41)
    first, second = _rows(rng, 5000, 0), _rows(rng, 7000, 5000)
    assert 5000 < PQ_MIN_ROWS <= 12000
    stores = {route: GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, index_type="PQ", m=M, filter_route=route) for route in ("subset", "bitmap")}
    flat = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB)
    loaded = None
    try:
        picks = [3, 500, 4999]
        dq = [(first[1][i] + 0.3 * rng.standard_normal(DIM)).tolist() for i in picks] + rng.standard_normal((7, DIM)).tolist()
        sq = [first[2][i] for i in picks] + [first[2][i] for i in range(7)]
        # under the threshold: exact rows, the FLAT store's answers
        _add(flat, first)
        want = _pairs(flat.query_batch(dense_queries=dq, search_type="dense", top_k=10))
        flt = 'metadata["document_id"] == "d7"'
        want_f = _pairs(flat.query_batch(dense_queries=dq, search_type="dense", top_k=10, filter=flt))
        for st in stores.values():
            _add(st, first)
            assert st.pq_stats() is None and isinstance(st._dense, DenseShard)
            assert _pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=10)) == want
            assert _pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=10, filter=flt)) == want_f
        # the flush that reaches it trains and swaps the PQ shard in
        for st in stores.values():
            _add(st, second)
            assert st.pq_stats() == {"m": M, "rows": 12000, "trained_rows": 12000} and isinstance(st._dense, PqShard)
        sub, bit = stores["subset"], stores["bitmap"]
        cb = sub._dense.codebooks()
        assert np.array_equal(cb.view(np.uint32), bit._dense.codebooks().view(np.uint32)), "training is deterministic"
        assert np.array_equal(cb.view(np.uint32), sub._pq_codebooks.view(np.uint32))
        n = 12000
        codes = R.encode(sub._dense_rows.data[:n], cb)
        assert np.array_equal(sub._dense.read(), codes) and np.array_equal(bit._dense.read(), codes)
        uq = sub._unit_queries(dq)
        S = R.scores(R.lut(uq, cb), codes)

        def want_lists(k, passing=None, ids=sub._ids, scores=None):
            return _lists(ids, *R.topk(S if scores is None else scores, k, passing))

        for st in (sub, bit):
            assert _pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=10)) == want_lists(10)
            assert _pairs([st.query(dense_query=dq[0], search_type="dense", top_k=7)]) == want_lists(7)[:1]
            assert _pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=100)) == want_lists(100)      # paged
        # the dense leg of a hybrid batch
        top_k = 6
        got = sub.query_batch(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=top_k)
        d_rows, d_scores = sub._topk_rows("dense", dq, 2 * top_k, None)
        s_rows, _ = sub._topk_rows("sparse", sq, 2 * top_k, None)
        want_d = R.topk(S, 2 * top_k)
        assert np.array_equal(d_rows, want_d[1]) and np.array_equal(np.asarray(d_scores, np.float32).view(np.uint32), want_d[0].view(np.uint32))
        rows, dist = rrf_merge_rows({"dense": d_rows, "sparse": s_rows}, top_k, {"dense": 0.5, "sparse": 0.5}, 60)
        assert [[(r.id, r.score) for r in rs] for rs in got] == \
            [[(f"id{r}", float(d)) for r, d in zip(rr, dd) if r >= 0] for rr, dd in zip(rows.tolist(), dist.tolist())]

        # a metadata filter, then a delete, on both routes: the reference over the passing rows
        passing = np.arange(n)[np.arange(n) % 40 == 7]
        for k in (5, 80):
            got = [_pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=k, filter=flt)) for st in (sub, bit)]
            assert got[0] == got[1] == want_lists(k, passing), k
        assert any(isinstance(parts[0][0], PqShard) for parts, _r, _d in sub._subsets.values() if parts), "the subset shard is a PQ shard"
        assert not bit._subsets
        gone = sorted({r.id for rs in sub.query_batch(dense_queries=dq, search_type="dense", top_k=3) for r in rs})
        for st in (sub, bit):
            st.delete(gone)
        alive = np.array([f"id{r}" not in set(gone) for r in range(n)])
        for flt_, keep in ((None, alive), ('metadata["half"] == 1', alive & (np.arange(n) % 2 == 1)), (flt, alive & (np.arange(n) % 40 == 7))):
            got = [_pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=10, filter=flt_)) for st in (sub, bit)]
            assert got[0] == got[1] == want_lists(10, np.nonzero(keep)[0]), flt_
            assert not {i for rs in got[0] for i, _ in rs} & set(gone)

        # an insert after the training is encoded with the frozen codebooks and found
        extra = _rows(rng, 3, n)
        shard = bit._dense
        _add(bit, extra)
        new_q = [extra[1][1].tolist()]
        got = bit.query_batch(dense_queries=new_q, search_type="dense", top_k=10)
        assert bit._dense is shard and len(shard) == n + 3 and bit.pq_stats() == {"m": M, "rows": n + 3, "trained_rows": 12000}
        assert np.array_equal(shard.codebooks().view(np.uint32), cb.view(np.uint32))
        codes3 = np.concatenate([codes, R.encode(bit._dense_rows.data[n:n + 3], cb)])
        assert np.array_equal(shard.read(), codes3)
        S3 = R.scores(R.lut(bit._unit_queries(new_q), cb), codes3)
        alive3 = np.concatenate([alive, np.ones(3, bool)])
        assert _pairs(got) == want_lists(10, np.nonzero(alive3)[0], ids=bit._ids, scores=S3)
        assert f"id{n + 1}" in [r.id for r in got[0]]

        # compact() and save / load keep ids and score bits; nothing trains again
        before = _pairs(bit.query_batch(dense_queries=dq, search_type="dense", top_k=10))
        before_f = _pairs(bit.query_batch(dense_queries=dq, search_type="dense", top_k=10, filter=flt))
        assert bit.compact() == len(gone)
        assert bit._dense is shard and len(shard) == n + 3 - len(gone) and np.array_equal(shard.read(), codes3[alive3])
        assert _pairs(bit.query_batch(dense_queries=dq, search_type="dense", top_k=10)) == before
        assert _pairs(bit.query_batch(dense_queries=dq, search_type="dense", top_k=10, filter=flt)) == before_f
        bit.save(str(tmp_path / "pq"))
        head = json.load(open(os.path.join(tmp_path, "pq", "store.json")))
        assert (head["index_type"], head["m"], head["nbits"], head["dense_dtype"]) == ("PQ", M, 8, "f32")
        loaded = GpuVectorStore.load(str(tmp_path / "pq"))
        assert loaded.index_type == "PQ" and loaded.m == M and np.array_equal(loaded._pq_codebooks.view(np.uint32), cb.view(np.uint32))
        assert _pairs(loaded.query_batch(dense_queries=dq, search_type="dense", top_k=10)) == before
        assert _pairs(loaded.query_batch(dense_queries=dq, search_type="dense", top_k=10, filter=flt)) == before_f
        assert isinstance(loaded._dense, PqShard) and loaded.pq_stats() == {"m": M, "rows": n + 3 - len(gone), "trained_rows": 12000}
        assert np.array_equal(loaded._dense.codebooks().view(np.uint32), cb.view(np.uint32))

        with pytest.raises(ValueError, match="grouping search .*index_type='PQ'"):
            sub.query(dense_query=dq[0], search_type="dense", top_k=3, search_params={"group_by_field": "document_id"})
    finally:
        for st in (*stores.values(), flat, loaded):
            _close(st)
