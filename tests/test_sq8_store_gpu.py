"""`GpuVectorStore(dense_dtype="int8")` through `query` / `query_batch`: every dense list is the ranking of tests/sq8_ref.py applied to
the store's own unit rows and unit queries -- after an append into the resident shard, after the capacity rebuild, under a
metadata filter and after a delete on both filter routes, paged (top_k 100), after save / load -- and a hybrid store fuses its own
int8 dense leg with its sparse leg."""
import json
import os

import numpy as np
import pytest

import sq8_ref as R

pytestmark = pytest.mark.gpu

DIM, VOCAB = 64, 500


def _rows(rng, n, first):
    dense = rng.standard_normal((n, DIM)).astype(np.float32)
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 8, replace=False), rng.integers(1, 64, 8) / 64)} for _ in range(n)]
    ids = [f"id{i}" for i in range(first, first + n)]
    texts = [f"row {i}" for i in range(first, first + n)]
    metas = [{"document_id": f"d{i % 40}", "half": i % 2} for i in range(first, first + n)]
    return ids, dense, sparse, texts, metas


def _add(st, batch, sparse=False):
    ids, dense, sp, texts, metas = batch
    st.add_vectors(ids, dense, sp if sparse else [None] * len(ids), texts, [""] * len(ids), metas)


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


def _want(st, dq, k, passing=None):
    """The reference's lists over the store's own unit rows (all of them, or the rows `passing`) as (id, score bits)."""
    n = len(st._ids)
    s, i = R.search(st._dense_rows.data[:n], st._unit_queries(dq), k, passing)
    return [[(f"id{r}", v.view(np.uint32).item()) for r, v in zip(rr, ss) if r >= 0] for rr, ss in zip(i, s)]


def test_int8_store(tmp_path):
    from verbatim_rag_amd.vector_stores import GpuVectorStore, Sq8Shard

    rng = np.random.default_rng(31)
    first, second, third = _rows(rng, 2000, 0), _rows(rng, 1000, 2000), _rows(rng, 2000, 3000)
    stores = {route: GpuVectorStore(dense_dim=DIM, dense_dtype="int8", enable_sparse=False, filter_route=route) for route in ("subset", "bitmap")}
    loaded = None
    try:
        dq = [(first[1][i] + 0.3 * rng.standard_normal(DIM)).tolist() for i in (3, 500, 1999)] + rng.standard_normal((7, DIM)).tolist()
        for st in stores.values():
            _add(st, first)
            assert _pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=5)) == _want(st, dq, 5)       # flushes: the shard is resident
            shard = st._dense
            assert isinstance(shard, Sq8Shard) and len(shard) == 2000
            codes, scales = shard.read()
            want_c, want_s = R.quantize(st._dense_rows.data[:2000])
            assert np.array_equal(codes, want_c) and np.array_equal(scales.view(np.uint32), want_s.view(np.uint32))
            _add(st, second)                                      # 3000 <= 2000 * dense_headroom: appended into the resident shard
            assert _pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=10)) == _want(st, dq, 10)
            assert st._dense is shard and len(shard) == 3000
            assert _pairs([st.query(dense_query=dq[0], search_type="dense", top_k=7)]) == _want(st, dq[:1], 7)
            assert _pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=100)) == _want(st, dq, 100)    # paged
        sub, bit = stores["subset"], stores["bitmap"]

        # a metadata filter, then a delete, on both routes: the reference over the passing rows
        n = 3000
        flt = 'metadata["document_id"] == "d7"'                   # 75 rows pass: the second pass answers
        passing = np.arange(n)[np.arange(n) % 40 == 7]
        for k in (5, 80):
            got = [_pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=k, filter=flt)) for st in (sub, bit)]
            assert got[0] == got[1] == _want(sub, dq, k, passing), k
        gone = sorted({r.id for rs in sub.query_batch(dense_queries=dq, search_type="dense", top_k=3) for r in rs})
        for st in (sub, bit):
            st.delete(gone)
        alive = np.array([f"id{r}" not in set(gone) for r in range(n)])
        for flt_, keep in ((None, alive), ('metadata["half"] == 1', alive & (np.arange(n) % 2 == 1)), (flt, alive & (np.arange(n) % 40 == 7))):
            got = [_pairs(st.query_batch(dense_queries=dq, search_type="dense", top_k=10, filter=flt_)) for st in (sub, bit)]
            assert got[0] == got[1] == _want(sub, dq, 10, np.nonzero(keep)[0]), flt_
            assert not {i for rs in got[0] for i, _ in rs} & set(gone)

        # save / load keeps the dtype and the lists
        before = _pairs(bit.query_batch(dense_queries=dq, search_type="dense", top_k=10))
        bit.save(str(tmp_path / "int8"))
        assert json.load(open(os.path.join(tmp_path, "int8", "store.json")))["dense_dtype"] == "int8"
        loaded = GpuVectorStore.load(str(tmp_path / "int8"))
        assert loaded.dense_dtype == "int8"
        assert _pairs(loaded.query_batch(dense_queries=dq, search_type="dense", top_k=10)) == before
        assert isinstance(loaded._dense, Sq8Shard)

        # a third insert overflows the headroom: the shard is rebuilt
        old = sub._dense
        _add(sub, third)
        n = 5000
        alive = np.array([f"id{r}" not in set(gone) for r in range(n)])
        assert _pairs(sub.query_batch(dense_queries=dq, search_type="dense", top_k=10)) == _want(sub, dq, 10, np.nonzero(alive)[0])
        assert sub._dense is not old and isinstance(sub._dense, Sq8Shard) and len(sub._dense) == 5000
    finally:
        for st in (*stores.values(), loaded):
            _close(st)


def test_int8_hybrid_store():
    from verbatim_rag_amd.vector_stores import GpuVectorStore, rrf_merge_rows

    rng = np.random.default_rng(32)
    batch = _rows(rng, 1500, 0)
    st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, dense_dtype="int8")
    try:
        _add(st, batch, sparse=True)
        picks = [5, 700, 1499, 42]
        dq, sq = [batch[1][i].tolist() for i in picks], [batch[2][i] for i in picks]
        top_k = 6
        got = st.query_batch(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=top_k)
        d_rows, d_scores = st._topk_rows("dense", dq, 2 * top_k, None)
        s_rows, _ = st._topk_rows("sparse", sq, 2 * top_k, None)
        want_d = R.search(st._dense_rows.data[:1500], st._unit_queries(dq), 2 * top_k)
        assert np.array_equal(d_rows, want_d[1]) and np.array_equal(np.asarray(d_scores, np.float32).view(np.uint32), want_d[0].view(np.uint32))
        rows, dist = rrf_merge_rows({"dense": d_rows, "sparse": s_rows}, top_k, {"dense": 0.5, "sparse": 0.5}, 60)
        assert [[(r.id, r.score) for r in rs] for rs in got] == \
            [[(f"id{r}", float(d)) for r, d in zip(rr, dd) if r >= 0] for rr, dd in zip(rows.tolist(), dist.tolist())]
        assert all(rs[0].id == f"id{p}" for rs, p in zip(got, picks))
        one = st.query(dense_query=dq[0], sparse_query=sq[0], top_k=top_k)
        assert [(r.id, r.score) for r in one] == [(r.id, r.score) for r in got[0]]
    finally:
        _close(st)
