"""`GpuVectorStore(filter_route="bitmap")` == `filter_route="subset"` through the C ABI: the same rows in two stores, every
result compared whole (ids, scores, texts, metadata) for `query` and `query_batch`, dense / sparse / hybrid / three-leg hybrid
with full text, under filters that a handful, a list, about half and all of the rows pass -- again after deletes of rows in the
unfiltered top-k, after an append (a sparse tail segment) and after a save / load round trip.  Data as in
tests/test_query_batch_gpu.py (bf16-exact unit rows, dyadic sparse weights): every score is exact, ties are frequent."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, VOCAB = 3000, 64, 2000
FILTERS = ['metadata["document_id"] == "d41"', 'metadata["n"] in [0, 1, 2, 3, 5, 8, 13, 21, 34, 2999, 3001, 3050]', 'metadata["half"] == 1', None]


def _rows(rng, n, first):
    dense = (rng.integers(0, 2, (n, DIM)) * 2 - 1).astype(np.float32) / np.float32(np.sqrt(DIM))
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 12, replace=False), rng.integers(1, 64, 12) / 64)} for _ in range(n)]
    ids = [f"id{i}" for i in range(first, first + n)]
    texts = [f"row {i} topic{i % 37} shared words" for i in range(first, first + n)]
    metas = [{"document_id": f"d{i % 500}", "half": i % 2, "n": i} for i in range(first, first + n)]
    return ids, dense, sparse, texts, metas


def _close(st):
    if st._dense is not None:
        st._dense.close()
    for shard, _base, _n in st._sparse_parts:
        shard.close()
    for parts, _rows_, _dev in list(st._subsets.values()):
        for shard, _base in parts:
            shard.close()


def _dump(per_q):
    return [[(r.id, r.score, r.text, r.enhanced_text, sorted(r.metadata.items())) for r in rs] for rs in per_q]


def _compare(sub, bm, dq, sq, tq, tag):
    nq = len(dq)
    cases = [dict(dense_queries=dq, search_type="dense", top_k=5), dict(sparse_queries=sq, search_type="sparse", top_k=7),
             dict(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=5),
             dict(dense_queries=dq, sparse_queries=sq, text_queries=tq, top_k=4,
                  hybrid_weights={"dense": 0.5, "sparse": 0.3, "full_text": 0.2}),
             dict(dense_queries=dq, search_type="dense", top_k=70)]
    for flt in FILTERS:
        for kw in cases:
            want, got = sub.query_batch(filter=flt, **kw), bm.query_batch(filter=flt, **kw)
            assert _dump(got) == _dump(want), (tag, flt, kw.get("search_type"), kw["top_k"])
            rest = {k: v for k, v in kw.items() if not k.endswith("_queries")}
            for i in (0, nq - 1):
                one = dict(dense_query=kw.get("dense_queries", [None] * nq)[i], sparse_query=kw.get("sparse_queries", [None] * nq)[i],
                           text_query=kw.get("text_queries", [None] * nq)[i], filter=flt, **rest)
                assert _dump([bm.query(**one)]) == _dump([sub.query(**one)]), (tag, flt, kw.get("search_type"), i)
        assert not bm._subsets, (tag, flt)
    assert sub._subsets                      # the default route did build its subset shards: the two routes were different code


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bitmap_route_equals_subset_route(dtype, tmp_path):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    rng = np.random.default_rng(11)
    ids, dense, sparse, texts, metas = _rows(rng, N, 0)
    stores = []
    for route in ("subset", "bitmap"):
        st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, dense_dtype=dtype, enable_full_text=True, filter_route=route)
        st.add_vectors(ids, dense, sparse, texts, [f"enh {i}" for i in range(N)], metas)
        stores.append(st)
    sub, bm = stores
    picks = [0, 1, 41, 541, 1500, 2998, 2999, 7, 100]
    dq = [dense[i].tolist() for i in picks]
    sq = [sparse[i] for i in picks]
    tq = [f"topic{i % 37} shared" for i in picks]
    loaded = None
    try:
        _compare(sub, bm, dq, sq, tq, "fresh")
        top = [r.id for rs in bm.query_batch(dense_queries=dq, search_type="dense", top_k=3) for r in rs]
        top += [r.id for rs in bm.query_batch(sparse_queries=sq, search_type="sparse", top_k=3) for r in rs]
        for st in (sub, bm):
            st.delete(sorted(set(top)))
        _compare(sub, bm, dq, sq, tq, "after deleting the top rows")
        ids2, dense2, sparse2, texts2, metas2 = _rows(rng, 100, N)
        for st in (sub, bm):
            st.add_vectors(ids2, dense2, sparse2, texts2, [""] * 100, metas2)
        dq2, sq2 = dq + [dense2[1].tolist(), dense2[50].tolist()], sq + [sparse2[1], sparse2[50]]
        _compare(sub, bm, dq2, sq2, tq + ["topic3 words", "row 3050"], "after the append")
        assert len(bm._sparse_parts) == 2 and bm._sparse_parts[1][1] % 32 != 0      # the tail segment starts inside a bitmap word
        bm.save(str(tmp_path / "s"))
        loaded = GpuVectorStore.load(str(tmp_path / "s"), filter_route="bitmap")
        assert loaded._filter_route == "bitmap"
        _compare(sub, loaded, dq2, sq2, tq + ["topic3 words", "row 3050"], "after save / load")
    finally:
        for st in (sub, bm, loaded):
            if st is not None:
                _close(st)
