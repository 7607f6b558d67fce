"""Grouping search through `GpuVectorStore` on the device, against the brute-force model of tests/grouped_cases.py (unit rows,
chain scores from the oracle's full ranking, grouping in Python): `query` and `query_batch`, filters on both `filter_route`s and
with `filter_eval="device"`, deletes, an insert between queries, `compact()`, `save` / `load`, and the refusals.  `==` on ids,
score bits and enhanced texts."""
import numpy as np
import pytest

import grouped_cases as GC
from store_model import vs

pytestmark = pytest.mark.gpu

ROUTES = {"subset": {}, "bitmap": {"filter_route": "bitmap"}, "bitmap_device_filters": {"filter_route": "bitmap", "filter_eval": "device"}}


def _make(dtype="f32", **kw):
    kw.setdefault("dense_dtype", dtype)
    return vs.GpuVectorStore(dense_dim=GC.DIM, sparse_vocab=None, enable_sparse=False, **kw)


@pytest.mark.parametrize("routes", list(ROUTES), ids=list(ROUTES))
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_store_scenario_matches_the_model(tmp_path, dtype, routes):
    kw = ROUTES[routes]
    GC.scenario(lambda **more: _make(dtype, **kw, **more), lambda path: vs.GpuVectorStore.load(path, **kw), tmp_path,
                n_rows=3000, n_queries=9)


def test_refusals():
    GC.refusals(_make)


@pytest.mark.parametrize("flt", [None, 'metadata["m"] >= 20 and metadata["m"] < 60'])
def test_grouping_by_a_unique_key_is_the_ungrouped_query_on_an_f32_store(flt):
    """f32 rows, dim 64, k <= 16: the plain route promises the sequential chain there (csrc/topk.hip, dense_use_exact), so on
    arbitrary rows -- scores that depend on the summation order -- the two searches must agree in ids and score bits."""
    rng = np.random.default_rng(21)
    n = 3000
    X = rng.standard_normal((n, GC.DIM)).astype(np.float32)
    st = _make("f32")
    try:
        st.add_vectors([f"id{i}" for i in range(n)], X, None, [f"t{i}" for i in range(n)], [f"e{i}" for i in range(n)],
                       [{"serial": i, "m": i % 100} for i in range(n)])
        st.delete(["id7", "id8"])
        Q = rng.standard_normal((6, GC.DIM)).astype(np.float32)
        for k in (1, 10, 16):
            plain = st.query_batch(dense_queries=[q.tolist() for q in Q], top_k=k, search_type="dense", filter=flt)
            grouped = st.query_batch(dense_queries=[q.tolist() for q in Q], top_k=k, search_type="dense", filter=flt,
                                     search_params={"group_by_field": "serial"})
            assert [GC.got_of(g) for g in grouped] == [GC.got_of(p) for p in plain] and all(len(p) == k for p in plain)
            one = st.query(dense_query=Q[0].tolist(), top_k=k, search_type="dense", filter=flt, search_params={"group_by_field": "serial"})
            assert GC.got_of(one) == GC.got_of(st.query(dense_query=Q[0].tolist(), top_k=k, search_type="dense", filter=flt))
    finally:
        st.close()
