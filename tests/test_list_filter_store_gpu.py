"""`json_contains` filters through `GpuVectorStore` on every route: the same rows in six stores (`filter_eval` host / device /
device with `filter_strings="device"`, each under `filter_route` subset and bitmap), masks compared by `==` and hit lists on ids
and score bits; then the life of a store -- an insert after the first list filter, delete + `compact()`, `auto_compact`,
save / load -- the host fallbacks, and a negative control that shows the comparison sees a kind confusion.
Data as in tests/test_filter_route_gpu.py: every score is exact, ties are frequent."""
import logging

import numpy as np
import pytest

from list_filter_cases import EXPRESSIONS, any_per_row, expected, list_rows
from test_filter_eval_store_gpu import _close

pytestmark = pytest.mark.gpu

N, MORE, DIM, VOCAB = 3000, 500, 64, 600
ROWS = list_rows(N + MORE, seed=7)
QUERIED = (EXPRESSIONS[0], EXPRESSIONS[3], EXPRESSIONS[5], EXPRESSIONS[13], EXPRESSIONS[19], EXPRESSIONS[20], EXPRESSIONS[22],
           EXPRESSIONS[25])
CONFIGS = [dict(filter_eval=e, filter_strings=s, filter_route=r) for r in ("subset", "bitmap")
           for e, s in (("host", "host"), ("device", "host"), ("device", "device"))]


def _vectors(seed, n):
    rng = np.random.default_rng(seed)
    dense = (rng.integers(0, 2, (n, DIM)) * 2 - 1).astype(np.float32) / np.float32(np.sqrt(DIM))
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 12, replace=False), rng.integers(1, 64, 12) / 64)} for _ in range(n)]
    return dense, sparse


DENSE, SPARSE = _vectors(11, N + MORE)


def _add(st, a, b, rows=ROWS):
    st.add_vectors([f"id{i}" for i in range(a, b)], DENSE[a:b], SPARSE[a:b], [f"text {i}" for i in range(a, b)],
                   [f"enh {i}" for i in range(a, b)], rows[a:b])


def _store(**kw):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, **kw)
    _add(st, 0, N)
    return st


def _hits(per_q):
    return [[(r.id, np.float64(r.score).tobytes()) for r in rs] for rs in per_q]


def _mask_of(st, flt, n):
    mask = st._mask(flt)
    return np.ones(n, bool) if mask is None else mask


def _searches(st, flt):
    picks = [0, 41, N // 2, N - 1]
    dq, sq = [DENSE[i].tolist() for i in picks], [SPARSE[i] for i in picks]
    return (_hits(st.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter=flt)),
            _hits(st.query_batch(sparse_queries=sq, search_type="sparse", top_k=7, filter=flt)),
            _hits(st.query_batch(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=5, filter=flt)),
            _hits([st.query(dense_query=dq[1], search_type="dense", top_k=4, filter=flt)]),
            _hits([st.query(filter=flt, top_k=9)]))                               # filter only


@pytest.fixture(scope="module")
def reference():
    """The masks (from the Python predicate) and the hit lists (from the host / subset store) every configuration must give."""
    host = _store(**CONFIGS[0])
    try:
        masks = {flt: expected(flt, ROWS[:N]) for flt in EXPRESSIONS}
        for flt, want in masks.items():
            assert np.array_equal(_mask_of(host, flt, N), want), flt
        yield masks, {flt: _searches(host, flt) for flt in QUERIED}
    finally:
        _close(host)


@pytest.mark.parametrize("config", CONFIGS[1:], ids=lambda c: "-".join(c.values()))
def test_every_route_gives_the_host_routes_masks_and_hits(reference, config):
    masks, hits = reference
    st = _store(**config)
    try:
        for flt in EXPRESSIONS:
            got = _mask_of(st, flt, N)
            assert got.dtype == bool and np.array_equal(got, masks[flt]), (config, flt)
        for flt in QUERIED:
            assert _searches(st, flt) == hits[flt], (config, flt)
        if config["filter_eval"] == "device":
            rf, cols = st._metadata.row_filter, st._metadata.row_filter_cols
            assert {"authors", "tags", "years", "flags"} <= set(cols)
            for key in ("authors", "tags", "years", "flags"):
                assert rf.list_rows(cols[key]) == (N, int(st._metadata.columns[key].elem_off[-1]))
            assert rf.rows(cols["years"]) == 0 and rf.rows(cols["authors"]) == N     # only `authors == ..` reads scalar rows of a list key
            if config["filter_strings"] == "device":
                assert rf.strings(cols["authors"])[0] == len(st._metadata.columns["authors"].strings)
        else:
            assert st._metadata.row_filter is None and not st._metadata.columns
    finally:
        _close(st)


@pytest.mark.parametrize("strings", ["host", "device"])
def test_insert_delete_compact_and_save_load(strings, tmp_path):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    filters = (EXPRESSIONS[0], EXPRESSIONS[14], EXPRESSIONS[20], EXPRESSIONS[23])
    dev = _store(filter_eval="device", filter_strings=strings, filter_route="bitmap")
    loaded = None
    try:
        for flt in filters:
            assert np.array_equal(_mask_of(dev, flt, N), expected(flt, ROWS[:N])), flt
        rf, cols = dev._metadata.row_filter, dev._metadata.row_filter_cols
        assert rf.list_rows(cols["authors"]) == (N, int(dev._metadata.columns["authors"].elem_off[-1]))
        appended = []
        plain = rf.append_lists
        rf.append_lists = lambda col, off, kinds, payload: (appended.append((col, len(off) - 1)), plain(col, off, kinds, payload))[1]
        _add(dev, N, N + MORE)                                                      # the host column grows with the insert ...
        assert len(dev._metadata.columns["authors"]) == N + MORE and rf.list_rows(cols["authors"])[0] == N
        for flt in filters:                                                         # ... the device's list part with the next list filter
            assert np.array_equal(_mask_of(dev, flt, N + MORE), expected(flt, ROWS)), flt
        for key in ("authors", "tags", "years"):
            assert rf.list_rows(cols[key]) == (N + MORE, int(dev._metadata.columns[key].elem_off[-1]))
        assert sorted(appended) == sorted((cols[key], MORE) for key in ("authors", "tags", "years"))   # extended, not rebuilt
        del rf.append_lists

        gone = [i for i in range(N + MORE) if i % 5 == 1 or 100 <= i < 300]
        dev.delete([f"id{i}" for i in gone])
        alive = np.ones(N + MORE, bool)
        alive[gone] = False
        for flt in filters:
            assert np.array_equal(_mask_of(dev, flt, N + MORE), expected(flt, ROWS) & alive), flt
        assert dev.compact() == len(gone)
        kept = [md for md, a in zip(ROWS, alive) if a]
        assert rf.list_rows(cols["authors"]) == (0, 0) and rf.rows(cols["source"]) == len(kept)      # dropped; the scalar rows compacted
        for flt in filters:
            assert np.array_equal(_mask_of(dev, flt, len(kept)), expected(flt, kept)), flt
        assert rf.list_rows(cols["authors"]) == (len(kept), int(dev._metadata.columns["authors"].elem_off[-1]))
        top = dev.query(dense_query=DENSE[7].tolist(), search_type="dense", top_k=5, filter=filters[0])
        want = expected(filters[0], ROWS) & alive
        assert len(top) == 5 and all(want[int(r.id[2:])] for r in top)

        dev.save(str(tmp_path / "s"))
        loaded = GpuVectorStore.load(str(tmp_path / "s"), filter_eval="device", filter_strings=strings)
        for flt in filters:
            assert np.array_equal(_mask_of(loaded, flt, len(kept)), expected(flt, kept)), flt
        assert _hits([loaded.query(dense_query=DENSE[7].tolist(), search_type="dense", top_k=5, filter=filters[0])]) == _hits([top])
    finally:
        for st in (dev, loaded):
            if st is not None:
                _close(st)


def test_auto_compact_keeps_list_filters_right():
    flt = EXPRESSIONS[13]
    stores = [_store(filter_eval=where, auto_compact=0.3) for where in ("host", "device")]
    try:
        for st in stores:
            assert np.array_equal(_mask_of(st, flt, N), expected(flt, ROWS[:N]))
            st.delete([f"id{i}" for i in range(0, N, 4)])                           # a quarter dead: nothing moves yet
            assert len(st._meta) == N
            st.delete([f"id{i}" for i in range(1, N, 4)])                           # half dead: over 0.3, the store compacts itself
            assert len(st._meta) == N // 2
            kept = [ROWS[i] for i in range(N) if i % 4 >= 2]
            assert np.array_equal(_mask_of(st, flt, len(kept)), expected(flt, kept))
            hits = st.query(filter=flt, top_k=len(kept))
            assert sorted(int(r.id[2:]) for r in hits) == [i for i in range(N) if i % 4 >= 2 and expected(flt, [ROWS[i]])[0]]
    finally:
        for st in stores:
            _close(st)


def test_host_fallbacks_are_logged_once_and_stay_correct(caplog):
    rows = [dict(md) for md in ROWS[:400]]
    rows[17]["tags"] = [5, float("nan"), "x"]
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    dev = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_eval="device")
    _add(dev, 0, 400, rows)
    too_long = "json_contains_any(years, [" + ", ".join(str(1960 + i) for i in range(65)) + "])"
    try:
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="verbatim_rag_amd.vector_stores"):
            for _ in range(2):
                for flt in ("json_contains(tags, 5) and year >= 2020", too_long, "tags == 5 or year >= 2024", "json_contains(years, 2020)"):
                    want = expected(flt, rows)
                    assert np.array_equal(_mask_of(dev, flt, 400), want) and want.any() and not want.all(), flt
                dev._drop_subsets()                                                 # the second round evaluates every mask again
        said = [r.getMessage() for r in caplog.records if "evaluated on the host" in r.getMessage()]
        assert len(said) == 2 and any("a list of metadata['tags'] holds a NaN" in m for m in said) and any("65 leaves" in m for m in said), said
        column = dev._metadata.columns["tags"]
        assert column.exact and not column.list_exact                               # the scalar filter on `tags` stayed on the device
        assert dev._metadata.row_filter.rows(dev._metadata.row_filter_cols["tags"]) == 400 and dev._metadata.row_filter.list_rows(dev._metadata.row_filter_cols["tags"]) == (0, 0)
        assert dev._metadata.row_filter.list_rows(dev._metadata.row_filter_cols["years"])[0] == 400
    finally:
        _close(dev)


def test_the_comparison_sees_a_kind_confusion():
    """Negative control: the test's own copy of the `flags` column with `true` encoded as the number 1 -- the device then answers
    `json_contains(flags, true)` and `json_contains(flags, 1)` differently from the host, and the `==` on the masks fails."""
    from verbatim_rag_amd.shards import RowFilter
    from verbatim_rag_amd.store_columns import KIND_BOOL, KIND_NUMBER, MetaColumn
    from verbatim_rag_amd.store_filter import compile_filter

    col = MetaColumn("flags")
    col.extend(ROWS[:N])
    kinds, payload = col.elem_kinds.copy(), col.elem_payload.copy()
    was_true = (kinds == KIND_BOOL) & (payload == 1)
    assert was_true.any()
    kinds[was_true], payload[was_true] = KIND_NUMBER, np.float64(1.0).view(np.uint64)
    rf = RowFilter()
    try:
        right, wrong = rf.add_column(), rf.add_column()
        rf.append_lists(right, col.elem_off, col.elem_kinds, col.elem_payload)
        rf.append_lists(wrong, col.elem_off, kinds, payload)
        for flt in ("json_contains(flags, true)", "json_contains(flags, 1)"):
            want = expected(flt, ROWS[:N])
            prog = compile_filter(flt)
            assert np.array_equal(rf.eval_program(prog, [(right, col)], N), want)
            confused = rf.eval_program(prog, [(wrong, col)], N)
            assert not np.array_equal(confused, want), flt
        # `true` finds nothing any more; `1` also finds the rows whose only match is a `true`
        assert not rf.eval_program(compile_filter("json_contains(flags, true)"), [(wrong, col)], N).any()
        assert np.array_equal(rf.eval_program(compile_filter("json_contains(flags, 1)"), [(wrong, col)], N),
                              expected("json_contains(flags, 1)", ROWS[:N]) | any_per_row(col.elem_off, was_true))
    finally:
        rf.close()
