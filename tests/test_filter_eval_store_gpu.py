"""`GpuVectorStore(filter_eval="device")` == `filter_eval="host"`: the same rows in two stores, the row mask of every filter
compared bit for bit and every result compared whole (ids, scores, texts, metadata) for `query`, `query_batch` and the
filter-only `query`, for every search type, under both `filter_route`s -- fresh, after an insert, after a delete, after a
save / load round trip, and for the filters the device route hands back to the host (a NaN in a filtered key, a program beyond
the limits).  Data as in tests/test_filter_route_gpu.py: every score is exact, ties are frequent."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, VOCAB = 5000, 64, 600
SOURCES = ["web", "journal", "arXiv", "Zürich", "", "5", "book"]
FILTERS = [
    "year >= 2020",
    'year >= 2010 and source != "web"',
    "(year < 2000 or year > 2025) and not peer == true",
    'metadata["year"] < 1995.5',
    "year <= 2020 && year > 2019",
    "year != 2020",
    'source != "journal"',
    'source < "b"',
    'source >= "web" or source == ""',
    'metadata["source"] > "Zürich" || peer != false',
    "not peer == true",
    "peer != true and score >= 0.5",
    "score < 0.25 or score > 0.75",
    "score >= -0.0 and score <= 0",
    'year in [1990, 2000.0, "2010"] or source in ["web", 5]',
    'not (year >= 2000 and (source == "web" or source == "arXiv") and peer == true)',
    'tag != 5 and tag != "5"',
    "missing_everywhere != 1",
    "missing_everywhere > 1",
    'document_id == "d41" and half == 1',
    'metadata["document_id"] == "d41"',               # one `==`: the value-index path, no column
]
# the rounds after the first one: ranges, `!=`, compounds, strings, a mixed `in`, the lookup path
LATER = FILTERS[:3] + [FILTERS[7], FILTERS[9], FILTERS[14], FILTERS[16], FILTERS[-1]]


def _rows(rng, n, first):
    dense = (rng.integers(0, 2, (n, DIM)) * 2 - 1).astype(np.float32) / np.float32(np.sqrt(DIM))
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 12, replace=False), rng.integers(1, 64, 12) / 64)} for _ in range(n)]
    ids = [f"id{i}" for i in range(first, first + n)]
    texts = [f"row {i} topic{i % 37} shared words" for i in range(first, first + n)]
    metas = []
    for i in range(first, first + n):
        md = {"document_id": f"d{i % 500}", "half": i % 2, "source": SOURCES[(i * 5) % len(SOURCES)], "score": ((i * 37) % 101) / 100}
        if i % 11:
            md["year"] = 1985 + (i * 7) % 45 if i % 3 else float(1985 + (i * 7) % 45)
        if i % 13 == 0:
            md["year"] = "2010"
        if i % 4:
            md["peer"] = bool(i % 8 < 4)
        if i % 17 == 0:
            md["score"] = None if i % 2 else -0.0
        md["tag"] = (5, "5", [5], True)[i % 4]
        metas.append(md)
    return ids, dense, sparse, texts, metas


def _close(st):
    if st._dense is not None:
        st._dense.close()
    for shard, _base, _n in st._sparse_parts:
        shard.close()
    for parts, _rows_, _dev in list(st._subsets.values()):
        for shard, _base in parts:
            shard.close()
    st.close()


def _dump(per_q):
    return [[(r.id, r.score, r.text, r.enhanced_text, sorted(r.metadata.items(), key=repr)) for r in rs] for rs in per_q]


def _compare(host, dev, dq, sq, tq, tag, filters=FILTERS):
    nq = len(dq)
    cases = [dict(dense_queries=dq, search_type="dense", top_k=5), dict(sparse_queries=sq, search_type="sparse", top_k=7),
             dict(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=5),
             dict(text_queries=tq, search_type="full_text", top_k=6),
             dict(dense_queries=dq, sparse_queries=sq, text_queries=tq, top_k=4,
                  hybrid_weights={"dense": 0.5, "sparse": 0.3, "full_text": 0.2})]
    for flt in filters:
        want_mask, got_mask = host._mask(flt), dev._mask(flt)
        assert (want_mask is None) == (got_mask is None), (tag, flt)
        if want_mask is not None:
            assert got_mask.dtype == want_mask.dtype == bool and np.array_equal(got_mask, want_mask), (tag, flt)
        for kw in cases:
            want, got = host.query_batch(filter=flt, **kw), dev.query_batch(filter=flt, **kw)
            assert _dump(got) == _dump(want), (tag, flt, kw.get("search_type"), kw["top_k"])
            rest = {k: v for k, v in kw.items() if not k.endswith("_queries")}
            one = dict(dense_query=kw.get("dense_queries", [None] * nq)[nq - 1], sparse_query=kw.get("sparse_queries", [None] * nq)[nq - 1],
                       text_query=kw.get("text_queries", [None] * nq)[nq - 1], filter=flt, **rest)
            assert _dump([dev.query(**one)]) == _dump([host.query(**one)]), (tag, flt, kw.get("search_type"))
        assert _dump([dev.query(filter=flt, top_k=9)]) == _dump([host.query(filter=flt, top_k=9)]), (tag, flt)   # filter only


@pytest.mark.parametrize("route", ["subset", "bitmap"])
def test_device_filter_evaluation_equals_the_host_route(route, tmp_path, caplog):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    rng = np.random.default_rng(7)
    ids, dense, sparse, texts, metas = _rows(rng, N, 0)
    stores = []
    for where in ("host", "device"):
        st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, enable_full_text=True, filter_route=route, filter_eval=where)
        st.add_vectors(ids, dense, sparse, texts, [f"enh {i}" for i in range(N)], metas)
        stores.append(st)
    host, dev = stores
    assert (host.filter_eval, dev.filter_eval) == ("host", "device")
    picks = [0, 41, 2500, 4999]
    dq = [dense[i].tolist() for i in picks]
    sq = [sparse[i] for i in picks]
    tq = [f"topic{i % 37} shared" for i in picks]
    loaded = None
    try:
        _compare(host, dev, dq, sq, tq, "fresh")
        # the device route did run: one column per key the compound filters name, every row uploaded; none for the lookup path
        assert not host._metadata.columns and host._metadata.row_filter is None
        assert {"year", "source", "peer", "score", "tag", "missing_everywhere", "half", "document_id"} == set(dev._metadata.columns)
        assert all(dev._metadata.row_filter.rows(c) == N for c in dev._metadata.row_filter_cols.values())
        masks = [m for m in (host._mask(f) for f in FILTERS) if m is not None]
        assert sum(bool(m.any() and not m.all()) for m in masks) >= 17       # the filters split the rows

        ids2, dense2, sparse2, texts2, metas2 = _rows(rng, 137, N)
        metas2[3]["source"] = "a source no earlier row had"
        for st in (host, dev):
            st.add_vectors(ids2, dense2, sparse2, texts2, [""] * 137, metas2)
        assert all(len(c) == N + 137 for c in dev._metadata.columns.values())    # extended by the insert, O(new rows)
        assert all(dev._metadata.row_filter.rows(c) == N for c in dev._metadata.row_filter_cols.values())   # ... uploaded by the next filter
        dq2, sq2, tq2 = dq + [dense2[3].tolist()], sq + [sparse2[3]], tq + ["row 5003"]
        _compare(host, dev, dq2, sq2, tq2, "after the insert", LATER)
        named = {"year", "source", "peer", "tag"}                              # the keys LATER's compound filters name
        assert all(dev._metadata.row_filter.rows(c) == (N + 137 if k in named else N) for k, c in dev._metadata.row_filter_cols.items())

        top = [r.id for rs in dev.query_batch(dense_queries=dq2, search_type="dense", top_k=3, filter="year >= 2020") for r in rs]
        for st in (host, dev):
            st.delete(sorted(set(top)) + ["id7", "id5003"])
        _compare(host, dev, dq2, sq2, tq2, "after the delete", LATER)

        dev.save(str(tmp_path / "s"))
        loaded = GpuVectorStore.load(str(tmp_path / "s"), filter_route=route, filter_eval="device")
        assert loaded.filter_eval == "device" and GpuVectorStore.load(str(tmp_path / "s")).filter_eval == "host"
        fresh_host = GpuVectorStore.load(str(tmp_path / "s"), filter_route=route)
        try:
            _compare(fresh_host, loaded, dq2, sq2, tq2, "after save / load", FILTERS[:4] + FILTERS[-2:])
            for flt in FILTERS:
                a, b = fresh_host._mask(flt), loaded._mask(flt)
                assert (a is None and b is None) or np.array_equal(a, b), flt
            assert loaded._metadata.columns and not fresh_host._metadata.columns
        finally:
            _close(fresh_host)

        # what the device route hands back to the host: a NaN in a filtered key, a program beyond the limits
        ids3, dense3, sparse3, texts3, metas3 = _rows(rng, 5, N + 137)
        metas3[2]["score"] = float("nan")
        for st in (host, dev):
            st.add_vectors(ids3, dense3, sparse3, texts3, [""] * 5, metas3)
        too_long = " or ".join(f"year == {1985 + i}" for i in range(65))
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="verbatim_rag_amd.vector_stores"):
            for _ in range(2):
                _compare(host, dev, dq2, sq2, tq2, "host fallbacks", ["score < 0.25 or score > 0.75", too_long, "year >= 2020"])
                dev._drop_subsets()                                          # the second round evaluates every mask again
        said = [r.getMessage() for r in caplog.records if "evaluated on the host" in r.getMessage()]
        assert len(said) == 2 and any("NaN" in m for m in said) and any("65 leaves" in m for m in said), said   # once per filter
        assert not dev._metadata.columns["score"].exact and dev._metadata.columns["year"].exact
    finally:
        for st in (host, dev, loaded):
            if st is not None:
                _close(st)
    assert dev._metadata.row_filter is None and not dev._metadata.row_filter_cols                # close() drops the RowFilter


def test_filter_eval_must_be_host_or_device(tmp_path):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    with pytest.raises(ValueError, match="filter_eval must be 'host' or 'device'"):
        GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_eval="gpu")
    st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB)
    assert st.filter_eval == "host"
    st.save(str(tmp_path / "e"))
    with pytest.raises(ValueError, match="filter_eval"):
        GpuVectorStore.load(str(tmp_path / "e"), filter_eval="gpu")
    # the grammar is the host's on both routes
    dev = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_eval="device")
    rng = np.random.default_rng(1)
    ids, dense, sparse, texts, metas = _rows(rng, 10, 0)
    dev.add_vectors(ids, dense, sparse, texts, texts, metas)
    for bad in ('metadata["x"] like "y%"', "year >", "year < true"):
        with pytest.raises(ValueError, match="GpuVectorStore: "):
            dev._mask(bad)
    assert not dev._metadata.columns
    _close(dev)
    _close(st)
