"""`LIKE`, `not (... LIKE ...)` and `not in` filters through `GpuVectorStore`: every combination of `filter_eval` x `filter_strings`
x `filter_route` returns exactly the rows a brute-force Python pass over the metadata allows (the pass uses the reference matcher
of tests/like_cases.py, not the store's parser), and the same hits as every other combination -- fresh, after an insert that brings
new distinct titles (only the new dictionary codes are uploaded), and after a delete."""
import itertools
import logging

import numpy as np
import pytest

from like_cases import STR, like_ref

pytestmark = pytest.mark.gpu

N, DIM, VOCAB = 3000, 64, 300
COMBOS = list(itertools.product(("host", "device"), ("host", "device"), ("subset", "bitmap")))      # eval, strings, route
TITLES = STR + ["BERT for retrieval", "A survey of BERT", "SciBERT 2025", "path/to/file.txt", "path/to/other.md", "100% sure", "snake_case"]


def title_of(md):
    return md["title"] if isinstance(md.get("title"), str) else None


def liked(pattern):
    return lambda md: title_of(md) is not None and like_ref(title_of(md), pattern)


# (filter, what a row's metadata must satisfy)
FILTERS = [
    ('metadata["title"] LIKE "%BERT%"', liked("%BERT%")),
    ('title LIKE "BERT%"', liked("BERT%")),
    ('title LIKE "%2025%"', liked("%2025%")),
    ('title LIKE "path/%.txt" or title LIKE "%\\%%"', lambda md: liked("path/%.txt")(md) or liked("%\\%%")(md)),
    ('title LIKE "_" || title LIKE "__"', lambda md: title_of(md) is not None and len(title_of(md)) in (1, 2)),
    ('not (title LIKE "%a%")', lambda md: not liked("%a%")(md)),
    ('not (metadata["title"] LIKE "%a%") and year >= 2010', lambda md: not liked("%a%")(md) and md["year"] >= 2010),
    ('title LIKE "%日%" and lang not in ["de", 5]', lambda md: liked("%日%")(md) and md.get("lang") != "de"),
    ('lang not in ["en"]', lambda md: md.get("lang") != "en"),
    ('title not in ["a", "b", "BERT"] and title LIKE "%"', lambda md: title_of(md) is not None and title_of(md) not in ("a", "b", "BERT")),
    ('title LIKE "snake\\_case" or title > "x"', lambda md: title_of(md) is not None and (title_of(md) == "snake_case" or title_of(md) > "x")),
    (f'title LIKE "%{"x" * 299}" or title LIKE "Z_rich"', lambda md: liked("%" + "x" * 299)(md) or liked("Z_rich")(md)),   # 300 bytes: a host table
]


def _rows(rng, n, first, titles):
    dense = (rng.integers(0, 2, (n, DIM)) * 2 - 1).astype(np.float32) / np.float32(np.sqrt(DIM))
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 8, replace=False), rng.integers(1, 64, 8) / 64)} for _ in range(n)]
    ids = [f"id{i}" for i in range(first, first + n)]
    metas = []
    for i in range(first, first + n):
        md = {"year": 1995 + (i * 7) % 35, "title": titles[(i * 5 + i // 7) % len(titles)]}
        if i % 3:
            md["lang"] = ("en", "de", "fr")[i % 5 % 3]
        if i % 9 == 0:
            del md["title"]                                             # some rows have no title
        if i % 31 == 0:
            md["title"] = (7, None, True, ["BERT"])[i % 4]              # or one that is no string
        metas.append(md)
    return ids, dense, sparse, [f"text {i}" for i in range(first, first + n)], metas


def _close(st):
    if st._dense is not None:
        st._dense.close()
    for shard, _base, _n in st._sparse_parts:
        shard.close()
    for parts, _rows_, _dev in list(st._subsets.values()):
        for shard, _base in parts:
            shard.close()
    st.close()


def _check(stores, ids, dense, metas, alive, dq, tag, filters=FILTERS):
    ids = np.asarray(ids)
    split = 0
    for flt, allows in filters:
        want = np.asarray([bool(allows(md)) for md in metas], dtype=bool) & alive
        split += int(want.any() and not want[alive].all())
        want_ids = ids[want].tolist()
        scores = dense @ np.asarray(dq, np.float32).T                   # exact: every product is +-1/64
        first = None
        for combo, st in stores.items():
            assert [r.id for r in st.query(filter=flt, top_k=len(ids))] == want_ids, (tag, flt, combo)      # every allowed row, no other
            batch = st.query_batch(dense_queries=dq, search_type="dense", top_k=8, filter=flt)
            one = st.query(dense_query=dq[-1], search_type="dense", top_k=8, filter=flt)
            for q, hits in enumerate(batch):
                got = [r.id for r in hits]
                assert len(got) == min(8, len(want_ids)) and set(got) <= set(want_ids), (tag, flt, combo, q)
                best = np.sort(scores[want, q])[::-1][: len(got)]
                assert np.allclose([r.score for r in hits], best, atol=1e-6), (tag, flt, combo, q)
            assert [r.id for r in one] == [r.id for r in batch[-1]], (tag, flt, combo)
            dump = [[(r.id, r.score) for r in hits] for hits in batch]
            first = first or dump
            assert dump == first, (tag, flt, combo)                     # identical hits across all eight combinations
    return split


def test_like_and_not_in_filters_under_every_combination_of_options(caplog):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    rng = np.random.default_rng(11)
    ids, dense, sparse, texts, metas = _rows(rng, N, 0, TITLES)
    stores = {}
    try:
        for ev, strings, route in COMBOS:
            st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_eval=ev, filter_strings=strings, filter_route=route)
            st.add_vectors(ids, dense, sparse, texts, texts, metas)
            stores[(ev, strings, route)] = st
        assert stores[("device", "device", "bitmap")].filter_strings == "device" and GpuVectorStore(dense_dim=DIM).filter_strings == "host"
        dq = [dense[i].tolist() for i in (0, 1500, 2999)]
        alive = np.ones(N, dtype=bool)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="verbatim_rag_amd.vector_stores"):
            assert _check(stores, ids, dense, metas, alive, dq, "fresh") >= len(FILTERS) - 1
        said = [r.getMessage() for r in caplog.records if "keeps host tables" in r.getMessage()]
        assert len(said) == 2 and all("300 bytes" in m for m in said), said          # the 300-byte pattern, once per device-strings store

        dev = stores[("device", "device", "subset")]
        title_col = dev._metadata.row_filter_cols["title"]
        n_titles = len({title_of(md) for md in metas} - {None})
        before = dev._metadata.row_filter.strings(title_col)
        assert before[0] == n_titles == len(dev._metadata.columns["title"].strings)
        assert before[1] == sum(len(s.encode()) for s in dev._metadata.columns["title"].strings)
        plain = stores[("device", "host", "subset")]
        assert plain._metadata.row_filter.strings(plain._metadata.row_filter_cols["title"]) == (0, 0)   # filter_strings="host" uploads no dictionary
        assert stores[("host", "device", "subset")]._metadata.row_filter is None              # and without filter_eval="device" it has no effect

        new_titles = ["BERT: a new title", "日本語 2025", "path/to/new.txt", "zz_new"]
        ids2, dense2, sparse2, texts2, metas2 = _rows(rng, 200, N, TITLES + new_titles)
        for st in stores.values():
            st.add_vectors(ids2, dense2, sparse2, texts2, texts2, metas2)
        ids, dense, metas = ids + ids2, np.concatenate([dense, dense2]), metas + metas2
        alive = np.ones(N + 200, dtype=bool)
        assert dev._metadata.row_filter.strings(title_col) == before                          # nothing travels before a filter asks
        arrived = len({title_of(md) for md in metas} - {None}) - n_titles
        assert 0 < arrived <= len(new_titles)
        _check(stores, ids, dense, metas, alive, dq, "after the insert", FILTERS[:3] + FILTERS[5:8])
        after = dev._metadata.row_filter.strings(title_col)
        fresh = dev._metadata.columns["title"].strings[n_titles:]
        assert after == (n_titles + arrived, before[1] + sum(len(s.encode()) for s in fresh))   # only the new codes were uploaded
        assert set(fresh) <= set(new_titles)

        gone = [r.id for r in dev.query(dense_query=dq[0], search_type="dense", top_k=5, filter='title LIKE "%BERT%"')] + ["id7", "id3100"]
        for st in stores.values():
            st.delete(gone)
        alive[[ids.index(g) for g in gone]] = False
        _check(stores, ids, dense, metas, alive, dq, "after the delete", FILTERS[:2] + FILTERS[5:6] + FILTERS[8:10])
        assert dev._metadata.row_filter.strings(title_col) == after
    finally:
        for st in stores.values():
            _close(st)


def test_a_title_without_a_utf8_form_keeps_its_column_on_host_tables(caplog):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    rng = np.random.default_rng(5)
    ids, dense, sparse, texts, metas = _rows(rng, 500, 0, TITLES)
    metas[17]["title"] = "BERT \ud800 lone surrogate"
    stores = {}
    try:
        for strings in ("host", "device"):
            st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_eval="device", filter_strings=strings)
            st.add_vectors(ids, dense, sparse, texts, texts, metas)
            stores[("device", strings, "subset")] = st
        dev = stores[("device", "device", "subset")]
        flt = 'title LIKE "BERT%" and lang not in ["de"] and year > 2000'
        allows = lambda md: liked("BERT%")(md) and md.get("lang") != "de" and md["year"] > 2000   # noqa: E731
        assert allows(metas[17]) or metas[17].get("lang") == "de" or metas[17]["year"] <= 2000
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="verbatim_rag_amd.vector_stores"):
            for _ in range(2):
                _check(stores, ids, dense, metas, np.ones(500, dtype=bool), [dense[3].tolist()], "surrogate", [(flt, allows)])
                dev._drop_subsets()                                     # the second round evaluates the mask again
        said = [r.getMessage() for r in caplog.records if "keeps host tables" in r.getMessage()]
        assert len(said) == 1 and "UTF-8" in said[0] and "title" in said[0], said    # once per filter string, with the reason
        assert not dev._metadata.columns["title"].encodable and dev._metadata.columns["lang"].encodable
        cols = dev._metadata.row_filter_cols
        assert dev._metadata.row_filter.strings(cols["title"]) == (0, 0) and dev._metadata.row_filter.strings(cols["lang"])[0] == 3   # the rest ran on the device
    finally:
        for st in stores.values():
            _close(st)


def test_filter_strings_must_be_host_or_device(tmp_path):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    with pytest.raises(ValueError, match="filter_strings must be 'host' or 'device'"):
        GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_strings="gpu")
    st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, filter_eval="device", filter_strings="device")
    st.save(str(tmp_path / "s"))
    loaded = GpuVectorStore.load(str(tmp_path / "s"), filter_eval="device", filter_strings="device")
    assert (loaded.filter_eval, loaded.filter_strings) == ("device", "device")
    assert GpuVectorStore.load(str(tmp_path / "s")).filter_strings == "host"
    with pytest.raises(ValueError, match="filter_strings"):
        GpuVectorStore.load(str(tmp_path / "s"), filter_strings="gpu")
    _close(loaded)
    _close(st)
