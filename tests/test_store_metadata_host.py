"""`store_metadata.StoreMetadata` driven directly (no store, no GPU, no library): what an insert extends, what falls back to the host
and how often that is said, which rows travel to the device, what a compaction and a `close()` leave.  The device handles are the
CPU stand-ins of tests/test_filter_eval_gloo.py and tests/grouped_cases.py; the row filter's insists that what was uploaded is
exactly the column it evaluates, so a wrong upload or a stale device column fails inside `held`."""
import logging
import re

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from grouped_cases import CpuGroupColumn
from test_filter_eval_gloo import CpuRowFilter
from verbatim_rag_amd.store_filter import parse_filter
from verbatim_rag_amd.store_metadata import StoreMetadata

SOURCES = ("web", "journal", "book")
NAN = float("nan")


def rows_of(first, n):
    """`tags` is a number in every fourth row and a list otherwise; `document_id` walks seven documents."""
    return [{"year": 1990 + (i * 13) % 40, "source": SOURCES[i % 3], "document_id": f"d{i % 7}", "score": i / 8,
             "tags": i if i % 4 == 0 else [i % 5, "x"]} for i in range(first, first + n)]


class RowFilter(CpuRowFilter):
    """`CpuRowFilter` with the `compact` and the `strings` / `kept` arguments of the real handle, and a record of what travelled."""

    keeps = ()      # what `eval_program(strings="device")` reports as kept on host tables

    def __init__(self, device=0):
        super().__init__(device)
        self.appended, self.compacted = [], []

    def append(self, col, kinds, payload):
        super().append(col, kinds, payload)
        self.appended.append((col, len(kinds)))

    def eval_program(self, program, columns, n_rows, strings="host", kept=None):
        if strings == "device":
            kept.extend(self.keeps)
        return super().eval_program(program, columns, n_rows)

    def compact(self, keep):
        self.compacted.append(keep)
        self.kinds = [k[keep[: len(k)]] for k in self.kinds]
        self.payload = [p[keep[: len(p)]] for p in self.payload]


@pytest.fixture
def md():
    RowFilter.made, RowFilter.keeps = 0, ()
    return StoreMetadata(RowFilter, CpuGroupColumn)


def expected(flt, meta):
    pred = parse_filter(flt)
    return np.asarray([bool(pred(m)) for m in meta], dtype=bool)


def test_extend_covers_the_new_rows_of_what_was_built_and_builds_nothing_else(md):
    meta = rows_of(0, 50)
    column = md.column("year", meta)
    assert md.column("year", meta) is column and len(column) == 50
    md.value_index("document_id", meta)
    more = rows_of(50, 8)                                   # every document gains a row
    meta.extend(more)
    md.extend(more, 50)
    assert set(md.columns) == {"year"} and set(md.value_indexes) == {"document_id"}      # nothing for keys nobody asked about
    assert md.columns["year"] is column and len(column) == 58
    assert column.payload.view(np.float64).tolist() == [float(m["year"]) for m in meta]
    assert all(len(segs) == 2 for segs in md.value_indexes["document_id"].values())     # one segment per insert
    index = md.value_index("document_id", meta)
    assert all(len(segs) == 1 for segs in md.value_indexes["document_id"].values())     # merged by the read
    assert {v: rows.tolist() for v, rows in index.items()} == \
        {("s", f"d{d}"): [i for i in range(58) if i % 7 == d] for d in range(7)}
    assert md.row_filter is None and RowFilter.made == 0 and md.group_codes == {}


def test_every_host_fallback_is_logged_once_per_filter_string(md, caplog):
    meta = rows_of(0, 50)
    meta[7]["score"] = NAN                                   # `exact` False
    meta[9]["tags"] = [1, NAN]                               # `list_exact` False, `exact` untouched
    over = " or ".join(f"year == {i}" for i in range(65))
    with caplog.at_level(logging.INFO, logger="verbatim_rag_amd.vector_stores"):
        for _ in range(2):
            for flt in (over, "score > 0.5 and year > 2000", "json_contains(tags, 3)"):
                assert md.held(flt, meta, "host") is None, flt
    said = [r.getMessage() for r in caplog.records]
    assert len(said) == 3 and all(s.startswith("GpuVectorStore: filter ") and "is evaluated on the host: " in s for s in said), said
    assert "65 leaves" in said[0]
    assert said[1].endswith("metadata['score'] holds a NaN or a number beyond float range")
    assert said[2].endswith("a list of metadata['tags'] holds a NaN or a number beyond float range")
    assert md.row_filter is None and RowFilter.made == 0    # none of them reached the device
    assert md.columns["tags"].exact and not md.columns["tags"].list_exact and not md.columns["score"].exact
    got = md.held("tags >= 20", meta, "host")               # the same column still serves a scalar filter
    assert np.array_equal(got, expected("tags >= 20", meta)) and got.any() and not got.all()
    assert md.row_filter.evals == 1


def test_kept_host_tables_are_logged_once_per_filter_string(md, caplog):
    meta = rows_of(0, 50)
    flt = 'source != "web" and year > 2000'
    RowFilter.keeps = ("source != 'web': the key holds a string without a UTF-8 form", "another")
    with caplog.at_level(logging.INFO, logger="verbatim_rag_amd.vector_stores"):
        for _ in range(2):
            assert np.array_equal(md.held(flt, meta, "device"), expected(flt, meta))
        assert np.array_equal(md.held(flt + " ", meta, "host"), expected(flt, meta))       # strings="host" keeps nothing to report
    said = [r.getMessage() for r in caplog.records]
    assert said == [f"GpuVectorStore: filter {flt!r} keeps host tables for: {RowFilter.keeps[0]}; another"]
    assert md.row_filter.evals == 3


def test_only_rows_not_uploaded_yet_travel(md):
    meta = rows_of(0, 50)
    both = 'year >= 2000 and source != "web"'
    assert np.array_equal(md.held(both, meta, "host"), expected(both, meta))
    rf, cols = md.row_filter, md.row_filter_cols
    assert RowFilter.made == 1 and set(cols) == {"year", "source"}
    assert rf.appended == [(cols["year"], 50), (cols["source"], 50)]
    more = rows_of(50, 8)
    meta.extend(more)
    md.extend(more, 50)
    assert rf.appended == [(cols["year"], 50), (cols["source"], 50)]            # nothing travels before a filter asks
    assert np.array_equal(md.held("year < 2010", meta, "host"), expected("year < 2010", meta))
    assert rf.appended[2:] == [(cols["year"], 8)]                                # exactly the new rows, of the named key only
    assert rf.rows(cols["year"]) == 58 and rf.rows(cols["source"]) == 50
    assert md.row_filter is rf and RowFilter.made == 1
    assert np.array_equal(md.held(both, meta, "host"), expected(both, meta))
    assert rf.appended[3:] == [(cols["source"], 8)]


def test_compact_keeps_the_columns_and_drops_what_is_rebuilt(md):
    meta = rows_of(0, 50)
    flt = "year >= 2000 and tags < 30"
    md.held(flt, meta, "host")
    md.value_index("document_id", meta)
    assert len(md.group_column("document_id", meta, 50)) == 50
    rf = md.row_filter
    keep = np.random.default_rng(4).random(50) < 0.6
    live = int(keep.sum())
    md.compact(keep)
    meta = [m for m, k in zip(meta, keep) if k]
    assert set(md.columns) == {"year", "tags", "document_id"} and all(len(c) == live for c in md.columns.values())
    assert md.row_filter is rf and len(rf.compacted) == 1 and rf.compacted[0] is keep
    assert md.group_codes == {} and md.group_cols == {} and md.value_indexes == {}
    device = md.group_column("document_id", meta, live)     # rebuilt from the surviving rows: first-seen order from 1
    seen = {}
    assert device.codes.tolist() == [seen.setdefault(m["document_id"], len(seen) + 1) for m in meta]
    assert len(md.group_codes["document_id"]) == live
    assert np.array_equal(md.held(flt, meta, "host"), expected(flt, meta))      # over the compacted device columns
    assert len(rf.appended) == 2                                                 # ... which needed no upload


def test_drop_device_keeps_the_host_side_and_uploads_again_on_demand(md):
    meta = rows_of(0, 50)
    md.held("year >= 2000", meta, "host")
    md.group_column("source", meta, 50)
    columns, codes = dict(md.columns), dict(md.group_codes)
    md.drop_device()
    assert md.row_filter is None and md.row_filter_cols == {} and md.group_cols == {}
    assert md.columns == columns and md.group_codes == codes and set(columns) == {"year", "source"} and set(codes) == {"source"}
    assert np.array_equal(md.held("year >= 2000", meta, "host"), expected("year >= 2000", meta))
    assert RowFilter.made == 2 and md.row_filter.appended == [(md.row_filter_cols["year"], 50)]     # one new handle, the whole column
    device = md.group_column("source", meta, 50)
    assert md.group_codes["source"] is codes["source"] and device.codes.tolist() == [1 + i % 3 for i in range(50)]


def test_group_column_refuses_a_key_that_holds_a_nan(md):
    meta = rows_of(0, 50)
    meta[11]["score"] = NAN
    text = "group_by_field: metadata['score'] holds a NaN or a number beyond float range; its rows cannot be grouped"
    with pytest.raises(ValueError, match=re.escape(text)):
        md.group_column("score", meta, 50)
    assert md.group_cols == {}                               # nothing reached the device
    assert len(md.group_column("year", meta, 50)) == 50     # other keys still group
