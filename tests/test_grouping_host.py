"""Grouping search, host side (no GPU): `parse_grouping`, the group-code builder (`store_groups.GroupCodes`), and the store's
routing and result assembly over exact CPU stand-ins (tests/grouped_cases.py: `DenseShard.search_grouped` answered by the oracle's
full ranking grouped in Python).  Compared with `==` on ids, score bits and enhanced texts."""
import numpy as np
import pytest

import grouped_cases as GC
import grouped_ref as GR
from store_model import vs
from verbatim_rag_amd.store_columns import MetaColumn
from verbatim_rag_amd.store_groups import NO_VALUE, GroupCodes


# ------------------------------------------------------------------------------------------------ parse_grouping
def test_parse_grouping_forms():
    G = vs.Grouping
    assert vs.parse_grouping(None) is None and vs.parse_grouping({}) is None and vs.parse_grouping({"nprobe": 4}) is None
    assert vs.parse_grouping({"group_by_field": "document_id"}) == G("document_id", 1, False)
    assert vs.parse_grouping({"group_by_field": 'metadata["document_id"]', "group_size": 3}) == G("document_id", 3, False)
    assert vs.parse_grouping({"group_by_field": "metadata['a b']", "group_size": np.int64(16)}) == G("a b", 16, False)
    assert vs.parse_grouping({"params": {"group_by_field": "k", "group_size": 2, "strict_group_size": True}}) == G("k", 2, True)
    # top level wins over "params", key by key, as for nprobe
    assert vs.parse_grouping({"group_by_field": "a", "params": {"group_by_field": "b", "group_size": 4}}) == G("a", 4, False)
    assert vs.parse_grouping({"group_by_field": " year ", "nprobe": 3, "strict_group_size": False}) == G("year", 1, False)
    # and nprobe still parses beside it
    assert vs.parse_nprobe({"group_by_field": "a", "nprobe": 7}, 16) == 7


@pytest.mark.parametrize("params, what", [
    ({"group_by_field": ""}, "group_by_field"), ({"group_by_field": None}, "group_by_field"), ({"group_by_field": 5}, "group_by_field"),
    ({"group_by_field": "metadata[document_id]"}, "group_by_field"), ({"group_by_field": 'metadata[""]'}, "group_by_field"),
    ({"group_by_field": "k", "group_size": 0}, "group_size"), ({"group_by_field": "k", "group_size": 17}, "group_size"),
    ({"group_by_field": "k", "group_size": True}, "group_size"), ({"group_by_field": "k", "group_size": 2.0}, "group_size"),
    ({"group_by_field": "k", "group_size": "2"}, "group_size"), ({"params": {"group_by_field": "k", "group_size": -1}}, "group_size"),
    ({"group_by_field": "k", "strict_group_size": 1}, "strict_group_size"), ({"group_by_field": "k", "strict_group_size": None}, "strict_group_size"),
    ({"group_size": 3}, "group_by_field"), ({"params": {"strict_group_size": True}}, "group_by_field"),
])
def test_parse_grouping_refusals(params, what):
    with pytest.raises(ValueError, match=what):
        vs.parse_grouping(params)


# ------------------------------------------------------------------------------------------------ the code builder
def _codes(values, key="k"):
    column = MetaColumn(key)
    column.extend([{} if v is ... else {key: v} for v in values])
    codes = GroupCodes(column)
    return codes, codes.sync().tolist()


def test_codes_follow_the_typing_rules_in_first_seen_order():
    values = ["5", 5, 5.0, True, 1, 1.0, False, 0, 0.0, -0.0, 2020, 2020.0, "2020", "5"]
    codes, got = _codes(values)
    #          "5" 5  5.0 True 1  1.0 False 0  0.0 -0.0 2020 2020.0 "2020" "5"
    assert got == [1, 2, 2, 3, 4, 4, 5, 6, 6, 6, 7, 7, 8, 1]
    assert codes.n_codes == 9 and codes.column.exact and NO_VALUE == 0
    assert codes.codes.dtype == np.int32


def test_rows_without_a_value_share_code_zero():
    _c, got = _codes([..., None, [1, 2], {"a": 1}, (), "x", ..., [], "x", None])
    assert got == [0, 0, 0, 0, 0, 1, 0, 0, 1, 0]
    codes, got = _codes([..., None])
    assert got == [0, 0] and codes.n_codes == 1


def test_a_nan_or_an_int_beyond_float_range_makes_the_key_inexact():
    for bad in (float("nan"), 10 ** 400):
        codes, _got = _codes(["a", bad, "b"])
        assert not codes.column.exact
    codes, _got = _codes(["a", float("inf"), -float("inf")])
    assert codes.column.exact


def test_codes_extend_with_the_columns_new_rows_only():
    column = MetaColumn("k")
    column.extend([{"k": v} for v in ("a", "b", "a", 3)])
    codes = GroupCodes(column)
    assert codes.sync().tolist() == [1, 2, 1, 3] and len(codes) == 4
    first = codes.codes.copy()
    column.extend([{"k": v} for v in ("c", 3.0, "b", None, -0.0, 0)])
    assert len(codes) == 4                                        # nothing happens until the next sync
    assert codes.sync().tolist() == [1, 2, 1, 3, 4, 3, 2, 0, 5, 5] and codes.n_codes == 6
    assert (codes.codes[:4] == first).all()
    assert codes.sync().tolist() == [1, 2, 1, 3, 4, 3, 2, 0, 5, 5]    # idempotent
    many = [{"k": f"v{i % 300}"} for i in range(5000)]
    column.extend(many)
    got = codes.sync()
    assert len(got) == 5010 and got[10:].tolist() == [6 + i % 300 for i in range(5000)]


def test_string_codes_survive_a_column_compaction_but_the_store_drops_them():
    """The column's dictionary keeps its codes through `MetaColumn.compact`; `GroupCodes` is not compacted -- a fresh one over the
    compacted column numbers the groups in the new first-seen order."""
    column = MetaColumn("k")
    column.extend([{"k": v} for v in ("a", "b", "c", "b")])
    assert GroupCodes(column).sync().tolist() == [1, 2, 3, 2]
    column.compact(np.asarray([False, True, True, True]))
    assert GroupCodes(column).sync().tolist() == [1, 2, 1]


# ------------------------------------------------------------------------------------------------ the store
def _make(**kw):
    return vs.GpuVectorStore(dense_dim=GC.DIM, sparse_vocab=None, enable_sparse=False, **kw)


@pytest.mark.parametrize("routes", [{}, {"filter_route": "bitmap"}], ids=["subset", "bitmap"])
def test_store_scenario_matches_the_model(tmp_path, routes):
    with GC.stand_ins():
        GC.scenario(lambda **kw: _make(**routes, **kw), lambda path: vs.GpuVectorStore.load(path, **routes), tmp_path,
                    n_rows=420, n_queries=5)


def test_one_search_grouped_call_per_batch_and_no_bitmap_without_filter_or_deletes(monkeypatch):
    rows = GC.rows_of(200, seed=2)
    with GC.stand_ins():
        st = _make()
        GC.fill(st, rows)
        seen = []
        real = GC.GroupedDense.search_grouped

        def spy(self, queries, n_groups, group_size, column, allow_words=None, n_allow=0, stream=None):
            seen.append((len(queries), n_groups, group_size, allow_words is None, n_allow, len(column)))
            return real(self, queries, n_groups, group_size, column, allow_words, n_allow, stream)

        monkeypatch.setattr(GC.GroupedDense, "search_grouped", spy)
        qs = [r.dense.tolist() for r in rows[:7]]
        params = {"group_by_field": "document_id", "group_size": 2}
        st.query_batch(dense_queries=qs, top_k=4, search_type="dense", search_params=params)
        assert seen == [(7, 4, 2, True, 0, 200)]
        st.query_batch(dense_queries=qs, top_k=4, search_type="dense", filter='metadata["m"] < 50', search_params=params)
        assert seen[-1] == (7, 4, 2, False, 200, 200) and len(seen) == 2
        st.delete(["id3"])
        st.query(dense_query=qs[0], top_k=4, search_type="dense", search_params=params)
        assert seen[-1] == (1, 4, 2, False, 200, 200) and len(seen) == 3
        # the queries reach the shard unit-normalised
        got = st.query(dense_query=(np.asarray(qs[1]) * 3).tolist(), top_k=4, search_type="dense", search_params=params)
        assert GC.got_of(got) == GC.got_of(st.query(dense_query=qs[1], top_k=4, search_type="dense", search_params=params))


def test_the_filter_columns_of_a_device_evaluated_store_are_reused(monkeypatch):
    rows = GC.rows_of(80, seed=2)
    with GC.stand_ins():
        st = _make()
        GC.fill(st, rows)
        column = st._metadata.columns["document_id"] = MetaColumn("document_id")     # what filter_eval="device" would have built
        column.extend(st._meta)
        st.query(dense_query=rows[0].dense.tolist(), top_k=3, search_type="dense", search_params={"group_by_field": "document_id"})
        assert st._metadata.group_codes["document_id"].column is column
        GC.fill(st, GC.rows_of(10, seed=3, first=80))
        assert len(column) == 90                                     # extended by the insert, like every typed column
        st.query(dense_query=rows[0].dense.tolist(), top_k=3, search_type="dense", search_params={"group_by_field": "document_id"})
        assert len(st._metadata.group_codes["document_id"]) == 90 and len(st._metadata.group_cols["document_id"]) == 90


def test_refusals():
    with GC.stand_ins():
        GC.refusals(_make)


class _OneRank:
    rank, world, on_gpu = 0, 1, False


def test_a_sharded_store_refuses():
    rows = GC.rows_of(30, seed=2)
    with GC.stand_ins():
        st = _make(comm=_OneRank())
        GC.fill(st, rows)
        with pytest.raises(ValueError, match="sharded"):
            st.query(dense_query=rows[0].dense.tolist(), top_k=3, search_type="dense", search_params={"group_by_field": "m"})
        assert st.query(dense_query=rows[0].dense.tolist(), top_k=3, search_type="dense")     # the plain query still answers


@pytest.mark.parametrize("flt", [None, 'metadata["m"] >= 20 and metadata["m"] < 60'])
def test_grouping_by_a_unique_key_is_the_ungrouped_query(flt):
    rows = GC.rows_of(300, seed=9)
    with GC.stand_ins():
        st = _make()
        GC.fill(st, rows)
        st.delete(["id7", "id8"])
        for k in (1, 10, 64):
            for r in rows[:4]:
                plain = st.query(dense_query=r.dense.tolist(), top_k=k, search_type="dense", filter=flt)
                grouped = st.query(dense_query=r.dense.tolist(), top_k=k, search_type="dense", filter=flt,
                                   search_params={"group_by_field": "serial"})
                assert GC.got_of(grouped) == GC.got_of(plain) and len(plain) == k


def test_the_reference_ranking_helper_groups_as_stated():
    """`group_ranked` on a hand-made ranking: groups in the order of their best row, rows in ranking order, later rows of a group
    beyond n_groups open no slot."""
    codes = np.asarray([0, 1, 0, 2, 1, 0, 3])
    ranked = np.asarray([3, 0, 1, 2, 6, 4, 5, -1])
    scores = np.asarray([9, 8, 8, 7, 6, 5, 4, 0], np.float32)
    s, r, g = GR.group_ranked(scores, ranked, codes, 3, 2)
    assert g.tolist() == [2, 0, 1] and r.tolist() == [[3, -1], [0, 2], [1, 4]]
    assert s[0].tolist() == [9.0, -np.inf] and s[2].tolist() == [8.0, 5.0]


class _RowProvider:
    """An embedding provider that answers a text with the dense row stored under that name."""

    def __init__(self, rows):
        self.rows = {r.id: r.dense.tolist() for r in rows}

    def embed_text(self, text):
        return self.rows[text]


def test_hot_path_index_hands_the_request_to_the_store_unchanged():
    from verbatim_rag_amd.index import HotPathIndex

    rows = GC.rows_of(150, seed=6)
    params = {"group_by_field": "document_id", "group_size": 2}
    with GC.stand_ins():
        st = _make()
        GC.fill(st, rows)
        idx = HotPathIndex(st, dense_provider=_RowProvider(rows))            # "auto" resolves to dense
        want = [GC.got_of(st.query(dense_query=r.dense.tolist(), top_k=4, search_type="dense", search_params=params)) for r in rows[:3]]
        assert [GC.got_of(idx.query(r.id, k=4, search_params=params)) for r in rows[:3]] == want and all(want)
        assert [GC.got_of(b) for b in idx.query_batch([r.id for r in rows[:3]], k=4, search_params=params)] == want
        assert want[0] != GC.got_of(idx.query(rows[0].id, k=4))              # and it is not the ungrouped list
        with pytest.raises(ValueError, match="filter-only"):
            idx.query(None, k=4, search_params=params)
        both = HotPathIndex(st, dense_provider=_RowProvider(rows), sparse_provider=_RowProvider(rows))   # "auto" resolves to hybrid
        with pytest.raises(ValueError, match="search_type='hybrid'"):
            both.query(rows[0].id, k=4, search_params=params)
