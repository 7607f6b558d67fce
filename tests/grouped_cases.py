"""Shared by the grouping-search tests of the store (tests/test_grouping_host.py over CPU stand-ins, tests/test_grouped_store_gpu.py
on the device): a brute-force model of a grouped query -- the live rows that pass a Python predicate, a full oracle ranking,
grouping by a Python restatement of the typing rules -- the stand-in shard and group column, and one scenario that walks a store
through queries, filters, deletes, an insert behind a built column, `compact()` and `save` / `load`.

The rows are store_model's dyadic-grid rows (entries 0, +-1/8, +-2/8: unit norm, bf16-exact, every dot product exact in any
order), so the store's normalisation is the identity, f32 and bf16 stores give the same bits and equal scores are frequent:
the tie order inside and between groups is what is tested.  `==` on ids, score bits and enhanced texts; no tolerance."""
from __future__ import annotations

import contextlib
from typing import Any, Callable, Dict, List

import numpy as np

import compact_cases as CC
import grouped_ref as GR
import store_model as M
from store_model import vs

DIM = 64
FILTERS = [
    (None, lambda md: True),
    ('metadata["m"] >= 20 and metadata["m"] < 60', lambda md: 20 <= md["m"] < 60),
    ('metadata["document_id"] == "d3"', lambda md: md.get("document_id") == "d3"),          # one group passes
    ('metadata["document_id"] in ["d1", "d2", "d5"]', lambda md: md.get("document_id") in ("d1", "d2", "d5")),   # three groups pass
    ('metadata["document_id"] == "nobody"', lambda md: False),
]
SHAPES = [(5, 1), (10, 3), (64, 16), (1, 2)]         # (top_k, group_size)


def metadata_of(serial: int) -> dict:
    """`document_id`: 23 documents interleaved over the rows, one row in 13 without the key, one in 29 with a list.  `year`: the
    typing rules in one key.  `serial`: unique."""
    md: Dict[str, Any] = {"m": serial % 100, "serial": serial}
    if serial % 13 == 5:
        pass
    elif serial % 29 == 7:
        md["document_id"] = ["d1", "d2"]
    else:
        md["document_id"] = f"d{(serial * 7) % 23}"
    md["year"] = (2020, 2020.0, "2020", True, 1, 0.0, -0.0, None)[serial % 8]
    return md


def identity(value) -> Any:
    """The group a metadata value belongs to, restated: bool before number, numbers by float value (so -0.0 is 0.0), strings as
    they are, everything else one "no value" group."""
    if isinstance(value, bool):
        return ("b", value)
    if isinstance(value, (int, float)):
        return ("n", float(value))
    if isinstance(value, str):
        return ("s", value)
    return None


def rows_of(n: int, seed: int, first: int = 0) -> List[M.Row]:
    rng = np.random.default_rng(seed)
    dense = M.unit_rows(rng, n, DIM)
    dense[1::17] = dense[0]                                  # exact duplicates, in different documents and in the same one
    return [M.Row(f"id{first + i}", first + i, dense[i], None, f"text {first + i}", [], metadata_of(first + i)) for i in range(n)]


def fill(st, rows: List[M.Row]) -> None:
    st.add_vectors([r.id for r in rows], np.stack([r.dense for r in rows]), None, [r.text for r in rows], [r.enh for r in rows],
                   [dict(r.meta) for r in rows])


class Model:
    """The rows as a list; a grouped query answered from nothing."""

    def __init__(self):
        self.rows: List[M.Row] = []

    def ranking(self, queries: np.ndarray, pred: Callable[[dict], bool]):
        """The full ranking of the live rows that pass `pred`, per query (shared by every shape asked under one filter)."""
        passing = np.asarray([i for i, r in enumerate(self.rows) if r.alive and pred(r.meta)], np.int64)
        return GR.rank_passing(np.stack([r.dense for r in self.rows]), queries, passing)

    def expected(self, ranking, key: str, top_k: int, group_size: int):
        """Per query the flat list [(id, score hex, enhanced text)] group by group."""
        seen: Dict[Any, int] = {}
        codes = np.asarray([seen.setdefault(identity(r.meta.get(key)), len(seen)) for r in self.rows], np.int64)
        s, i, _g = GR.group_all(*ranking, codes, top_k, group_size)
        return [[(self.rows[r].id, float(v).hex(), self.rows[r].enh) for v, r in zip(s[q].reshape(-1).tolist(), i[q].reshape(-1).tolist())
                 if r >= 0] for q in range(len(s))]


def got_of(results) -> List[tuple]:
    return [(r.id, float(r.score).hex(), r.enhanced_text) for r in results]


# ------------------------------------------------------------------------------------------------ stand-ins (CPU run)
class CpuGroupColumn:
    """Stand-in for `shards.GroupColumn`."""

    def __init__(self, device=0):
        self.codes = np.empty(0, np.int32)

    def append(self, codes):
        codes = np.asarray(codes, np.int32).reshape(-1)
        assert (codes >= 0).all()
        self.codes = np.concatenate([self.codes, codes])

    def __len__(self):
        return len(self.codes)

    def close(self):
        pass


class GroupedDense(CC.CompactDense):
    """`CompactDense` with `DenseShard.search_grouped`, answered by the oracle; counts its calls."""

    calls = 0

    def search_grouped(self, queries, n_groups, group_size, column, allow_words=None, n_allow=0, stream=None):
        type(self).calls += 1
        n = min(len(self.rows), len(column))
        passing = np.arange(n, dtype=np.int64) if allow_words is None else M._allowed(allow_words, n_allow, n)
        return GR.grouped_topk(self.rows, queries, column.codes, n_groups, group_size, passing)


@contextlib.contextmanager
def stand_ins():
    with M.stand_ins(dense=GroupedDense):
        saved = vs.GroupColumn
        vs.GroupColumn = CpuGroupColumn
        try:
            yield
        finally:
            vs.GroupColumn = saved


# ------------------------------------------------------------------------------------------------ the scenario
def check(st, model: Model, queries: np.ndarray, key: str, where: str, shapes=SHAPES, filters=FILTERS) -> int:
    """`query` and `query_batch` against the model for every shape and filter; returns the number of non-empty answers."""
    filled = 0
    for flt, pred in filters:
        ranking = model.ranking(queries, pred)
        for top_k, g in shapes:
            params = {"group_by_field": key, "group_size": g}
            want = model.expected(ranking, key, top_k, g)
            batch = st.query_batch(dense_queries=[q.tolist() for q in queries], top_k=top_k, search_type="dense", filter=flt,
                                   search_params=params)
            assert [got_of(b) for b in batch] == want, (where, "query_batch", top_k, g, flt)
            for i in (0, len(queries) - 1):
                one = st.query(dense_query=queries[i].tolist(), top_k=top_k, search_type="dense", filter=flt, search_params=params)
                assert got_of(one) == want[i] == got_of(batch[i]), (where, "query", top_k, g, flt, i)
            assert all(len(w) <= top_k * g for w in want)
            filled += sum(bool(w) for w in want)
    return filled


def scenario(make_store, load_store, tmp_dir, n_rows: int, n_queries: int, key: str = "document_id") -> None:
    """`make_store()` -> an empty dense-only store; `load_store(path)` -> the saved one."""
    model = Model()
    first = rows_of(n_rows, seed=11)
    st = make_store()
    fill(st, first)
    model.rows.extend(first)
    rng = np.random.default_rng(5)
    queries = np.concatenate([M.unit_rows(rng, n_queries - 2, DIM), np.stack([first[0].dense, first[40].dense])])
    assert check(st, model, queries, key, "fresh") > 0
    assert key in st._metadata.group_codes and len(st._metadata.group_codes[key]) == n_rows
    # deletes: single rows, and every row of one document
    gone = [r.id for r in first if r.serial % 5 == 2 or r.meta.get("document_id") == "d4"]
    st.delete(gone)
    for r in first:
        r.alive = r.alive and r.id not in set(gone)
    check(st, model, queries, key, "after delete", shapes=SHAPES[1:3])
    # an insert behind the built column: the codes are extended by the new rows only
    codes_before = st._metadata.group_codes[key]
    more = rows_of(max(n_rows // 8, 40), seed=12, first=n_rows)
    fill(st, more)
    model.rows.extend(more)
    check(st, model, queries, key, "after insert", shapes=SHAPES[1:3])
    assert st._metadata.group_codes[key] is codes_before and len(codes_before) == len(model.rows)
    # compact(): the columns are dropped and rebuilt lazily
    assert st.compact() == len(gone)
    model.rows = [r for r in model.rows if r.alive]
    assert st._metadata.group_codes == {} and st._metadata.group_cols == {}
    check(st, model, queries, key, "after compact", shapes=SHAPES[1:3])
    assert len(st._metadata.group_codes[key]) == len(model.rows)
    # the typing rules, on the store
    check(st, model, queries, "year", "year", shapes=[(10, 3)], filters=FILTERS[:2])
    check(st, model, queries, "no_such_key", "missing key", shapes=[(5, 2)], filters=FILTERS[:1])
    # save / load: nothing of the grouping is persisted
    st.delete([model.rows[3].id])
    model.rows[3].alive = False
    path = str(tmp_dir / "grouped-store")
    st.save(path)
    st.close()
    st = load_store(path)
    model.rows = [r for r in model.rows if r.alive]
    assert st._metadata.group_codes == {}
    check(st, model, queries, key, "after load", shapes=SHAPES[:2])
    st.close()


def refusals(make_store, with_int8: bool = True) -> None:
    """Every combination a grouped query refuses, each a ValueError that names what is supported."""
    import pytest

    rows = rows_of(60, seed=3)
    q = rows[0].dense.tolist()
    params = {"group_by_field": "document_id"}
    st = make_store()
    fill(st, rows)
    supported = "search_type='dense' on a single-GPU store"
    for kw in (dict(search_type="sparse"), dict(search_type="hybrid"), dict(search_type="full_text"),
               dict(search_type="dense", hybrid_weights={"dense": 1.0})):
        with pytest.raises(ValueError, match=supported):
            st.query(dense_query=q, sparse_query={1: 1.0}, text_query="x", top_k=3, search_params=params, **kw)
        with pytest.raises(ValueError, match=supported):
            st.query_batch(dense_queries=[q], sparse_queries=[{1: 1.0}], text_queries=["x"], top_k=3, search_params=params, **kw)
    with pytest.raises(ValueError, match="filter-only"):
        st.query(top_k=3, search_type="dense", filter='metadata["m"] < 5', search_params=params)
    with pytest.raises(ValueError, match="filter-only"):
        st.query_batch(dense_queries=[q, None], top_k=3, search_type="dense", search_params=params)
    for bad in (0, 65, -1, True, 2.5):
        with pytest.raises(ValueError, match="top_k"):
            st.query(dense_query=q, top_k=bad, search_type="dense", search_params=params)
    for bad in (0, 17, True, "3", 1.5):
        with pytest.raises(ValueError, match="group_size"):
            st.query(dense_query=q, top_k=3, search_type="dense", search_params=dict(params, group_size=bad))
    with pytest.raises(ValueError, match="strict_group_size"):
        st.query(dense_query=q, top_k=3, search_type="dense", search_params=dict(params, strict_group_size="yes"))
    # strict_group_size is accepted and changes nothing
    a = st.query(dense_query=q, top_k=3, search_type="dense", search_params=dict(params, group_size=2, strict_group_size=True))
    b = st.query(dense_query=q, top_k=3, search_type="dense", search_params={"params": dict(params, group_size=2)})
    assert got_of(a) == got_of(b) and a
    # an inexact key
    bad_rows = rows_of(5, seed=4, first=1000)
    bad_rows[2].meta["score"] = float("nan")
    fill(st, bad_rows)
    with pytest.raises(ValueError, match="NaN"):
        st.query(dense_query=q, top_k=3, search_type="dense", search_params={"group_by_field": "score"})
    assert st.query(dense_query=q, top_k=3, search_type="dense", search_params=params)      # other keys still group
    st.close()
    configs = [dict(index_type="IVF_FLAT")] + ([dict(dense_dtype="int8")] if with_int8 else [])
    for kw in configs:
        other = make_store(**kw)
        fill(other, rows)
        with pytest.raises(ValueError, match=supported):
            other.query(dense_query=q, top_k=3, search_type="dense", search_params=params)
        other.close()
