"""`GpuVectorStore.compact()` over the exact CPU stand-ins: the state it leaves is the state `load(save())` produces, column by
column; what it returns; who may not call it; when `auto_compact` calls it; deletes and searches after it; a compaction that
lands inside a filtered query; and two negative controls -- a device layer that compacts out of order, and a store whose
epoch does not move -- that the comparisons notice.  The rows are store_model's dyadic-grid rows (entries 0, +-1/8, +-2/8: every
score is exact and rows tie exactly, so a wrong order among equal scores shows)."""
from operator import attrgetter

import numpy as np
import pytest

import compact_cases as CC
import store_model as M
from store_model import vs

DIM = 64


def _stand_ins(dense=None):
    return M.stand_ins(dense=dense or CC.CompactDense)


def _rows(n, seed=3, text=False):
    rng = np.random.default_rng(seed)
    dense = M.unit_rows(rng, n, DIM)
    return [M.Row(f"id{i}", i, dense[i], M.sparse_row(rng, 6), M.text_row(rng)[0] if text else f"text {i}", [], M.metadata_of(i))
            for i in range(n)]


def _fill(st, rows):
    st.add_vectors([r.id for r in rows], np.stack([r.dense for r in rows]), [r.sparse for r in rows], [r.text for r in rows],
                   [r.enh for r in rows], [dict(r.meta) for r in rows])


def _store(rows, **kw):
    st = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=M.VOCAB, **kw)
    _fill(st, rows)
    return st


def _dense_answers(st, rows, flt=None, k=10):
    return [CC.answers(st.query(dense_query=r.dense.tolist(), top_k=k, search_type="dense", filter=flt)) for r in rows[:5]]


COLUMNS = ("_ids", "_texts", "_enh", "_meta", "_all_ids_truthy", "_ids_unique", "_id_seen", "_id_rows", "_metadata.value_indexes", "_masks",
           "_subsets", "_documents")
ARRAYS = ("_alive", "_owned", "_dense_rows", "_sp_ptr", "_sp_idx", "_sp_val")


@pytest.mark.parametrize("text", [False, True], ids=["dense_sparse", "three_way"])
def test_state_after_compact_is_the_state_after_save_and_load(tmp_path, text):
    rows = _rows(300, text=text)
    with _stand_ins():
        st = _store(rows, enable_full_text=text)
        st.add_documents([{"id": "doc", "title": "t", "metadata": {"document_id": "d3"}}])
        _dense_answers(st, rows, 'metadata["document_id"] == "d3"')          # a value index, a mask, a subset shard
        gone = [r.id for r in rows if r.serial % 3 == 1] + ["id0", "id299"]
        st.delete(gone)
        _fill(st, _rows(20, seed=4, text=text)[10:])                             # ten rows not flushed yet (ids id10 .. id19 again)
        st.delete(["id12"])                                                      # both rows of that id
        dead = int((~st._alive.data).sum())
        st.save(str(tmp_path / "s"))
        loaded = vs.GpuVectorStore.load(str(tmp_path / "s"))
        assert st.compact() == dead > 100
        assert len(st) == len(loaded) == 310 - dead
        for name in COLUMNS:
            assert attrgetter(name)(st) == attrgetter(name)(loaded), name
        for name in ARRAYS:
            a, b = getattr(st, name).data, getattr(loaded, name).data
            assert a.dtype == b.dtype and np.array_equal(a, b), name
        assert st._id_rows is None and st._metadata.value_indexes == {} and not st._ids_unique
        # after a flush the device layers hold the same rows, and every method answers alike
        live = [r for r in rows if r.id not in set(gone) | {"id12"}]
        for kw in (dict(search_type="dense"), dict(search_type="sparse"), dict(search_type="hybrid"),
                   dict(search_type="dense", filter='metadata["m"] >= 20 and metadata["m"] < 60')):
            for r in live[:4]:
                q = dict(dense_query=r.dense.tolist(), sparse_query=r.sparse, top_k=7, **kw)
                assert CC.answers(st.query(**q)) == CC.answers(loaded.query(**q)), kw
        if text:
            for words in ("common", M.WORDS[0], M.WORDS[1] + " " + M.WORDS[2]):
                q = dict(text_query=words, top_k=7, search_type="full_text")
                assert CC.answers(st.query(**q)) == CC.answers(loaded.query(**q)), words
        assert np.array_equal(st._dense.rows, loaded._dense.rows)
        assert len(st._sparse_parts) == len(loaded._sparse_parts) == 1
        for a, b in zip(st._sparse_parts[0][0].csr, loaded._sparse_parts[0][0].csr):
            assert np.array_equal(a, b)
        assert st.compact() == 0


def test_compact_of_a_clean_store_returns_zero_and_touches_nothing():
    rows = _rows(50)
    with _stand_ins():
        st = _store(rows)
        _dense_answers(st, rows)
        shard, ids, epoch = st._dense, st._ids, st._epoch
        assert st.compact() == 0
        assert st._dense is shard and st._ids is ids and st._epoch == epoch and not st._dirty and len(st) == 50
        st.delete(["nobody"])
        assert st.compact() == 0
        empty = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=M.VOCAB)
        assert empty.compact() == 0 and len(empty) == 0


def test_len_is_the_live_count_and_everything_may_go():
    rows = _rows(40)
    with _stand_ins():
        st = _store(rows)
        st.delete([r.id for r in rows[:15]])
        assert len(st) == 40 and st.compact() == 15 and len(st) == 25
        assert [x[0][0] for x in _dense_answers(st, rows[20:])] == [r.id for r in rows[20:25]]
        st.delete([r.id for r in rows])
        assert st.compact() == 25 and len(st) == 0
        assert st.query(dense_query=rows[0].dense.tolist(), sparse_query=rows[0].sparse, top_k=3) == []
        _fill(st, rows[:5])
        assert len(st) == 5 and _dense_answers(st, rows)[0][0][0] == "id0"


class _OneRank:
    rank, world, on_gpu = 0, 1, False


def test_a_sharded_store_refuses():
    with _stand_ins():
        st = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=M.VOCAB, comm=_OneRank())
        with pytest.raises(ValueError, match="single-GPU"):
            st.compact()
        with pytest.raises(ValueError, match="single-GPU"):
            vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=M.VOCAB, comm=_OneRank(), auto_compact=0.5)
        for bad in (0, 1, 1.5, -0.1, True, "half"):
            with pytest.raises(ValueError, match="auto_compact"):
                vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=M.VOCAB, auto_compact=bad)


def test_auto_compact_fires_above_its_threshold_and_not_at_it(tmp_path):
    rows = _rows(100)
    with _stand_ins():
        plain = _store(rows)
        plain.delete([r.id for r in rows[:90]])
        assert len(plain) == 100 and plain.auto_compact is None          # None: never implicit
        st = _store(rows, auto_compact=0.25)
        st.delete([r.id for r in rows[:25]])
        assert len(st) == 100                                              # 25 % dead is not more than 25 %
        st.delete([rows[25].id])
        assert len(st) == 74 and st._alive.data.all()
        st.delete([r.id for r in rows[26:44]])                             # 18 of 74: under the fraction again
        assert len(st) == 74
        st.delete([rows[44].id])                                           # 19 of 74 = 25.7 %
        assert len(st) == 55
        st.save(str(tmp_path / "s"))
        again = vs.GpuVectorStore.load(str(tmp_path / "s"), auto_compact=0.5)
        assert again.auto_compact == 0.5 and vs.GpuVectorStore.load(str(tmp_path / "s")).auto_compact is None
        again.delete([r.id for r in rows[45:73]])                          # 28 of 55 = 50.9 %
        assert len(again) == 27


def test_delete_by_id_after_a_compaction_finds_the_renumbered_rows():
    rows = _rows(60)
    with _stand_ins():
        st = _store(rows)
        st.delete(["id3"])                                                 # builds the id table
        assert st._id_rows is not None
        st.delete([r.id for r in rows[:30]])
        assert st.compact() == 30 and st._id_rows is None
        st.delete(["id31", "id59", "id3"])
        assert [i for i, a in enumerate(st._alive.data) if not a] == [1, 29]
        got = _dense_answers(st, rows[30:35], k=3)
        assert [g[0][0] for i, g in enumerate(got) if i != 1] == ["id30", "id32", "id33", "id34"]     # each finds itself first
        assert "id31" not in {hit[0] for g in got for hit in g}
        assert st.compact() == 2 and len(st) == 28


def _racing_compact(st, query):
    """`query()` with a `compact()` right after the query has built its row mask (the hook of `Runner._racing_single`)."""
    build, raced = st._mask, []

    def mask_then_compact(flt):
        mask = build(flt)
        if mask is not None and not raced:
            raced.append(st.compact())
        return mask

    st._mask = mask_then_compact
    try:
        return query(), raced
    finally:
        del st._mask


@pytest.mark.parametrize("route", ["subset", "bitmap"])
def test_a_compaction_inside_a_filtered_query_gives_one_sides_answer(route):
    rows = _rows(400)
    flt = 'metadata["m"] >= 20 and metadata["m"] < 60'
    with _stand_ins():
        st = _store(rows, filter_route=route)
        ref = _store(rows, filter_route=route)
        for s in (st, ref):
            s.delete([r.id for r in rows if r.serial % 5 in (0, 3)])
        probe = rows[21]
        ask = dict(dense_query=probe.dense.tolist(), sparse_query=probe.sparse, top_k=8, filter=flt)
        before = CC.answers(ref.query(**ask))
        ref.compact()
        after = CC.answers(ref.query(**ask))
        assert before == after and len(before) == 8                        # both sides hold the same answer, under other row numbers
        got, raced = _racing_compact(st, lambda: st.query(**ask))
        assert raced == [160] and len(st) == 240
        assert CC.answers(got) == before
        batch, raced = _racing_compact(ref, lambda: ref.query_batch(dense_queries=[probe.dense.tolist()] * 2,
                                                                      sparse_queries=[probe.sparse] * 2, top_k=8, filter=flt))
        assert raced == [0] and [CC.answers(b) for b in batch] == [before, before]


def test_control_a_store_whose_epoch_stands_still_mixes_the_two_sides(monkeypatch):
    """The same race with the epoch left where it was: the query decodes rows of the new numbering through the mask of the old."""
    rows = _rows(400)
    flt = 'metadata["m"] >= 20 and metadata["m"] < 60'
    real = vs.GpuVectorStore.compact

    def compact_quietly(self):
        epoch = self._epoch
        try:
            return real(self)
        finally:
            self._epoch = epoch

    with _stand_ins():
        st = _store(rows)
        st.delete([r.id for r in rows if r.serial % 5 in (0, 3)])
        probe = rows[21]
        ask = dict(dense_query=probe.dense.tolist(), sparse_query=probe.sparse, top_k=8, filter=flt)
        want = CC.answers(st.query(**ask))
        monkeypatch.setattr(vs.GpuVectorStore, "compact", compact_quietly)
        try:
            got = CC.answers(_racing_compact(st, lambda: st.query(**ask))[0])
        except Exception:
            got = None
        assert got != want


@pytest.mark.parametrize("name", ["f32_subset", "three_way"])
def test_sequences_with_compactions_match_the_model(name, tmp_path):
    total = M.Coverage()
    with _stand_ins():
        for seed in (0, 1, 2):
            total.merge(CC.CompactRunner(M.CONFIGS[name], seed, tmp_path, host=True).run())
    assert total.seen.get("compact_dead", 0) >= 2 and total.seen.get("compact_then_add", 0) >= 1, total.seen


def test_control_a_compaction_that_reorders_rows_is_caught(tmp_path):
    """The last live row moved into the first hole: the right set of rows under the wrong numbers.  Caught by the queries around
    the compaction (another id, text or metadata at a rank) or by the model comparison of a later query."""
    found = []
    with _stand_ins(dense=CC.LastRowIntoFirstHole):
        for seed in (0, 1, 2):
            try:
                CC.CompactRunner(M.CONFIGS["f32_subset"], seed, tmp_path, host=True, modes=[("dense", None, 1)]).run()
            except M.Mismatch as e:
                found.append(e)
    assert found, "the run did not notice the reordering compaction"
    assert all("compact" in " ".join(e.runner.log) for e in found)
