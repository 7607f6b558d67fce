"""Random operation sequences against `GpuVectorStore` over the exact CPU stand-ins, every answer compared with the brute-force
model of tests/store_model.py (ids and score bits, `==`).  The coverage assertions make the sequences' reach a condition; the
negative controls show that the run notices a stale cache, a wrong tie order, a half-done delete, a leaking mask and a wrong
fusion order; the repeated-id case states the `query_batch` / `query` disagreement this work found on its own."""
import numpy as np
import pytest

import store_model as M
from store_model import vs

SEEDS = range(6)


@pytest.mark.parametrize("name", M.HOST_CONFIGS)
def test_sequences_match_the_model_and_reach_every_transition(name, tmp_path):
    with M.stand_ins():
        total = M.run_config(name, SEEDS, tmp_path, host=True)
    M.check_coverage(M.CONFIGS[name], total, host=True)


def test_an_insert_inside_a_filtered_query_is_not_seen_by_it(tmp_path):
    total = M.Coverage()
    with M.stand_ins():
        for seed in SEEDS:
            total.merge(M.Runner(M.CONFIGS["f32_subset"], seed, tmp_path, host=True, race=True).run())
    assert total.seen.get("racing_add", 0) >= 6


# ------------------------------------------------------------------------------------------------ negative controls
def _fails(name, tmp_path, seeds=SEEDS, **runner):
    """The mismatches the sequences of `name` end in under an injected defect, one per failing seed (at least one)."""
    found = []
    for seed in seeds:
        try:
            M.Runner(M.CONFIGS[name], seed, tmp_path, host=True, **runner).run()
        except M.Mismatch as e:
            found.append(e)
    assert found, f"the model run did not notice the defect ({name})"
    return found


def _rows_got(e):
    """Model rows of the hits the store returned (by their unique enhanced text); None = a row the model dropped at a save."""
    row_of = {r.enh: r for r in e.runner.model.rows}
    return [row_of.get(hit[2]) for hit in e.got]


SINGLE = [("dense", None, 1), ("sparse", None, 1)]      # without fusion a wrong row set shows as one (fusion can turn it into ranks)


def _fuses(e):
    return e.op.split()[1].startswith(("hybrid", "weighted"))


def test_control_stale_masks_and_subsets(tmp_path, monkeypatch):
    with M.stand_ins():
        monkeypatch.setattr(vs.GpuVectorStore, "_drop_subsets", lambda self: None)
        found = _fails("f32_subset", tmp_path, modes=SINGLE)
    # a mask from before the last insert or delete: other ROWS than expected (a deleted row, or a new row missing), not another order
    assert all({hit[2] for hit in e.got} != {hit[2] for hit in e.want} for e in found)
    assert all("add" in " ".join(e.runner.log[1:]) or "delete" in " ".join(e.runner.log) for e in found)


class _TiesDescending(M.ModelDense):
    def search(self, queries, k, stream=None):
        n = len(self.rows)
        kk = min(k, n)
        s, i = M.T.dense_topk(self.rows[::-1], np.asarray(queries, np.float32), kk)
        return M._pad(s, np.where(i >= 0, n - 1 - i, -1), k)


def test_control_ties_broken_by_row_descending(tmp_path):
    with M.stand_ins(dense=_TiesDescending):
        found = _fails("f32_subset", tmp_path)
    for e in found:
        assert e.op.split()[1] == "dense" or _fuses(e), e.op                 # only what has a dense leg
        if e.op.split()[1] == "dense":                                       # the same score at the first difference, another row
            assert e.got[e.at][1] == e.want[e.at][1] and e.got[e.at][2] != e.want[e.at][2]
    assert any(e.op.split()[1] == "dense" for e in found)


def test_control_delete_clears_one_row_of_a_shared_id(tmp_path, monkeypatch):
    real = vs.GpuVectorStore._note_id

    def keep_first(self, key, row):
        if key not in self._id_rows:
            real(self, key, row)

    with M.stand_ins():
        monkeypatch.setattr(vs.GpuVectorStore, "_note_id", keep_first)
        found = _fails("f32_subset", tmp_path, modes=SINGLE)
    # a row the model has deleted comes back, and its id is one that several rows carry
    for e in found:
        dead = [r for r in _rows_got(e) if r is None or not r.alive]
        assert dead and all(sum(r.id == other.id for other in e.runner.model.rows) > 1 for r in dead if r is not None), e.op


def test_control_rows_beyond_the_mask_pass(tmp_path, monkeypatch):
    def leaky(mask, n):
        if mask is None or len(mask) >= n:
            return mask if mask is None else mask[:n]
        return np.concatenate([mask, np.ones(n - len(mask), dtype=bool)])

    with M.stand_ins():
        monkeypatch.setattr(vs.GpuVectorStore, "_fit_mask", staticmethod(leaky))
        found = _fails("f32_subset", tmp_path, race=True, modes=SINGLE)
    # the query that raced an insert returns rows of that insert (the 7 newest rows of the model)
    for e in found:
        newest = {r.enh for r in e.runner.model.rows[-7:]}
        assert "+racing add" in e.op and newest & {hit[2] for hit in e.got}, e.op


def test_control_fusion_in_another_method_order(tmp_path, monkeypatch):
    merge_rows, merge_hits = vs.rrf_merge_rows, vs.merge_hybrid_results

    def backwards(fn):
        return lambda lists, *a, **kw: fn(dict(reversed(list(lists.items()))), *a, **kw)

    with M.stand_ins():
        monkeypatch.setattr(vs, "rrf_merge_rows", backwards(merge_rows))
        monkeypatch.setattr(vs, "merge_hybrid_results", backwards(merge_hits))
        found = _fails("f32_subset", tmp_path)
    assert all(_fuses(e) for e in found)


# ------------------------------------------------------------------------------------------------ rows that share an id
@pytest.mark.parametrize("n_q", [2, 70])
@pytest.mark.parametrize("weights", [None, {"dense": 0.7, "sparse": 0.3}], ids=["hybrid", "weighted"])
def test_rows_that_share_an_id_fuse_as_one_candidate(n_q, weights):
    """60 rows over 20 ids: `query_batch` == per-query `query` == the model (fusion by id, hybrid_search.py:73-129)."""
    cfg = M.CONFIGS["f32_subset"]
    rng = np.random.default_rng(5)
    dense = M.unit_rows(rng, 60, cfg.dim)
    rows = [M.Row(f"id{i % 20}", i, dense[i], M.sparse_row(rng, 6), f"text {i}", [], M.metadata_of(i)) for i in range(60)]
    model = M.Model(cfg)
    model.add(rows)
    queries = [{"dense": q, "sparse": M.sparse_row(rng, 5)} for q in M.unit_rows(rng, n_q, cfg.dim)]
    kw = dict(top_k=5, hybrid_weights=weights) if weights else dict(top_k=5, search_type="hybrid")
    want = [model.expected(hits) for hits in model.answer("weighted" if weights else "hybrid", queries, 5, 0, weights, 60)]
    with M.stand_ins():
        st = vs.GpuVectorStore(dense_dim=cfg.dim, sparse_vocab=M.VOCAB)
        st.add_vectors([r.id for r in rows], dense, [r.sparse for r in rows], [r.text for r in rows], [r.enh for r in rows],
                       [r.meta for r in rows])
        assert not st._ids_unique
        batch = st.query_batch(dense_queries=[q["dense"].tolist() for q in queries], sparse_queries=[q["sparse"] for q in queries], **kw)
        single = [st.query(dense_query=q["dense"].tolist(), sparse_query=q["sparse"], **kw) for q in queries]
    assert [M.got_of(r) for r in single] == want
    assert [M.got_of(r) for r in batch] == want
    assert any(len({r.id for r in res}) == len(res) == 5 for res in batch)


def test_unique_ids_keep_the_array_fusion(monkeypatch):
    """Stores whose ids are unique fuse a batch in one `rrf_merge_rows` call, as before; `load` restores the flag."""
    cfg = M.CONFIGS["f32_subset"]
    rng = np.random.default_rng(6)
    dense = M.unit_rows(rng, 40, cfg.dim)
    calls = []
    real = vs.rrf_merge_rows
    monkeypatch.setattr(vs, "rrf_merge_rows", lambda lists, *a, **kw: calls.append(next(iter(lists.values())).shape[0]) or real(lists, *a, **kw))
    with M.stand_ins():
        st = vs.GpuVectorStore(dense_dim=cfg.dim, sparse_vocab=M.VOCAB)
        st.add_vectors([f"id{i}" for i in range(40)], dense, [M.sparse_row(rng, 6) for _ in range(40)], [""] * 40, [""] * 40, [{}] * 40)
        assert st._ids_unique
        st.query_batch(dense_queries=dense[:3].tolist(), sparse_queries=[M.sparse_row(rng, 5) for _ in range(3)], top_k=5)
        assert calls == [3]
        st.add_vectors(["id7"], dense[:1], [M.sparse_row(rng, 6)], [""], [""], [{}])
        assert not st._ids_unique
        st.delete(["id7"])
        assert not st._ids_unique          # conservative after a delete
