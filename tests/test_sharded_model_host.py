"""The random operation sequences of tests/sharded_model.py against a ROW-SHARDED `GpuVectorStore` at worlds 2 and 3 over gloo, on
the exact CPU stand-ins with the host merge: every answer `==` the brute-force model on every rank, every rank's answers the
same, rank 0's world -> 1 reopen at every save + load, and the coverage conditions of `sharded_model.coverage_wanted` per case
over its seeds.  One spawn per world (module scope); the parametrised tests read their rows from its reports.

The negative controls inject one defect each inside the workers of a world of 2 and show that the run ends in the mismatch that
defect must cause: a merge that leaves ties in list order, a `union_mask` / `sum_int64` that returns the local array, BM25
totals kept over a delete, a row table shifted at load."""
import pytest

import sharded_model as S

# Chosen on the CPU so that the MODEL passes through every condition of `coverage_wanted` between them (the draws do not depend
# on the store, so they hold for every run); the tiny cases also so that at most a quarter of a sequence's queries expect an
# empty answer (a store of two rows answers most filters with nothing).
SEEDS = {
    2: {name: (0, 1, 2) for name in S.cases_of(2, host=True)},
    3: {name: (0, 1, 2) for name in S.cases_of(3, host=True)},
}
SEEDS[2]["f32_bitmap_device_large"], SEEDS[3]["f32_bitmap_device_large"] = (0, 1), (0, 4)      # 8 400 / 12 600 rows and more: two seeds
SEEDS[3]["f32_subset_tiny"] = SEEDS[3]["three_way_tiny"] = (0, 1, 3)
PAIRS = [(world, name) for world in SEEDS for name in SEEDS[world]]


@pytest.fixture(scope="module")
def world_reports(tmp_path_factory):
    """world -> the ranks' reports; a world is spawned once, and a world that failed is not started again."""
    cache = {}

    def get(world):
        if world not in cache:
            jobs = [(name, seed) for name, seeds in SEEDS[world].items() for seed in seeds]
            try:
                cache[world] = S.run_world(world, dict(backend="gloo", host=True, jobs=jobs, tmp=str(tmp_path_factory.mktemp(f"w{world}"))))
            except S.WorldFailed as e:
                cache[world] = e
        if isinstance(cache[world], Exception):
            pytest.fail(str(cache[world]))
        return cache[world]

    return get


@pytest.mark.parametrize("world", list(SEEDS))
def test_every_rank_received_the_same_answers(world, world_reports):
    reports = world_reports(world)
    assert [r["backend"] for r in reports] == ["gloo"] * world and not any(r["on_gpu"] for r in reports)
    S.assert_ranks_agree(reports)
    assert all(len(rec["digests"]) >= 20 for rec in reports[0]["results"])          # every query of a sequence was digested


@pytest.mark.parametrize("world,name", PAIRS)
def test_sequences_match_the_model_on_every_rank(world, name, world_reports):
    sequences = S.by_case(world_reports(world))[name]
    assert [ranks[0]["seed"] for ranks in sequences] == list(SEEDS[world][name])
    for ranks in sequences:
        for rec in ranks:
            assert rec["mismatch"] is None, rec["mismatch"]["message"]
            assert rec["ops"] == S.N_OPS and rec["empty"] * 4 <= rec["queries"]
    case = S.CASES[name]
    S.check_coverage(case, world, True, S.merged_seen(sequences))
    if case.cfg(world).start > 4096:
        assert max(ranks[0]["rows_max"] for ranks in sequences) > 4200 * world


# ------------------------------------------------------------------------------------------------ negative controls
SINGLE = [("dense", None, 1), ("sparse", None, 1)]         # without fusion a wrong row shows as one
NO_SEARCH = (0.30, 0.10, 0.0, 0.0, 0.04, 0.40)             # add, delete, save_load and filter-only queries
NO_BROWSE = (0.30, 0.10, 0.12, 0.40, 0.08, 0.0)            # no filter-only query
DELETES = (0.10, 0.30, 0.15, 0.40, 0.03, 0.02)             # a delete before every other query, few inserts between them


def _control(defect, jobs, tmp_path, **spec):
    """(reports, the mismatches the ranks recorded, at least one) of a world of 2 under `defect`."""
    try:
        reports = S.run_world(2, dict(backend="gloo", host=True, jobs=jobs, tmp=str(tmp_path), defect=defect, **spec))
    except S.WorldFailed as e:
        pytest.fail(str(e))
    found = [rec["mismatch"] for rep in reports for rec in rep["results"] if rec["mismatch"]]
    assert found, f"the sharded model run did not notice the defect {defect!r}"
    return reports, found


def _kind(e):
    return e["op"].split()[1]


def test_control_merge_breaks_ties_by_list_order(tmp_path):
    reports, found = _control("merge_ties_by_list_order", [("f32_subset", s) for s in (0, 1, 2)], tmp_path, modes=SINGLE)
    for e in found:       # the same score at the first difference, another row
        assert _kind(e) in ("dense", "sparse") and e["at"] < min(len(e["got"]), len(e["want"])), e["message"]
        assert e["got"][e["at"]][1] == e["want"][e["at"]][1] and e["got"][e["at"]][2] != e["want"][e["at"]][2], e["message"]
    assert any(_kind(e) == "dense" for e in found)
    S.assert_ranks_agree(reports)              # every rank merges the same lists the same wrong way


def test_control_union_mask_returns_the_local_array(tmp_path):
    reports, found = _control("union_mask_local", [("f32_subset", s) for s in (0, 1, 2)], tmp_path, op_p=NO_SEARCH)
    for e in found:       # a filtered browse loses exactly the rows of the other rank
        assert e["op"].startswith("filter_only") and not e["op"].endswith("f=0"), e["message"]
        owner = [e["owner_of"][hit[2]] for hit in e["want"]]
        mine = [hit for hit, o in zip(e["want"], owner) if o == e["rank"]]
        assert len(mine) < len(e["want"]) and e["got"][:len(mine)] == mine, e["message"]
        assert all(e["owner_of"][hit[2]] == e["rank"] for hit in e["got"]), e["message"]
    assert {e["rank"] for e in found} == {0, 1}
    with pytest.raises(AssertionError, match="received different answers"):
        S.assert_ranks_agree(reports)


def test_control_sum_int64_returns_the_local_array(tmp_path):
    jobs = [("three_way", s) for s in (0, 1, 2)] + [("f32_subset", 0)]
    reports, found = _control("sum_int64_local", jobs, tmp_path)
    assert all(rec["mismatch"] is None for rep in reports for rec in rep["results"] if rec["case"] == "f32_subset")
    differ = 0
    for e in found:       # only what has a full-text leg; there, rows both lists hold carry other score bits
        assert "full_text" in e["op"], e["message"]
        want = {hit[2]: hit[1] for hit in e["want"]}
        differ += _kind(e) == "full_text" and any(hit[2] in want and want[hit[2]] != hit[1] for hit in e["got"])
    assert differ


def test_control_text_totals_kept_over_a_delete(tmp_path):
    _reports, found = _control("text_totals_kept_over_delete", [("three_way", s) for s in (0, 1, 2)], tmp_path, op_p=DELETES)
    for e in found:       # a full-text leg, and the last change before it was a delete (an insert or a load sums again)
        assert "full_text" in e["op"], e["message"]
        changes = [op.split()[0] for op in e["log"][:e["op_index"]] if op.split()[0] in ("add", "delete", "save_load")]
        assert changes[-1] == "delete", e["message"]


def test_control_row_table_shifted_at_load(tmp_path):
    reports, found = _control("owned_shifted_at_load", [("f32_subset", s) for s in (0, 1, 2)], tmp_path, op_p=NO_BROWSE)
    for e in found:
        assert "save_load" in e["log"][:e["op_index"]], e["message"]
    # every sequence that loads notices, on every rank; one that never loads has nothing to notice
    for rep in reports:
        for rec in rep["results"]:
            assert (rec["mismatch"] is not None) == bool(rec["seen"].get("query_after_load")), (rec["case"], rec["seed"], rec["rank"])
