"""The random operation sequences of tests/sharded_model.py against a ROW-SHARDED `GpuVectorStore` on the device, one seed per
case, every answer `==` the brute-force model in ids and score bits on every rank:

  * world 2 over gloo, both ranks on GPU 0 (as tests/test_sharded_gpu.py): the real `DenseShard` / `SparseShard` / `TextIndex`,
    host lists, the cross-rank merge on the device; every case of `sharded_model.CASES` a world of 2 can run;
  * world 1 with the `nccl` backend (started as tests/test_nccl_gpu.py starts it): the device-resident route -- lists written
    through the HBM row table, ONE all-gather, the merge in place, sharded full text with device lists -- which is exactly the
    code the 8-GPU run takes.  The worker counts the calls of `_device_topk_resident` through a wrapper.

One spawn per world (module scope); the parametrised tests read their rows from its reports and take no time of their own.
A failing library call, a dead worker or a world that does not answer ends the session: nothing more is launched."""
import pytest

import sharded_model as S

pytestmark = pytest.mark.gpu

# One seed per case, chosen on the CPU (the draws are the same there): each passes through a save + load and, between them, the
# seeds of a world pass through every condition of `coverage_wanted`.
GLOO2 = {"f32_subset": 0, "f32_noprefilter_dim72": 0, "f32_bitmap_device_large": 0, "bf16_subset_large": 3, "bf16_bitmap": 2,
         "three_way": 1, "text_only": 1, "falsy_id": 2, "f32_subset_replicated": 0, "three_way_replicated": 0}
NCCL1 = {"f32_subset": 0, "bf16_subset_large": 0, "three_way": 0, "falsy_id": 0}
# told per case whatever the seed count: a save + load with rank 0's reopen, and what the case is named for
PER_CASE = ("query_after_load", "reopen_world1")


def _spawn(world, backend, jobs, tmp):
    try:
        return S.run_world(world, dict(backend=backend, host=False, jobs=list(jobs.items()), tmp=str(tmp)))
    except S.WorldFailed as e:
        pytest.exit(f"sharded store model: {e}", returncode=3)


@pytest.fixture(scope="module")
def gloo2(tmp_path_factory):
    assert sorted(GLOO2) == sorted(S.cases_of(2, host=False))
    return _spawn(2, "gloo", GLOO2, tmp_path_factory.mktemp("gloo2"))


@pytest.fixture(scope="module")
def nccl1(tmp_path_factory):
    return _spawn(1, "nccl", NCCL1, tmp_path_factory.mktemp("nccl1"))


def _check_case(name, world, sequences):
    case = S.CASES[name]
    for ranks in sequences:
        for rec in ranks:
            assert rec["mismatch"] is None, rec["mismatch"]["message"]
            assert rec["ops"] == S.N_OPS and rec["empty"] * 4 <= rec["queries"]
    seen = S.merged_seen(sequences)
    rec = sequences[0][0]
    print(f"{name} world {world}: {rec['seconds']:.1f} s, rows up to {rec['rows_max']}, {rec['ops']} operations, {rec['queries']} queries, "
          f"searches {rec['counts']}, seen {dict(sorted(seen.items()))}")
    wanted = [c for c in S.coverage_wanted(case, world, False) if c in PER_CASE + ("falsy_id_fusion", "rrf_device_batch")]
    S.check_coverage(case, world, False, seen, wanted)
    if case.cfg(world).start > 4096:
        assert rec["rows_max"] > 4200 * world
    return seen


def test_gloo2_every_rank_received_the_same_answers(gloo2):
    assert [(r["backend"], r["on_gpu"], r["exchange_backend"]) for r in gloo2] == [("gloo", False, "host")] * 2
    S.assert_ranks_agree(gloo2)


@pytest.mark.parametrize("name", list(GLOO2))
def test_gloo2_sequences_match_the_model_on_the_device(name, gloo2):
    sequences = S.by_case(gloo2)[name]
    assert [ranks[0]["seed"] for ranks in sequences] == [GLOO2[name]]
    _check_case(name, 2, sequences)
    assert not sequences[0][0]["counts"].get("resident")          # host lists under gloo


def test_gloo2_cases_reach_every_sharded_condition_between_them(gloo2):
    total, wanted = {}, set()
    for name, sequences in S.by_case(gloo2).items():
        for k, v in S.merged_seen(sequences).items():
            total[k] = total.get(k, 0) + v
        wanted |= set(S.coverage_wanted(S.CASES[name], 2, False))
    missing = sorted(w for w in wanted if not total.get(w))
    assert not missing, f"the cases never passed through {missing} (seen: {total})"


@pytest.mark.parametrize("name", list(NCCL1))
def test_nccl1_sequences_take_the_resident_route_and_match_the_model(name, nccl1):
    assert [(r["backend"], r["on_gpu"], r["exchange_backend"]) for r in nccl1] == [("nccl", True, "vrag_comm")]
    sequences = S.by_case(nccl1)[name]
    assert [ranks[0]["seed"] for ranks in sequences] == [NCCL1[name]]
    seen = _check_case(name, 1, sequences)
    S.check_coverage(S.CASES[name], 1, False, seen)
    counts = sequences[0][0]["counts"]
    # every dense / sparse search of at most DEVICE_K rows kept its lists in HBM
    assert counts.get("wanted", 0) > 20 and counts.get("resident", 0) == counts["wanted"], counts
    # and the full-text searches of at most DEVICE_K rows wrote device lists into the exchange payload
    text_lists = counts.get("slots", 0) - counts["resident"]
    assert text_lists > 0 if S.CASES[name].cfg(1).text else text_lists == 0, counts
