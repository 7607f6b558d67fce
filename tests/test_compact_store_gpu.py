"""`GpuVectorStore.compact()` on the device: the operation sequences of tests/store_model.py with compaction steps drawn among
them (tests/compact_cases.py), one seed of each configuration whose device structures differ -- fp32 rows with subset shards,
fp32 rows with the prefilter image, device filter columns and the filtered kernels, bf16 rows, SQ8 rows, an IVF overlay, and the
three-method store.  Every answer `==` the brute-force model in ids and score bits; around each compaction the same queries return
identical ids, scores, texts and metadata; and the sequences must have compacted with dead rows present, inserted after a
compaction, and (IVF) kept `trained_rows` across one.

A failing library call ends the session: nothing more is launched."""
import pytest

import compact_cases as CC
import store_model as M

pytestmark = pytest.mark.gpu

SEEDS = {"f32_subset": 0, "f32_bitmap_device_large": 0, "bf16_bitmap": 0, "int8_bitmap_large": 0, "f32_ivf_large": 0, "three_way": 0}


@pytest.mark.parametrize("name", list(SEEDS))
def test_sequences_with_compactions_match_the_model_on_the_device(name, tmp_path):
    cfg = M.CONFIGS[name]
    try:
        cover = CC.CompactRunner(cfg, SEEDS[name], tmp_path, host=False).run()
    except M.StoreFault as e:
        pytest.exit(f"store model with compactions: {e}", returncode=3)
    print(f"{name}: rows up to {cover.rows_max}, reached {dict(sorted(cover.seen.items()))}")
    assert cover.seen.get("compact_dead", 0) >= 1, cover.seen
    assert cover.seen.get("compact_then_add", 0) >= 1, cover.seen
    if cfg.ivf:
        assert cover.seen.get("ivf_compact", 0) >= 1, cover.seen
