"""SQ8 dense rows on the host: properties of the quantisation rule as tests/sq8_ref.py restates it, what the rule costs in
recall on a planted-neighbour corpus, the constructor's refusals (checked before any device is touched), and the register
budget of the kernels of csrc/sq8.hip."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sq8_ref as R
import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import vector_stores as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_codes_stay_in_range_and_the_largest_component_maps_to_127():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((500, 37)) * 10.0 ** rng.uniform(-3, 3, (500, 1))).astype(np.float32)
    codes, scales = R.quantize(x)
    assert codes.dtype == np.int8 and scales.dtype == np.float32 and codes.shape == x.shape and scales.shape == (500,)
    assert codes.min() >= -127 and codes.max() <= 127
    top = np.abs(x).argmax(axis=1)
    rows = np.arange(500)
    assert np.array_equal(codes[rows, top], np.where(x[rows, top] > 0, 127, -127))
    assert np.array_equal(scales, np.abs(x).max(axis=1) / np.float32(127.0))
    one, s1 = R.quantize(x[7])                       # a single vector is a batch of one
    assert np.array_equal(one[0], codes[7]) and s1[0] == scales[7]


def test_a_zero_row_has_zero_codes_and_scale_zero():
    x = np.zeros((3, 24), np.float32)
    x[1, 5] = -2.5
    codes, scales = R.quantize(x)
    assert not codes[0].any() and not codes[2].any() and scales[0] == 0 and scales[2] == 0
    assert scales.view(np.uint32)[0] == 0            # +0, not -0 and not NaN
    assert codes[1, 5] == -127 and np.count_nonzero(codes[1]) == 1


def test_halves_round_to_even():
    # m = 127 -> s = 1 exactly, so the quotients are the components themselves
    x = np.array([[127.0, 0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 126.5, -126.5, 0.49999997, 2.5000002]], np.float32)
    codes, scales = R.quantize(x)
    assert scales[0] == 1.0
    assert codes[0].tolist() == [127, 0, 2, 2, 4, 0, -2, -2, 126, -126, 0, 3]


def test_scores_are_the_three_rounding_recipe():
    rng = np.random.default_rng(2)
    cq, cr = rng.integers(-127, 128, (5, 4096)).astype(np.int8), rng.integers(-127, 128, (9, 4096)).astype(np.int8)
    cq[0], cr[0] = 127, 127                          # the largest integer dot of the contract: 4096 * 127^2 > 2^24
    sq, sr = rng.uniform(1e-3, 1.0, 5).astype(np.float32), rng.uniform(1e-3, 1.0, 9).astype(np.float32)
    S = R.scores(cq, sq, cr, sr)
    assert S.dtype == np.float32
    for q in range(5):
        for r in range(9):
            idot = int(cq[q].astype(np.int64) @ cr[r].astype(np.int64))
            assert S[q, r] == np.float32(idot) * np.float32(sq[q] * sr[r])
    s, i = R.topk(np.array([[1.0, 3.0, 3.0, -1.0]], np.float32), 6)
    assert i.tolist() == [[1, 2, 0, 3, -1, -1]] and np.isneginf(s[0, 4:]).all()
    s, i = R.topk(np.array([[1.0, 3.0, 3.0, -1.0]], np.float32), 2, passing=[0, 2, 3])
    assert i.tolist() == [[2, 0]]


# ---------------------------------------------------------------------------------------------------------------- recall
@pytest.mark.parametrize("dim,n", [(64, 2_000), (768, 20_000)])
def test_planted_neighbour_is_found(dim, n):
    """n unit Gaussian rows, 64 queries = row[i] + 0.5 N(0, 1) / sqrt(dim), renormalised: the int8 top-1 is the planted row for
    every query (recall@10 against the fp32 ranking is printed: 0.99 and 0.98)."""
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = X[:64] + (0.5 * rng.standard_normal((64, dim)) / np.sqrt(dim)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    _s, ids = R.search(X, Q, 10)
    exact = np.argsort(-(Q.astype(np.float64) @ X.astype(np.float64).T), axis=1, kind="stable")[:, :10]
    recall = np.mean([len(set(ids[q]) & set(exact[q])) / 10 for q in range(64)])
    print(f"dim {dim}, n {n}: recall@10 against fp32 {recall:.3f}")
    assert np.array_equal(ids[:, 0], np.arange(64))


# ---------------------------------------------------------------------------------------------------------------- the store's refusals
def test_int8_refusals_need_no_device():
    with pytest.raises(ValueError, match="single-GPU"):
        VS.GpuVectorStore(dense_dtype="int8", distributed=True)
    with pytest.raises(ValueError, match="single-GPU"):
        VS.GpuVectorStore(dense_dtype="int8", comm=object())
    with pytest.raises(ValueError, match="IVF_FLAT"):
        VS.GpuVectorStore(dense_dtype="int8", index_type="IVF_FLAT")
    for bad in ("fp16", "INT8", "sq8", None):
        with pytest.raises(ValueError, match="'f32', 'bf16' or 'int8'"):
            VS.GpuVectorStore(dense_dtype=bad)
    with pytest.raises(ValueError, match="'f32', 'bf16' or 'int8'"):
        VS.check_dense_dtype("f16", "FLAT", False)
    for dtype in ("f32", "bf16"):                    # the existing dtypes: sharded and IVF_FLAT as before
        VS.check_dense_dtype(dtype, "FLAT", True)
        VS.check_dense_dtype(dtype, "IVF_FLAT", False)
    VS.check_dense_dtype("int8", "FLAT", False)
    assert VS.Sq8Shard.__name__ == "Sq8Shard" and VS.DENSE_DTYPES == ("f32", "bf16", "int8")


def test_int8_store_builds_sq8_shards(monkeypatch):
    """The store's part on a CPU box: `dense_dtype="int8"` builds its resident shard and its filter subsets as `Sq8Shard`, never
    asks for the prefilter image, and the other dtypes still build `DenseShard`."""
    made = []

    class _Shard:
        def __init__(self, *a, **kw):
            made.append((type(self).__name__, a, kw))

    class _Sq8(_Shard):
        pass

    class _Dense(_Shard):
        pass

    monkeypatch.setattr(VS._lib, "load", lambda: None)
    monkeypatch.setattr(VS._lib, "require_gpu", lambda: None)
    monkeypatch.setattr(VS, "Sq8Shard", _Sq8)
    monkeypatch.setattr(VS, "DenseShard", _Dense)
    st = VS.GpuVectorStore(dense_dim=64, dense_dtype="int8", enable_sparse=False)
    assert st.dense_dtype == "int8" and st._use_prefilter() is False
    st._new_dense_shard(1500)
    assert made == [("_Sq8", (64, 1500, 0), {})]
    del made[:]
    VS.GpuVectorStore(dense_dim=64, dense_dtype="bf16", enable_sparse=False)._new_dense_shard(10)
    assert made[0][0] == "_Dense" and made[0][1][:3] == (64, 10, "bf16")


# ---------------------------------------------------------------------------------------------------------------- kernel resources
def _resources(src, *flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(ROOT, "verbatim-rag_amd", "csrc", src),
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage", *flags]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(?:[^:]+:\d+:\d+:\s+)?(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            rows.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sq8_kernels_use_no_scratch_and_spill_nothing():
    rows = [r for r in _resources("sq8.hip") if "sq8_" in r["name"]]
    for kernel in ("sq8_quantize_kernel", "sq8_query_kernel", "sq8_scan_kernel", "sq8_tile_kernel"):
        assert sum(kernel in r["name"] for r in rows) == 1, kernel
    assert len(rows) == 4
    for r in rows:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
