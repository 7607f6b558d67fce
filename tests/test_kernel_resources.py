"""Register / scratch budget of the hot kernels, checked at build time on the CPU box (hipcc cross-compiles gfx950).

Round 5 lesson: compiling a tuning probe out of the fused Wqkv + attention kernel changed nothing in its arithmetic and moved
650 VGPRs of its non-banded instantiations into scratch -- 0.3 -> 3.4 ms per launch, the headline at a third -- and every parity
test stayed green.  The compiler's resource-usage remarks (tools/kernel_resources.py) catch that without a GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


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
@pytest.mark.parametrize("flags", [(), ("-DVRAG_DEBUG_API",)], ids=["product", "harness"])
def test_fused_qkv_attention_kernel_keeps_everything_in_registers(flags):
    rows = [r for r in _resources("qkv_attn.hip", *flags) if "qkv_attn_kernel" in r["name"]]
    assert len(rows) == 8                                        # banded / global x fold / plain x bf16 / fp16
    for r in rows:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
        assert int(r["Occupancy [waves/SIMD]"]) >= 2, r


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_gemm_kernels_scratch_budget():
    """The throughput instantiations (256 x 256 tiles): the GeGLU, SPLADE and top-k epilogues spill nothing; the residual and
    Wqkv + RoPE epilogues keep a handful of loop-invariant values in scratch around the epilogue (reloaded once per tile, none
    inside the K loop: NEXT.md) -- bounded here so that a change that pushes the K loop's fragments out is noticed."""
    rows = [r for r in _resources("gemm_bf16.hip") if "gemm_bf16_kernel" in r["name"]]
    assert len(rows) >= 30
    worst = {}
    for r in rows:
        m = re.search(r"gemm_bf16_kernelILi(\d+)ELi(\d+)ELi(\d+)E", r["name"])
        epi, bm = int(m.group(1)), int(m.group(2))
        worst[(epi, bm)] = max(worst.get((epi, bm), 0), int(r["ScratchSize [bytes/lane]"]))
    for (epi, bm), scr in worst.items():
        limit = 96 if (epi in (3, 5) and bm == 256) else 0
        assert scr <= limit, (epi, bm, scr)


FULLTEXT_KERNELS = ("tok_count_kernel", "tok_emit_kernel", "scan_reduce_kernel", "scan_sums_kernel", "scan_down_kernel",
                    "radix_hist_kernel", "radix_scatter_kernel", "rle_flags_kernel", "rle_scatter_kernel", "rle_tf_kernel",
                    "expand_kernel", "live_sum_kernel", "kd_kernel", "df_kernel", "ft_lookup_kernel", "ft_score_kernel",
                    "ft_bound_kernel")   # the device-resident search exports through csrc/topk.hip's topk_export_keys_kernel


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_full_text_kernels_are_the_same_in_the_harness_build():
    """csrc/fulltext.hip is compiled a second time for the harness library, with its unit-test hook (-DVRAG_DEBUG_API): host code
    only.  Both builds hold the same 17 kernels with the same registers, LDS and scratch (none), so what the unit tests run is
    what the product runs."""
    prod, dbg = ({r["name"]: r for r in _resources("fulltext.hip", *flags)} for flags in ((), ("-DVRAG_DEBUG_API",)))
    assert sorted(prod) == sorted(dbg) and len(prod) == len(FULLTEXT_KERNELS)
    for k in FULLTEXT_KERNELS:
        assert sum(k in name for name in prod) == 1, k
    for name, r in prod.items():
        assert r == dbg[name], name
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
