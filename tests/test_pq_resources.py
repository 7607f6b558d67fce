"""Register / scratch budget of csrc/pq.hip, checked at build time without a GPU (the compiler's resource-usage remarks, as
tests/test_grouped_resources.py reads them; tools/kernel_resources.py prints the same table), with the product's flags and with the
harness build's -DVRAG_DEBUG_API: every pq_* kernel uses no scratch memory and spills nothing, the scan kernel stays under the 128
registers that its 1024-thread workgroups (4 waves per SIMD) allow, and the file adds exactly these five kernels."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "verbatim-rag_amd", "csrc", "pq.hip")
KERNELS = ("pq_half_kernel", "pq_encode_kernel", "pq_mean_kernel", "pq_lut_kernel", "pq_scan_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("flags", [(), ("-DVRAG_DEBUG_API",)], ids=["product", "harness"])
def test_pq_kernels_use_no_scratch_and_spill_nothing(flags):
    env = dict(os.environ, PATH=os.path.dirname(HIPCC) + os.pathsep + os.environ.get("PATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC, *flags], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stderr
    rows = [line.split(None, 6) for line in out.stdout.splitlines()[1:]]
    assert rows and all(len(r) == 7 for r in rows), out.stdout
    for kernel in KERNELS:
        assert sum(bool(re.search(rf"\b{kernel}\b", r[6])) for r in rows) == 1, (kernel, out.stdout)
    assert len(rows) == len(KERNELS), out.stdout
    for vgpr, agpr, _sgpr, spill, scratch, _occ, name in rows:
        assert int(spill) == 0 and int(scratch) == 0, (name, spill, scratch)
        assert int(vgpr) <= 128 and int(agpr) == 0, (name, vgpr, agpr)


def test_the_pq_kernels_are_built_into_both_libraries():
    text = open(os.path.join(ROOT, "verbatim-rag_amd", "build.py")).read()
    sources = re.search(r"^SOURCES = \[(.*)\]$", text, re.M).group(1)
    assert '"pq.hip"' in sources and os.path.exists(SRC)          # the harness library links every product object it does not recompile
    assert '"pq.hip"' not in re.search(r"^DEBUG_RECOMPILED = \[(.*)\]$", text, re.M).group(1)
