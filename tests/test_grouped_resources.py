"""Register / scratch budget of csrc/grouped.hip, checked at build time without a GPU (the compiler's resource-usage remarks, as
tests/test_list_filter_resources.py reads them; tools/kernel_resources.py prints the same table): the scoring kernel (one
instantiation per row type), the selection -- whose 16 level-0 keys per thread must stay in registers -- and the gather use no
scratch memory and spill nothing, and the file adds exactly these four kernels."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "verbatim-rag_amd", "csrc", "grouped.hip")
KERNELS = {"grouped_score_kernel": 2, "grouped_select_kernel": 1, "grouped_gather_kernel": 1}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_grouped_kernels_use_no_scratch():
    env = dict(os.environ, PATH=os.path.dirname(HIPCC) + os.pathsep + os.environ.get("PATH", ""))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC], capture_output=True, text=True,
                         timeout=600, env=env)
    assert out.returncode == 0, out.stderr
    rows = [line.split(None, 6) for line in out.stdout.splitlines()[1:]]
    assert rows and all(len(r) == 7 for r in rows), out.stdout
    for kernel, count in KERNELS.items():
        mine = [r for r in rows if re.search(rf"\b{kernel}\b", r[6])]
        assert len(mine) == count, (kernel, out.stdout)
    assert len(rows) == sum(KERNELS.values()), out.stdout
    for vgpr, agpr, sgpr, spill, scratch, occ, name in rows:
        assert int(spill) == 0 and int(scratch) == 0, (name, spill, scratch)
        assert int(vgpr) <= 128 and int(agpr) == 0, (name, vgpr, agpr)      # DESIGN.md section 3 records 88 / 54 / 11 VGPRs


def test_the_grouped_kernels_are_built_into_the_library():
    text = open(os.path.join(ROOT, "verbatim-rag_amd", "build.py")).read()
    assert '"grouped.hip"' in text and os.path.exists(SRC)
