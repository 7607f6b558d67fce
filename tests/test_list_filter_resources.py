"""Register / scratch budget of csrc/listfilter.hip, checked at build time without a GPU (the compiler's resource-usage remarks,
as tests/test_compact_resources.py reads them; tools/kernel_resources.py prints the same table): the list kernel walks a row's
elements with a bounded loop and keeps the evaluation stack in one register, so it has no scratch and spills nothing -- and the
file adds exactly one kernel; csrc/rowfilter.hip keeps its one (tests/test_filter_program_host.py)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "verbatim-rag_amd", "csrc", "listfilter.hip")
KERNELS = {"list_filter_eval_kernel": 1}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_list_kernel_uses_no_scratch():
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
        assert int(occ) == 8 and int(vgpr) <= 32, (name, vgpr, occ)      # DESIGN.md section 3 records 20 VGPRs


def test_the_list_kernel_is_built_into_the_library():
    spec_path = os.path.join(ROOT, "verbatim-rag_amd", "build.py")
    text = open(spec_path).read()
    assert '"listfilter.hip"' in text and os.path.exists(SRC)
