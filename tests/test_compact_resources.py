"""Register / scratch budget of the kernels of csrc/compact.hip, checked at build time without a GPU (the compiler's
resource-usage remarks, as tests/test_kernel_resources.py reads them for the other sources; tools/kernel_resources.py prints the
same table): the row-list kernels and every instantiation of the row mover keep everything in registers."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "verbatim-rag_amd", "csrc", "compact.hip")
KERNELS = {"filter_count_kernel": 1, "filter_scan_kernel": 1, "filter_emit_kernel": 1, "compact_move_kernel": 4}   # 16-, 8-, 4-, 1-byte pieces


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_compaction_kernels_use_no_scratch():
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
        assert int(occ) >= 4, (name, occ)
