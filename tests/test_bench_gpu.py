"""bench.py's two modes: a plain run is the headline alone (set-up, warm-up, timed steps, line); --full adds what takes runs of
its own.  Both print the same keys, so a reader of the line never has to know which mode wrote it."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("cpu_baseline", "parity_max_abs_err_vs_oracle", "ragged_leg", "topk_recall_vs_cpu_ref", "api_leg", "token_head_f16",
         "e2e_text_leg", "sharded_topk")


def _bench_line(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", *extra],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_and_full_bench_runs():
    plain = _bench_line()
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["higher_is_better"] is True
    assert abs(plain["value"] - 256 / (plain["ms_per_step"] * 1e-3)) < 1e-6 * plain["value"]
    assert plain["breakdown"] and plain["roofline"]["phase"].startswith("timed region")
    assert not any(k.startswith("isolated") or k.startswith("power_limited") for k in plain["roofline"])
    assert all(plain[k] is None for k in MOVED), {k: plain[k] for k in MOVED if plain[k] is not None}

    full = _bench_line("--full", "--cpu-budget", "0")       # the single-stream pass; the legs are the --cpu-budget share of --full
    assert set(full) == set(plain)
    assert full["roofline"]["isolated_pass"]["classes"] and full["roofline"]["isolated_frac"] > 0
