#!/usr/bin/env python3
"""IVF_SQ8 (IvfOverlay over an Sq8Shard) against IVF_FLAT over bf16 rows with the same lists' parameters and against the FLAT SQ8
search, on the MI355X -> profiles/ivf_sq8_probe.txt.

Corpus: the one of tools/probes/ivf_probe.py and profiles/sq8_probe.txt -- 1.25 M x 768 rows, a unit-normalised mixture of Gaussians
(16 384 unit centres, noise of norm ~0.6 around them, seed fixed); queries are fresh draws from the same mixture.  nlist = 4096
(64 training rows per list, 10 Lloyd rounds) on both overlays.  For nprobe in {8, 64} and nq in {1, 32, 256}: ms per call (host clock
around the synchronous call; the three searches of a line are called in turn, 3 warm-up rounds, then the median of 21 rounds),
recall@10 of IVF_SQ8 against the FLAT SQ8 result, mean scanned fraction; largest list of both overlays; the register line of
ivf_sq8_scan_kernel (tools/kernel_resources.py) when hipcc is on the PATH.

usage: python tools/probes/ivf_sq8_probe.py [--rows N] [--dim D] [--nlist L] [--centres C] [--out FILE]"""
import argparse
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ivf_probe import mixture  # noqa: E402


def medians_ms(fns, reps=21, warm=3):
    """[(median, min, max)] of each of `fns`, called in turn round after round so that drift hits all of them alike."""
    ts = [[] for _ in fns]
    for r in range(warm + reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            if r >= warm:
                ts[i].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def register_line():
    if not (shutil.which("hipcc") and shutil.which("c++filt")):
        return "ivf_sq8_scan_kernel registers: hipcc not on the PATH here (python tools/kernel_resources.py verbatim-rag_amd/csrc/ivf_sq8.hip)"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "verbatim-rag_amd", "csrc", "ivf_sq8.hip")], capture_output=True, text=True).stdout.splitlines()
    return "\n".join(["# tools/kernel_resources.py verbatim-rag_amd/csrc/ivf_sq8.hip"] + ["# " + l[:100] for l in out if "vgpr" in l or "ivf_sq8_scan_kernel" in l])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_sq8_probe.txt"))
    args = ap.parse_args()
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.vector_stores import DenseShard, IvfOverlay, Sq8Shard

    n, dim, nlist, k = args.rows, args.dim, args.nlist, 10
    rng = np.random.default_rng(20240607)
    centres = rng.standard_normal((args.centres, dim)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    X = mixture(rng, n, dim, centres, 0.6)
    Q = mixture(rng, 256, dim, centres, 0.6)
    print(f"corpus ready: {X.shape}", flush=True)
    _lib.require_gpu()          # a measurement without a device fails; it does not fall back
    lines = [f"# tools/probes/ivf_sq8_probe.py: {n} x {dim} rows, {args.centres}-centre unit mixture, nlist {nlist}, k {k}; one session, two shards of the same rows",
             f"# HBM per row: int8 {((dim + 15) & ~15) + 4} B, bf16 {2 * dim} B; both overlays: 10 Lloyd rounds over {min(n, 64 * nlist)} rows",
             "# ms = median of 21 synchronous calls after 3 warm-up calls (min .. max), the three searches of a line called in turn;",
             "# ivf_sq8 = IvfOverlay over the Sq8Shard, ivf_bf16 = IvfOverlay over the bf16 DenseShard, flat_sq8 = Sq8Shard.search (automatic route)"]
    sq8, bf16 = Sq8Shard(dim, n), DenseShard(dim, n, "bf16")
    try:
        overlays = []
        for name, sh in (("ivf_sq8", sq8), ("ivf_bf16", bf16)):
            sh.add(X)
            ov = IvfOverlay(sh, nlist)
            t0 = time.perf_counter()
            ov.train(10, 64 * nlist)
            t1 = time.perf_counter()
            ov.sync()
            t2 = time.perf_counter()
            st = ov.stats()
            sh.ivf = ov
            overlays.append(ov)
            lines.append(f"{name}: train {(t1 - t0) * 1e3:.1f} ms   sync ({n} rows) {(t2 - t1) * 1e3:.1f} ms   largest_list {st['largest_list']} rows, mean {n / nlist:.0f}")
            print(lines[-1], flush=True)
        del X
        ov8, ov16 = overlays
        head = f"{'nq':>4} {'nprobe':>6}"
        for name in ("ivf_sq8", "ivf_bf16", "flat_sq8"):
            head += f" {name + ' ms':>11} {'(min .. max)':>19}"
        lines.append(head + f" {'scanned':>8} {'recall@10':>9}")
        for nq in (1, 32, 256):
            q = np.ascontiguousarray(Q[:nq])
            flat_ids = sq8.search(q, k)[1]
            for nprobe in (8, 64):
                _s, ids, seen = ov8.search(q, k, nprobe, scanned=True)
                recall = np.mean([len(set(ids[i]) & set(flat_ids[i])) / k for i in range(nq)])
                res = medians_ms([lambda: ov8.search(q, k, nprobe), lambda: ov16.search(q, k, nprobe), lambda: sq8.search(q, k)])
                line = f"{nq:>4} {nprobe:>6}"
                for med, lo, hi in res:
                    line += f" {med:>11.3f} {f'({lo:.3f} .. {hi:.3f})':>19}"
                lines.append(line + f" {seen.mean() / n:>8.4f} {recall:>9.3f}")
                print(lines[-1], flush=True)
    finally:
        sq8.close()
        bf16.close()
    lines.append(register_line())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
