#!/usr/bin/env python3
"""IVF_FLAT overlay against the FLAT search of the same build, on the MI355X -> profiles/ivf_probe.txt.

Corpus: 1.25 M x 768 fp32 rows, a unit-normalised mixture of Gaussians (16 384 unit centres -- four per list, so lists hold several
clusters and come out balanced --, noise of norm ~0.6 around them, seed fixed); queries are fresh draws from the same mixture.  nlist = 4096 (64 training rows per list, 10 Lloyd rounds).  For nprobe in
{8, 32, 128, nlist} and nq in {1, 32, 256}: ms per call (host clock around the synchronous call, median of 21 after 3 warm-up calls),
mean scanned fraction, recall@10 against the FLAT result; training and sync time once.  FLAT = DenseShard.search on the same shard
(fp32 rows + bf16 prefilter image, the store's default), timed the same way next to every line.

usage: python tools/probes/ivf_probe.py [--rows N] [--dim D] [--nlist L] [--centres C] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def mixture(rng, n, dim, centres, spread):
    out = np.empty((n, dim), np.float32)
    for a in range(0, n, 65536):
        b = min(n, a + 65536)
        x = centres[rng.integers(0, len(centres), b - a)] + rng.standard_normal((b - a, dim), dtype=np.float32) * np.float32(spread / np.sqrt(dim))
        out[a:b] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return out


def median_ms(fn, reps=21, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_probe.txt"))
    args = ap.parse_args()
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.vector_stores import DenseShard, IvfOverlay

    n, dim, nlist, k = args.rows, args.dim, args.nlist, 10
    rng = np.random.default_rng(20240607)
    centres = rng.standard_normal((args.centres, dim)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    X = mixture(rng, n, dim, centres, 0.6)
    Q = mixture(rng, 256, dim, centres, 0.6)
    print(f"corpus ready: {X.shape}", flush=True)
    _lib.require_gpu()          # a measurement without a device fails; it does not fall back
    lines = [f"# tools/probes/ivf_probe.py: {n} x {dim} fp32 rows (+ bf16 prefilter image), {args.centres}-centre unit mixture, nlist {nlist}, k {k}",
             "# ms = median of 21 synchronous calls after 3 warm-up calls (min .. max); FLAT = DenseShard.search on the same shard"]
    sh = DenseShard(dim, n, "f32", prefilter=True)
    try:
        sh.add(X)
        ov = IvfOverlay(sh, nlist)
        t0 = time.perf_counter()
        ov.train(10, 64 * nlist)
        t1 = time.perf_counter()
        ov.sync()
        t2 = time.perf_counter()
        st = ov.stats()
        lines.append(f"train (10 rounds, {min(n, 64 * nlist)} rows): {(t1 - t0) * 1e3:.1f} ms   sync ({n} rows): {(t2 - t1) * 1e3:.1f} ms   "
                     f"largest list {st['largest_list']} rows, mean {n / nlist:.0f}")
        lines.append(f"{'nq':>4} {'nprobe':>6} {'ivf ms':>9} {'(min .. max)':>19} {'flat ms':>9} {'(min .. max)':>19} {'scanned':>8} {'recall@10':>9}")
        for nq in (1, 32, 256):
            q = np.ascontiguousarray(Q[:nq])
            flat_ids = sh.search(q, k)[1]
            f_med, f_lo, f_hi = median_ms(lambda: sh.search(q, k))
            for nprobe in (8, 32, 128, nlist):
                _s, ids, seen = ov.search(q, k, nprobe, scanned=True)
                recall = np.mean([len(set(ids[i]) & set(flat_ids[i])) / k for i in range(nq)])
                med, lo, hi = median_ms(lambda: ov.search(q, k, nprobe))
                lines.append(f"{nq:>4} {nprobe:>6} {med:>9.3f} {f'({lo:.3f} .. {hi:.3f})':>19} {f_med:>9.3f} {f'({f_lo:.3f} .. {f_hi:.3f})':>19} "
                             f"{seen.mean() / n:>8.4f} {recall:>9.3f}")
                print(lines[-1], flush=True)
    finally:
        sh.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
