#!/usr/bin/env python3
"""PQ dense rows (PqShard, m = 96) against the SQ8, bf16 and fp32 FLAT search of the same rows, on the MI355X -> profiles/pq_probe.txt.

Corpus: tools/probes/ivf_probe.py's -- 1.25 M x 768 fp32 rows, a unit-normalised mixture of Gaussians (16 384 unit centres, noise
of norm ~0.6, seed fixed); queries are fresh draws from the same mixture.  Four shards of the same rows in one session: PQ
(PqShard, codebooks trained as the store trains them: 65 536 evenly strided rows, 10 Lloyd rounds), int8 (Sq8Shard), bf16 and
fp32 + bf16 prefilter image (DenseShard, the store's default).  For nq in {1, 4, 32, 256}, k = 10: ms per call (host clock around
the synchronous call, median of 21 after 3 warm-up calls), the four shards called in turn.  Then recall@1 and @10 of the PQ lists
(and, beside them, of the int8 and bf16 lists) against the exact fp32 lists over 1 000 queries, the training time, the add rate
and the HBM per row.

Kernel level: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/probes/pq_probe.py --only-pq` (tools/rocpd_summary.py) and,
in a run of its own, `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d DIR -- python ... --only-pq` (tools/pmc_summary.py);
both summaries are appended to profiles/pq_probe.txt by hand.

usage: python tools/probes/pq_probe.py [--rows N] [--dim D] [--m M] [--centres C] [--out FILE] [--only-pq]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ivf_probe import median_ms, mixture  # noqa: E402
from sq8_probe import recall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pq_probe.txt"))
    ap.add_argument("--only-pq", action="store_true", help="train, add and search the PQ shard only and write no file (for rocprofv3 runs)")
    args = ap.parse_args()
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.vector_stores import PQ_TRAIN_ITERS, PQ_TRAIN_ROWS_MAX, DenseShard, PqShard, Sq8Shard

    n, dim, m, k = args.rows, args.dim, args.m, 10
    rng = np.random.default_rng(20240607)
    centres = rng.standard_normal((args.centres, dim)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    X = mixture(rng, n, dim, centres, 0.6)
    Q = mixture(rng, 1000, dim, centres, 0.6)
    print(f"corpus ready: {X.shape}", flush=True)
    _lib.require_gpu()          # a measurement without a device fails; it does not fall back
    stride = (m + 15) // 16 * 16
    lines = [f"# tools/probes/pq_probe.py: {n} x {dim} rows, {args.centres}-centre unit mixture, m {m}, k {k}; one session, four shards of the same rows",
             f"# HBM per row: pq {stride} B (+ {dim * 1024} B of codebooks per shard), int8 {(dim + 15) // 16 * 16 + 4} B, bf16 {2 * dim} B, "
             f"f32 + prefilter image {6 * dim} B",
             "# ms = median of 21 synchronous calls after 3 warm-up calls (min .. max), the four shards called in turn per nq"]
    shards = {}
    try:
        pq = shards["pq"] = PqShard(dim, m, n)
        take = min(n, PQ_TRAIN_ROWS_MAX)
        sample = np.ascontiguousarray(X[(np.arange(take, dtype=np.int64) * n) // take])
        t0 = time.perf_counter()
        pq.train(sample, PQ_TRAIN_ITERS)
        t_train = time.perf_counter() - t0
        t0 = time.perf_counter()
        pq.add(X)
        t_add = time.perf_counter() - t0
        lines.append(f"# training: {take} rows, {PQ_TRAIN_ITERS} Lloyd rounds, {t_train:.2f} s (host clock, upload included); "
                     f"add: {n} host rows in {t_add:.2f} s = {n / t_add / 1e6:.2f} M rows/s (upload and encoding)")
        print(lines[-1], flush=True)
        if args.only_pq:            # the run under the profiler: the PQ kernels alone, a few calls per batch size
            for nq in (1, 4, 32, 256):
                q = np.ascontiguousarray(Q[:nq])
                print(nq, median_ms(lambda: pq.search(q, k), reps=5, warm=1), flush=True)
            return
        shards["int8"] = Sq8Shard(dim, n)
        shards["bf16"] = DenseShard(dim, n, "bf16")
        shards["f32"] = DenseShard(dim, n, "f32", prefilter=True)
        for name in ("int8", "bf16", "f32"):
            shards[name].add(X)
        cell = lambda t: f"{t[0]:>8.3f} {f'({t[1]:.3f} .. {t[2]:.3f})':>19}"      # noqa: E731
        lines.append(f"{'nq':>4} {'pq FLAT':>28} {'int8 FLAT':>28} {'bf16 FLAT':>28} {'f32 FLAT':>28}")
        for nq in (1, 4, 32, 256):
            q = np.ascontiguousarray(Q[:nq])
            row = f"{nq:>4}"
            for name in ("pq", "int8", "bf16", "f32"):
                sh = shards[name]
                row += " " + cell(median_ms(lambda: sh.search(q, k)))
            lines.append(row)
            print(row, flush=True)
        exact = shards["f32"].search(Q, k)[1]
        lines.append(f"recall against the exact fp32 lists, {len(Q)} queries:")
        for name in ("pq", "int8", "bf16"):
            ids = shards[name].search(Q, k)[1]
            lines.append(f"  {name}: recall@1 {recall(ids, exact, 1):.4f}   recall@10 {recall(ids, exact, 10):.4f}")
            print(lines[-1], flush=True)
    finally:
        for sh in shards.values():
            sh.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
