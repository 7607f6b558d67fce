#!/usr/bin/env python3
"""SQ8 dense rows (Sq8Shard) against the bf16 and fp32 FLAT search of the same rows, on the MI355X -> profiles/sq8_probe.txt.

Corpus: tools/probes/ivf_probe.py's -- 1.25 M x 768 fp32 rows, a unit-normalised mixture of Gaussians (16 384 unit centres, noise
of norm ~0.6, seed fixed); queries are fresh draws from the same mixture.  Three shards of the same rows in one session: int8
(Sq8Shard), bf16 and fp32 + bf16 prefilter image (DenseShard, the store's default).  For nq in {1, 4, 32, 64, 256}, k = 10: ms
per call (host clock around the synchronous call, median of 21 after 3 warm-up calls) on the int8 shard under the scan kernel,
the tile kernel and the automatic route, and on the two FLAT shards.  Then recall@1 and @10 of the int8 lists (and, beside them,
of the bf16 lists) against the exact fp32 lists over 1 000 queries.

usage: python tools/probes/sq8_probe.py [--rows N] [--dim D] [--centres C] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ivf_probe import median_ms, mixture  # noqa: E402


def recall(ids, exact, k):
    return float(np.mean([len(set(ids[i, :k]) & set(exact[i, :k])) / k for i in range(len(ids))]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq8_probe.txt"))
    args = ap.parse_args()
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.vector_stores import DenseShard, Sq8Shard

    n, dim, k = args.rows, args.dim, 10
    rng = np.random.default_rng(20240607)
    centres = rng.standard_normal((args.centres, dim)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    X = mixture(rng, n, dim, centres, 0.6)
    Q = mixture(rng, 1000, dim, centres, 0.6)
    print(f"corpus ready: {X.shape}", flush=True)
    _lib.require_gpu()          # a measurement without a device fails; it does not fall back
    lines = [f"# tools/probes/sq8_probe.py: {n} x {dim} rows, {args.centres}-centre unit mixture, k {k}; one session, three shards of the same rows",
             f"# HBM per row: int8 {(dim + 15) // 16 * 16 + 4} B, bf16 {2 * dim} B, f32 + prefilter image {6 * dim} B",
             "# ms = median of 21 synchronous calls after 3 warm-up calls (min .. max); route 1 = scan kernel (4 queries per pass over",
             "# the shard), route 2 = tile kernel (64 query columns per pass), auto = scan up to SQ8_SCAN_MAX_Q = 4 queries, tile above"]
    shards = {}
    try:
        shards["int8"] = Sq8Shard(dim, n)
        shards["bf16"] = DenseShard(dim, n, "bf16")
        shards["f32"] = DenseShard(dim, n, "f32", prefilter=True)
        for sh in shards.values():
            sh.add(X)
        sq8 = shards["int8"]
        cell = lambda t: f"{t[0]:>8.3f} {f'({t[1]:.3f} .. {t[2]:.3f})':>19}"      # noqa: E731
        lines.append(f"{'nq':>4} {'int8 scan':>28} {'int8 tile':>28} {'int8 auto':>28} {'bf16 FLAT':>28} {'f32 FLAT':>28}")
        for nq in (1, 4, 32, 64, 256):
            q = np.ascontiguousarray(Q[:nq])
            row = f"{nq:>4}"
            lists = []
            for route in (1, 2, 0):
                sq8.set_route(route)
                lists.append(sq8.search(q, k))
                row += " " + cell(median_ms(lambda: sq8.search(q, k)))
            for a in lists[1:]:
                assert np.array_equal(a[1], lists[0][1]) and np.array_equal(a[0].view(np.uint32), lists[0][0].view(np.uint32)), "routes differ"
            for name in ("bf16", "f32"):
                sh = shards[name]
                row += " " + cell(median_ms(lambda: sh.search(q, k)))
            lines.append(row)
            print(row, flush=True)
        sq8.set_route(0)
        exact = shards["f32"].search(Q, k)[1]
        lines.append(f"recall against the exact fp32 lists, {len(Q)} queries:")
        for name in ("int8", "bf16"):
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
