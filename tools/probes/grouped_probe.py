#!/usr/bin/env python3
"""Grouping search against the filtered and the plain search of the same build, on the MI355X -> profiles/grouped_search_probe.txt.

Corpus: the 1.25 M x 768 clustered synthetic rows of tools/probes/ivf_probe.py (a unit-normalised mixture of 16 384 Gaussians,
seed fixed), as an fp32 shard (with the bf16 prefilter image, the store's default) and as a bf16 shard; queries are fresh draws
from the same mixture.  Group layouts: groups of ~50 consecutive rows (documents of ~50 chunks), one single group, and every row
its own group.  For nq in {1, 32, 256}, top_k 10 and group_size in {1, 3}: ms per `DenseShard.search_grouped` call (host clock
around the synchronous call, median of 21 after 3 warm-up calls).  Next to it, in the same session on the same shard:
  filtered  `search_filtered(k = 10)` under an all-ones bitmap -- the same serial chains over the same rows, so the difference to the
            grouped call is what the reduction, the selection and the query slicing cost;
  plain     `search(k = 64)` -- what over-fetching would start from (the prefilter image / tiled routes: other kernels altogether).

usage: python tools/probes/grouped_probe.py [--rows N] [--dim D] [--centres C] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ivf_probe import median_ms, mixture  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--centres", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_search_probe.txt"))
    args = ap.parse_args()
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.shards import GroupColumn, _bitmap
    from verbatim_rag_amd.vector_stores import DenseShard

    n, dim, k = args.rows, args.dim, 10
    rng = np.random.default_rng(20240607)
    centres = rng.standard_normal((args.centres, dim)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    X = mixture(rng, n, dim, centres, 0.6)
    Q = mixture(rng, 256, dim, centres, 0.6)
    print(f"corpus ready: {X.shape}", flush=True)
    _lib.require_gpu()          # a measurement without a device fails; it does not fall back
    layouts = {"~50 rows": (np.arange(n) // 50).astype(np.int32), "one group": np.zeros(n, np.int32),
               "all distinct": np.arange(n, dtype=np.int32)}
    ones = _bitmap(np.ones(n, bool))
    lines = [f"# tools/probes/grouped_probe.py: {n} x {dim} rows, {args.centres}-centre unit mixture, top_k {k}",
             "# ms = median of 21 synchronous calls after 3 warm-up calls (min .. max); filtered = search_filtered(k = 10) under an all-ones",
             "# bitmap (the same chains); plain = search(k = 64); same session, same shard"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    for dtype in ("f32", "bf16"):
        sh = DenseShard(dim, n, dtype, prefilter=True)
        cols = {}
        try:
            sh.add(X)
            for name, codes in layouts.items():
                cols[name] = GroupColumn()
                cols[name].append(codes)
            emit(f"## {dtype} rows" + (" (+ bf16 prefilter image)" if dtype == "f32" else ""))
            emit(f"{'nq':>4} {'layout':>13} {'size':>4} {'grouped ms':>10} {'(min .. max)':>21} {'filtered ms':>11} {'plain k=64 ms':>13}")
            for nq in (1, 32, 256):
                q = np.ascontiguousarray(Q[:nq])
                f_med, _lo, _hi = median_ms(lambda: sh.search_filtered(q, k, ones, n))
                p_med, _lo, _hi = median_ms(lambda: sh.search(q, 64))
                for name, col in cols.items():
                    for g in (1, 3):
                        med, lo, hi = median_ms(lambda: sh.search_grouped(q, k, g, col))
                        emit(f"{nq:>4} {name:>13} {g:>4} {med:>10.3f} {f'({lo:.3f} .. {hi:.3f})':>21} {f_med:>11.3f} {p_med:>13.3f}")
        finally:
            for col in cols.values():
                col.close()
            sh.close()


if __name__ == "__main__":
    main()
