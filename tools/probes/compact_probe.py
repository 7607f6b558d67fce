#!/usr/bin/env python3
"""What `GpuVectorStore.compact()` costs beside the two ways there were to drop deleted rows -> profiles/compact_probe.txt.

One dense-only store of `--rows` x `--dim` fp32 rows with the bf16 prefilter image (1.25 M x 768 by default), a random 10 % or
50 % of its rows deleted.  Per case and repetition a fresh store is built, flushed and its rows deleted; then, host clock, the
device work synchronised inside each call:
  compact          `store.compact()` in all, and of it the device part (`DenseShard.compact`: bitmap upload, row list, the
                   bounce waves over the fp32 rows and the image)
  re-upload        a new dense shard of the same capacity filled from the compacted host copy -- what a capacity rebuild does
  save + load      `save` (drops the deleted rows), `load`, and the first flush of the loaded store
and for the 50 % case the time of a 32-query dense batch (`query_batch`, top_k 10) per query before and after the compaction.
Median of `--reps` (>= 5) after one warm-up repetition, with min and max, one process.

usage: python tools/probes/compact_probe.py [--rows 1250000] [--dim 768] [--reps 5] [--out FILE]"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    return f"{statistics.median(ms):>10.1f} {min(ms):>10.1f} {max(ms):>10.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1250000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_probe.txt"))
    args = ap.parse_args()
    assert args.reps >= 5

    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd import vector_stores as vs

    n, dim = args.rows, args.dim
    rng = np.random.default_rng(0)
    X = rng.standard_normal((n, dim), dtype=np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((32, dim), dtype=np.float32)
    ids = [f"r{i}" for i in range(n)]
    empty, no_meta = [""] * n, [{}] * n
    tmp = tempfile.mkdtemp(prefix="compact_probe_")

    def build(p):
        st = vs.GpuVectorStore(dense_dim=dim, sparse_vocab=None, enable_sparse=False, dense_prefilter=True)
        st.add_vectors(ids, X, None, empty, empty, no_meta)
        st.query_batch(dense_queries=Q[:1], top_k=1, search_type="dense")          # flush: the rows are resident
        gone = np.nonzero(np.random.default_rng(1).random(n) < p)[0]
        st.delete([ids[i] for i in gone])
        return st, len(gone)

    def batch_ms(st):
        st.query_batch(dense_queries=Q, top_k=10, search_type="dense")             # warm-up (masks, scratch)
        return statistics.median(clock(lambda: st.query_batch(dense_queries=Q, top_k=10, search_type="dense"))[0] for _ in range(args.reps)) / 32

    lines = [f"compact_probe: {n} x {dim} fp32 rows + bf16 prefilter image, dense only; ms, median / min / max of {args.reps} "
             f"after one warm-up repetition",
             f"{'case':<10} {'what':<28} {'median':>10} {'min':>10} {'max':>10}"]
    for p in (0.10, 0.50):
        total, device, upload, saveload, before, after = [], [], [], [], [], []
        for rep in range(args.reps + 1):
            st, dead = build(p)
            if p == 0.50:
                before.append(batch_ms(st))
            path = os.path.join(tmp, f"s{rep}")
            t_save = clock(lambda: st.save(path))[0]
            loaded = []
            t_load = clock(lambda: loaded.append(vs.GpuVectorStore.load(path)) or
                           loaded[0].query_batch(dense_queries=Q[:1], top_k=1, search_type="dense"))[0]
            loaded[0].close()
            shutil.rmtree(path, ignore_errors=True)
            shard, dev = st._dense, []
            real = shard.compact
            shard.compact = lambda keep: dev.append(clock(lambda: real(keep))) or dev[-1][1]
            t_all, reclaimed = clock(st.compact)
            del shard.compact
            assert reclaimed == dead and len(st) == n - dead
            t_up = clock(lambda: st._new_dense_shard(st._dense_cap).add(st._dense_rows.data))[0]
            if p == 0.50:
                after.append(batch_ms(st))
            st.close()
            if rep:                                                                    # repetition 0 is the warm-up
                total.append(t_all), device.append(dev[0][0]), upload.append(t_up), saveload.append(t_save + t_load)
        case = f"{int(p * 100)} % dead"
        lines += [f"{case:<10} {'compact(), total':<28} {spread(total)}",
                  f"{case:<10} {'  of it DenseShard.compact':<28} {spread(device)}",
                  f"{case:<10} {'re-upload of the kept rows':<28} {spread(upload)}",
                  f"{case:<10} {'save + load + flush':<28} {spread(saveload)}"]
        if p == 0.50:
            lines += [f"{case:<10} {'32-query batch / query, before':<28} {spread(before[1:])}",
                      f"{case:<10} {'32-query batch / query, after':<28} {spread(after[1:])}"]
    shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
