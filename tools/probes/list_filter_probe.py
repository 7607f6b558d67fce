#!/usr/bin/env python3
"""`json_contains(metadata["authors"], "...")` from the filter string to the mask -> profiles/list_filter_probe.txt.

One store per case (dense only, dim 8: a mask needs no search) of `rows` rows, each with a list of 1-5 authors drawn from a pool
of `--authors` distinct names.  Every timed filter is one the store has not seen: a different author per repetition, so no mask
cache answers.  Host clock around `store._mask(filter)` -- the device work synchronised inside -- after one warm-up filter per
mode, median of `--reps` (>= 5) with min and max, one process:
  host             filter_eval="host": one Python predicate call per row, each walking the row's list
  device/host      filter_eval="device", filter_strings="host": Python applies `==` once per distinct author, the list kernel
                   walks the rows' elements
  device/device    filter_eval="device", filter_strings="device": the match kernel makes the table from the dictionary in HBM
The three masks of every author are compared bit for bit.  The modes are run-time choices, so one store takes them in turn; its
typed column, the list part and the device dictionary are in place before anything is timed (the first device mask, which pays
for them once, is reported on its own).  The comparison is the host route of the same commit: no earlier commit has the filter.

usage: python tools/probes/list_filter_probe.py [--cases 1000000,10000000] [--authors 50000] [--reps 5] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DIM = 8
MODES = (("host", "host"), ("device", "host"), ("device", "device"))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    return f"{statistics.median(ms):>10.2f} {min(ms):>10.2f} {max(ms):>10.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1000000,10000000")
    ap.add_argument("--authors", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_filter_probe.txt"))
    args = ap.parse_args()
    assert args.reps >= 5
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    names = [f"Author {i:06d} of the pool" for i in range(args.authors)]
    head = f"{'median':>10} {'min':>10} {'max':>10}"
    lines = [f"list_filter probe: ms, host clock around synchronous calls, one warm-up then {args.reps} repetitions, one process",
             "", "_mask('json_contains(metadata[\"authors\"], \"<author>\")'), an author per repetition that no cache has seen; 1-5 authors "
             f"per row from {args.authors} names",
             f"{'rows':>9} {'elements':>10} {'eval/strings':>14} {head}"]
    print(lines[0], flush=True)
    for case in args.cases.split(","):
        n = int(case)
        rng = np.random.default_rng(3)
        t0 = time.perf_counter()
        st = GpuVectorStore(dense_dim=DIM, enable_sparse=False, sparse_vocab=None, filter_eval="device", filter_strings="device")
        for a in range(0, n, 250_000):
            m = min(250_000, n - a)
            lens = rng.integers(1, 6, m)
            picks = rng.integers(0, args.authors, int(lens.sum())).tolist()
            ends = np.cumsum(lens).tolist()
            metas = [{"authors": [names[j] for j in picks[e - k:e]]} for e, k in zip(ends, lens.tolist())]
            st.add_vectors([f"r{i}" for i in range(a, a + m)], rng.standard_normal((m, DIM)).astype(np.float32), None, [""] * m, [""] * m, metas)
            del metas, picks
        print(f"built the store of {n} rows in {time.perf_counter() - t0:.1f} s", flush=True)
        first = clock(lambda: st._mask('json_contains(authors, "warm-up")'))[0]      # builds the column, uploads lists and dictionary
        elements = int(st._metadata.columns["authors"].elem_off[-1])
        lines.append(f"{n:>9} {elements:>10} {'first mask':>14} {first:>10.2f}   once: column build in Python + uploads")
        print(lines[-1], flush=True)
        times = {mode: [] for mode in MODES}
        for rep in range(-1, args.reps):                                  # rep -1 warms every mode up
            author = names[(rep + 2) * 7919 % args.authors]
            masks = []
            for mode in MODES:
                st.filter_eval, st.filter_strings = mode
                flt = f'json_contains(metadata["authors"], "{author}")' + " " * MODES.index(mode)   # one cache key per mode
                ms, mask = clock(lambda: st._mask(flt))
                masks.append(mask)
                if rep >= 0:
                    times[mode].append(ms)
            assert all(np.array_equal(masks[0], m) for m in masks[1:]) and masks[0].any() and not masks[0].all(), author
        for mode in MODES:
            lines.append(f"{n:>9} {elements:>10} {mode[0] + '/' + mode[1]:>14} {spread(times[mode])}")
            print(lines[-1], flush=True)
        st.close()
        del st
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
