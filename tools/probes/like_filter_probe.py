#!/usr/bin/env python3
"""`title LIKE "%word%"` over many distinct titles: who should make the string leaf's table -> profiles/like_filter_probe.txt.

One store per case (dense only, dim 8: a mask needs no search) with `titles` distinct synthetic titles of 40-80 bytes and
`rows_per_title` rows each.  Every timed filter is one the store has not seen: a different word per repetition, so no table cache
and no mask cache answers.  Host clock around `store._mask(filter)` -- from the filter string to the finished mask, the device
work synchronised inside -- after one warm-up filter per mode, median of `--reps` (>= 5) with min and max, one process:
  host             filter_eval="host": one Python predicate call per row
  device/host      filter_eval="device", filter_strings="host": Python applies the pattern once per distinct title, the row
                   kernel does the rest
  device/device    filter_eval="device", filter_strings="device": the match kernel makes the table from the dictionary in HBM
The three masks of every word are compared bit for bit.  The modes are run-time choices, so one store takes them in turn; its
typed columns and the device dictionary are in place before anything is timed (their one-time costs are reported on their own).
Then, per dictionary, on a `RowFilter` of its own:
  upload           MetaColumn.string_bytes (UTF-8 encoding in Python) and RowFilter.append_strings (validation + copy), once
  match            RowFilter.match over the whole dictionary: launch + kernel + copy of the table to the host + synchronise, and
                   the same call over 64 codes (a launch that does next to nothing): the difference is the kernel's own time
  lone long string the same two calls on the dictionary plus ONE string of 1 MB (the pattern's word stands at its end): one lane
                   walks it alone while the rest of the device is idle

usage: python tools/probes/like_filter_probe.py [--cases 100000x1,100000x10,1000000x1,1000000x10] [--reps 5] [--no-dictionary]
       [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DIM = 8
WORDS = ("retrieval", "attention", "sparse", "dense", "ranking", "survey", "neural", "hybrid", "index", "search", "transformer",
         "evaluation", "benchmark", "language", "model", "graph", "vision", "speech", "robust", "efficient", "scaling", "memory",
         "kernel", "compiler", "quantised", "contrastive", "distilled", "multilingual", "biomedical", "legal", "financial", "open")
MODES = (("host", "host"), ("device", "host"), ("device", "device"))


def title(i):
    """40-80 bytes, distinct per i, a handful of WORDS in an order that depends on i."""
    t = f"{WORDS[i % 32]} {WORDS[(i // 32) % 32]} {WORDS[(i * 7 + 3) % 32]} for {WORDS[(i // 5) % 32]} #{i}"
    while len(t) < 40:
        t += " " + WORDS[(i * 11 + len(t)) % 32]
    return t


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    return f"{statistics.median(ms):>10.2f} {min(ms):>10.2f} {max(ms):>10.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="100000x1,100000x10,1000000x1,1000000x10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-dictionary", action="store_true", help="only the store's masks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "like_filter_probe.txt"))
    args = ap.parse_args()
    assert args.reps >= 5
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd.shards import RowFilter
    from verbatim_rag_amd.store_columns import MetaColumn
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    head = f"{'median':>10} {'min':>10} {'max':>10}"
    lines = [f"like_filter probe: ms, host clock around synchronous calls, one warm-up then {args.reps} repetitions, one process",
             "", f"_mask('title LIKE \"%word%\"'), a word per repetition that no cache has seen",
             f"{'titles':>9} {'rows':>9} {'eval/strings':>14} {head}"]
    print(lines[0], flush=True)
    rng = np.random.default_rng(3)
    dictionaries = {}
    for case in args.cases.split(","):
        n_titles, per = (int(x) for x in case.split("x"))
        titles = dictionaries.get(n_titles) or dictionaries.setdefault(n_titles, [title(i) for i in range(n_titles)])
        assert len(set(titles)) == n_titles and 40 <= min(map(len, titles)) and max(map(len, titles)) <= 80
        n = n_titles * per
        t0 = time.perf_counter()
        st = GpuVectorStore(dense_dim=DIM, enable_sparse=False, sparse_vocab=None, filter_eval="device", filter_strings="device")
        for a in range(0, n, 250_000):
            m = min(250_000, n - a)
            st.add_vectors([f"r{i}" for i in range(a, a + m)], rng.standard_normal((m, DIM)).astype(np.float32), None, [""] * m, [""] * m,
                           [{"title": titles[i % n_titles]} for i in range(a, a + m)])
        print(f"built the store of {n} rows in {time.perf_counter() - t0:.1f} s", flush=True)
        first = clock(lambda: st._mask('title LIKE "%warm-up%"'))[0]      # builds the column, uploads rows and dictionary
        print(f"{case}: first device/device mask (column build + uploads) {first:.1f} ms", flush=True)
        times = {mode: [] for mode in MODES}
        for rep in range(-1, args.reps):                                  # rep -1 warms every mode up
            word = WORDS[(rep + 7) % 32][: 4 + rep % 3]
            masks = []
            for mode in MODES:
                st.filter_eval, st.filter_strings = mode
                flt = f'title LIKE "%{word}%"' + " " * MODES.index(mode)    # one cache key per mode, the same program
                ms, mask = clock(lambda: st._mask(flt))
                masks.append(mask)
                if rep >= 0:
                    times[mode].append(ms)
            assert all(np.array_equal(masks[0], m) for m in masks[1:]) and masks[0].any() and not masks[0].all(), word
        for mode in MODES:
            lines.append(f"{n_titles:>9} {n:>9} {mode[0] + '/' + mode[1]:>14} {spread(times[mode])}")
            print(lines[-1], flush=True)
        st.close()
        del st

    lines += ["", "the dictionary alone (RowFilter): one-time upload, and match('like', '%word%') over it",
              f"{'titles':>9} {'what':>34} {head}"]
    for n_titles, titles in ({} if args.no_dictionary else dictionaries).items():
        for lone in (False, True):
            strings = titles + ["x" * (1_000_000 - 9) + " zzneedle"] if lone else titles
            col = MetaColumn("title")
            col.extend([{"title": s} for s in strings])
            rf = RowFilter()
            at = rf.add_column()
            enc, (data, off) = clock(lambda: col.string_bytes())
            up, _ = clock(lambda: rf.append_strings(at, data, off))
            tag = " + one 1 MB string" if lone else ""
            if not lone:
                lines.append(f"{n_titles:>9} {'string_bytes (Python encode)':>34} {enc:>10.2f}   once, {len(data)} bytes")
                lines.append(f"{n_titles:>9} {'append_strings (check + copy)':>34} {up:>10.2f}   once")
            whole, small = [], []
            for rep in range(-1, args.reps):
                word = "needle" if lone else WORDS[(rep + 11) % 32][:5]
                ms, got = clock(lambda: rf.match(at, "like", f"%{word}%"))
                ms64, _ = clock(lambda: rf.match(at, "like", f"%{word}%", 64))
                if rep >= 0:
                    whole.append(ms)
                    small.append(ms64)
                want = col.string_table("like", f"%{word}%")
                assert np.array_equal(got, want) and got.any(), word
            lines.append(f"{n_titles:>9} {'match, all codes' + tag:>34} {spread(whole)}")
            lines.append(f"{n_titles:>9} {'match, 64 codes' + tag:>34} {spread(small)}")
            print("\n".join(lines[-2:]), flush=True)
            rf.close()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
