#!/usr/bin/env python3
"""Row masks of compound filters: `GpuVectorStore(filter_eval="host")` against `filter_eval="device"` -> profiles/filter_eval_probe.txt.

Stores of 10^6 and 10^7 rows (dense only, dim 8: a mask needs no search) with synthetic metadata -- `year` an int in 1990 .. 2029
(missing in a tenth of the rows), `source` one of five strings, `peer` a bool (missing in a fifth).  Per filter and route, host
clock around `store._mask(filter)`:
  first      the first mask of that filter on a store that has answered no filter yet (device: builds the columns of the keys it
             names -- one Python pass per key --, uploads them, runs the kernel)
  again      another filter string over the same keys (device: columns in place, the kernel and the copies only; host: the same
             Python pass as `first`)
  insert     the mask after one insert of 1 000 rows, which empties the mask cache (device: the columns grow by the new rows,
             1 000 rows per key are uploaded), median of `--reps` inserts
Both routes' masks are compared bit for bit on the way.

usage: python tools/probes/filter_eval_probe.py [--rows 1000000,10000000] [--reps 3] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FILTERS = ("year >= 2020", 'year >= 2010 and source != "web"', "(year < 2000 or year > 2025) and not peer == true")
SOURCES = ("web", "journal", "arXiv", "book", "report")
DIM = 8


def metadata(first, n):
    out = []
    for i in range(first, first + n):
        md = {"source": SOURCES[(i * 7) % 5]}
        if i % 10:
            md["year"] = 1990 + (i * 13) % 40
        if i % 5:
            md["peer"] = (i * 3) % 7 < 3
        out.append(md)
    return out


def insert(store, first, n, rng):
    slab = 250_000
    for a in range(first, first + n, slab):
        m = min(slab, first + n - a)
        store.add_vectors([f"r{i}" for i in range(a, a + m)], rng.standard_normal((m, DIM)).astype(np.float32), None, [""] * m, [""] * m,
                          metadata(a, m))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_eval_probe.txt"))
    args = ap.parse_args()
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    lines = [f"filter_eval probe: _mask(filter) in ms, host clock, one run; insert = median of {args.reps} inserts of 1 000 rows",
             f"{'rows':>9} {'route':>7} {'first':>10} {'again':>10} {'insert':>10}  filter"]
    print(lines[0], flush=True)
    for n in (int(x) for x in args.rows.split(",")):
        rng = np.random.default_rng(5)
        stores = {}
        for route in ("host", "device"):
            t0 = time.perf_counter()
            stores[route] = GpuVectorStore(dense_dim=DIM, enable_sparse=False, sparse_vocab=None, filter_eval=route)
            insert(stores[route], 0, n, rng)
            print(f"built the {route} store of {n} rows in {time.perf_counter() - t0:.1f} s", flush=True)
        rows = {route: [] for route in stores}
        for fi, flt in enumerate(FILTERS):
            twin = flt + " "                                  # another cache key, the same program
            first, again = {}, {}
            for route, st in stores.items():
                if route == "device":                        # every filter starts from a store without columns
                    st._metadata.columns.clear()
                    st._metadata.row_filter, st._metadata.row_filter_cols = None, {}
                st._drop_subsets()
                first[route] = clock(lambda: st._mask(flt))
                again[route] = clock(lambda: st._mask(twin))
                print(f"{n} {route} {flt!r}: first {first[route][0]:.1f} ms, again {again[route][0]:.1f} ms", flush=True)
            assert np.array_equal(first["host"][1], first["device"][1]) and np.array_equal(again["host"][1], again["device"][1]), flt
            rows["host"].append([first["host"][0], again["host"][0], []])
            rows["device"].append([first["device"][0], again["device"][0], []])
        for flt in FILTERS:                                   # every column in place before the inserts
            stores["device"]._mask(flt)
        at = n
        for rep in range(args.reps):
            for st in stores.values():
                insert(st, at, 1000, rng)
            at += 1000
            for fi, flt in enumerate(FILTERS):
                got = {route: clock(lambda: st._mask(flt)) for route, st in stores.items()}
                assert np.array_equal(got["host"][1], got["device"][1]), flt
                for route in stores:
                    rows[route][fi][2].append(got[route][0])
            print(f"{n}: insert {rep + 1} of {args.reps} done", flush=True)
        for fi, flt in enumerate(FILTERS):
            for route in ("host", "device"):
                f, a, ins = rows[route][fi]
                lines.append(f"{n:>9} {route:>7} {f:>10.1f} {a:>10.1f} {statistics.median(ins):>10.1f}  {flt}")
        for st in stores.values():
            st.close()
        stores.clear()
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
