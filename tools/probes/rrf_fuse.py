"""Host against device fusion of a hybrid batch: `rrf_merge_rows` (numpy, on this machine's CPU) and `rrf_fuse_rows_device`
(`vrag_rrf_fuse`, host form: its copies in and out and its synchronise are inside the time) on identical inputs in one session.
Random overlapping lists (rows drawn per method from a pool of 1.5 x the list length, 20 % holes, as in the tests); one warm-up call, then the
median of REPS calls each, host wall clock in ms.  Every shape is first checked for bit equality.
usage: python tools/probes/rrf_fuse.py [--reps 20] [--out FILE]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd.vector_stores import rrf_fuse_rows_device, rrf_merge_rows

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default="")
args = ap.parse_args()
METHODS = ("dense", "sparse", "full_text")
WEIGHTS = {"dense": 0.5, "sparse": 0.3, "full_text": 0.2}
#         queries, list length per method, top_k
SHAPES = [(1000, (20, 20, 20), 10), (10240, (20, 20), 10), (1024, (2048, 2048), 1024)] + [(q, (20, 20), 10) for q in (1, 4, 16, 64, 256)]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def lists_for(rng, nq, lens):
    out = {}
    for m, n in zip(METHODS, lens):
        pool = int(1.5 * n)
        rows = np.argsort(rng.random((nq, pool)), axis=1)[:, :n].astype(np.int64)      # per query: n of the pool, no repeats
        rows[rng.random((nq, n)) < 0.2] = -1
        out[m] = rows
    return out


def median_ms(fn, reps):
    fn()                                                                               # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


say(f"# rrf_fuse probe: ms per call, median of {args.reps} after one warm-up; host = rrf_merge_rows (numpy), "
    f"device = rrf_fuse_rows_device (copies and synchronise included)")
say(f"{'queries':>8} {'lists':>14} {'top_k':>6} {'host ms':>10} {'device ms':>10} {'host/device':>12}")
rng = np.random.default_rng(0)
for nq, lens, top_k in SHAPES:
    lists = lists_for(rng, nq, lens)
    want, got = rrf_merge_rows(lists, top_k, WEIGHTS), rrf_fuse_rows_device(lists, top_k, WEIGHTS)
    if not (np.array_equal(want[0], got[0]) and np.array_equal(want[1].view(np.uint64), got[1].view(np.uint64))):
        say(f"{nq:>8} {'+'.join(map(str, lens)):>14} {top_k:>6}  RESULTS DIFFER")
        sys.exit(1)
    reps = args.reps
    host = median_ms(lambda: rrf_merge_rows(lists, top_k, WEIGHTS), reps)
    dev = median_ms(lambda: rrf_fuse_rows_device(lists, top_k, WEIGHTS), reps)
    say(f"{nq:>8} {'+'.join(map(str, lens)):>14} {top_k:>6} {host:>10.3f} {dev:>10.3f} {host / dev:>12.1f}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
