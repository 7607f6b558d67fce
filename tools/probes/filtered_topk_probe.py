"""filter_route="subset" against "bitmap" on one store (the route is switched between runs: same rows, same build): the first
filtered query after a mutation (cold: the subset route builds its second shard from the host copies, the bitmap route
compacts the bitmap) and the repeated query (warm), for a 64-row document filter, a 1 % filter and an unfiltered query whose
best row was just deleted.  Times are host wall clock around `query_batch` (it ends in a device synchronise), in ms.
usage: python tools/probes/filtered_topk_probe.py [--legs f32,bf16,sparse] [--rows 1250000] [--docs 1000000] [--out FILE]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd.vector_stores import GpuVectorStore

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="f32,bf16,sparse")
ap.add_argument("--rows", type=int, default=1_250_000)
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--out", default="")
args = ap.parse_args()
K, CHUNK, VOCAB, WARM = 10, 125_000, 30522, 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ingest(st, n, dense):
    rng = np.random.default_rng(1)
    for a in range(0, n, CHUNK):
        b = min(n, a + CHUNK)
        ids = [f"id{i}" for i in range(a, b)]
        metas = [{"document_id": f"d{i // 64}", "bucket": i % 100} for i in range(a, b)]
        if dense:
            st.add_vectors(ids, rng.standard_normal((b - a, args.dim), dtype=np.float32), None, [""] * (b - a), [""] * (b - a), metas)
        else:
            lens = rng.integers(32, 97, b - a)
            ptr = np.zeros(b - a + 1, np.int64)
            np.cumsum(lens, out=ptr[1:])
            # term j of a document = (start + j * step) mod VOCAB: distinct inside the document (96 * 300 < VOCAB)
            j = np.arange(int(ptr[-1]), dtype=np.int64) - np.repeat(ptr[:-1], lens)
            idx = ((np.repeat(rng.integers(0, VOCAB, b - a), lens) + j * np.repeat(rng.integers(1, 301, b - a), lens)) % VOCAB).astype(np.int32)
            st.add_vectors(ids, None, (ptr, idx, rng.random(int(ptr[-1]), dtype=np.float32)), [""] * (b - a), [""] * (b - a), metas)


def timed(st, kw):
    t0 = time.perf_counter()
    st.query_batch(**kw)
    cold = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for _ in range(WARM):
        st.query_batch(**kw)
    return cold, (time.perf_counter() - t0) / WARM * 1e3


def leg(name):
    dense = name != "sparse"
    n = args.rows if dense else args.docs
    st = GpuVectorStore(dense_dim=args.dim, sparse_vocab=VOCAB, enable_dense=dense, enable_sparse=not dense,
                        dense_dtype=name if dense else "f32")
    t0 = time.perf_counter()
    ingest(st, n, dense)
    rng = np.random.default_rng(2)
    if dense:
        queries = rng.standard_normal((32, args.dim), dtype=np.float32)
        kw = lambda nq: dict(dense_queries=list(queries[:nq]), search_type="dense", top_k=K)
    else:
        queries = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 24, replace=False), rng.random(24) + 0.1)} for _ in range(32)]
        kw = lambda nq: dict(sparse_queries=queries[:nq], search_type="sparse", top_k=K)
    st.query_batch(**kw(32))                                       # flush to HBM, warm the unfiltered routes
    say(f"# {name}: {n} rows ingested and flushed in {time.perf_counter() - t0:.1f} s")
    victim = n - 1                                                 # an unrelated row to delete: drops masks and subset shards
    for scenario, flt in (("64 rows pass", f'metadata["document_id"] == "d{n // 128}"'), ("1 % pass", 'metadata["bucket"] == 7'),
                          ("top row deleted", None)):
        for nq in (1, 32):
            row = {}
            for route in ("subset", "bitmap"):
                st._filter_route = route
                if flt is None:       # delete the current best row of query 0, then ask again
                    best = st.query_batch(**kw(1))[0][0].id
                    st.delete([best])
                else:
                    st.delete([f"id{victim}"])
                    victim -= 1
                row[route] = timed(st, dict(filter=flt, **kw(nq)))
            (cs, ws), (cb, wb) = row["subset"], row["bitmap"]
            say(f"{name:7s} {scenario:16s} nq={nq:<3d} cold subset {cs:10.2f}  bitmap {cb:10.2f}   warm subset {ws:8.2f}  bitmap {wb:8.2f}"
                f"   {'ok' if cb <= cs else 'BITMAP SLOWER COLD'}")
    st.close()


say(f"# filtered_topk_probe: rows={args.rows} dim={args.dim} docs={args.docs} vocab={VOCAB} top_k={K}; ms per query_batch call; "
    f"cold = first call after a delete, warm = mean of the next {WARM}")
for name in args.legs.split(","):
    leg(name)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
