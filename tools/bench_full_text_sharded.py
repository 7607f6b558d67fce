"""Wall time of full-text queries on a row-sharded GpuVectorStore: world N over gloo with every rank on GPU 0, beside the
single-rank store on the same corpus.  For information only: ranks that share one GPU and exchange through host memory say
nothing about RCCL over xGMI -- the figure shows what the two statistics sums, the list all-gather and the payload gather add on
the host side.  Prints one JSON line (rank 0).
usage: python tools/bench_full_text_sharded.py [--world 2] [--rows 100000] [--words 300] [--reps 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(store, queries_of, nq, k, reps):
    batches = [queries_of(nq) for _ in range(reps + 1)]
    run = (lambda q: store.query(text_query=q[0], top_k=k, search_type="full_text")) if nq == 1 else \
          (lambda q: store.query_batch(text_queries=q, top_k=k, search_type="full_text"))
    run(batches[0])
    times = []
    for q in batches[1:]:
        t = time.perf_counter()
        run(q)
        times.append(time.perf_counter() - t)
    return round(float(np.median(times)) * 1e3, 3)


def _worker(rank, world, port, a, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    try:
        import torch.distributed as dist

        import verbatim_rag_amd  # noqa: F401
        from tools.bench_full_text import corpus
        from verbatim_rag_amd import vector_stores as vs
        from verbatim_rag_amd.distributed import ShardComm

        dist.init_process_group("gloo", rank=rank, world_size=world)
        texts, words = corpus(a.rows, a.words, vocab=50000, seed=11)
        n = len(texts)
        res = {"world": world, "backend": "gloo", "ranks_share_one_gpu": True, "rows": n, "mean_words": a.words}
        for name, comm in (("single", None), ("sharded", ShardComm(device=0))):
            st = vs.GpuVectorStore(dense_dim=None, enable_dense=False, enable_sparse=False, enable_full_text=True, comm=comm)
            st.add_vectors([f"id{i}" for i in range(n)], None, None, texts, [""] * n, [{} for _ in range(n)])
            rng = np.random.default_rng(5)             # the same queries on every rank

            def queries_of(m):
                return [" ".join(words[int(j)] for j in rng.zipf(1.3, size=int(rng.integers(2, 6))) if j < len(words)) or words[1]
                        for _ in range(m)]

            for nq in (1, 256):
                res[f"{name}_q{nq}_k10_ms"] = _timed(st, queries_of, nq, 10, a.reps)
            st.close()
        q.put((rank, res))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:
        import traceback

        q.put((rank, f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"))


def main():
    import torch.multiprocessing as mp

    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--words", type=int, default=300)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 41500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, a.world, port, a, q)) for r in range(a.world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=1200) for _ in procs), key=lambda x: x[0])
    for p in procs:
        p.join(60)
    bad = [r for r in res if not isinstance(r[1], dict)]
    if bad:
        raise SystemExit(str(bad))
    line = json.dumps(res[0][1])
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
