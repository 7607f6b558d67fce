"""BM25 full-text search on a row-sharded `GpuVectorStore`: every rank scores its rows with the
corpus-wide statistics -- `(N, sum dl)` and the batch's `df` vector summed over the ranks as exact integers
(`ShardComm.sum_int64`, `vrag_text_index_set_corpus_stats`) -- so ids and fp32 score bits equal the single-rank store's and the
host restatement's (tests/full_text_oracle.py), on every rank.

World 2 runs over gloo with both ranks on GPU 0 (host lists, device merge); the RCCL branch -- `vrag_text_index_search_device`
writing the lists into the exchange payload in HBM -- runs at world 1 over nccl, as tests/test_nccl_gpu.py does for the
other methods."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _gloo_worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    try:
        import torch.distributed as dist

        import verbatim_rag_amd  # noqa: F401
        from tests.full_text_sharded_cases import session
        from verbatim_rag_amd.distributed import ShardComm

        dist.init_process_group("gloo", rank=rank, world_size=world)
        own = os.path.join(tmp, f"rank{rank}")
        os.makedirs(own, exist_ok=True)
        single, single_checks, world1_dir = session(None, "sharded", own)          # one GPU holds everything
        out = {"single": (single, single_checks)}
        for payload in ("sharded", "replicated"):
            comm = ShardComm(device=0)
            got, checks, _dir = session(comm, payload, tmp, world1_dir=world1_dir)
            out[payload] = (got, checks)
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:
        import traceback

        q.put((rank, f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"))


def _assert_transcript(got, want, keys, label):
    for key in keys:
        ids, scores = got[key]
        w_ids, w_scores = want[key]
        assert np.array_equal(ids, w_ids), f"{label}: ids of {key!r} differ"
        assert np.array_equal(scores, w_scores), f"{label}: scores of {key!r} differ"


def test_sharded_full_text_world2_equals_single_rank_and_oracle(tmp_path):
    import torch.multiprocessing as mp

    from tests.full_text_sharded_cases import ORACLE_KEYS, oracle_session

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=900) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(60)
    oracle = oracle_session()
    for rank, out in res:
        assert isinstance(out, dict), out
        single, single_checks = out["single"]
        assert all(single_checks.values()), (rank, single_checks)
        _assert_transcript(single, oracle, ORACLE_KEYS, f"rank {rank}, single-rank store vs oracle")
        assert (oracle["one"][0] >= 0).all() and (oracle["k100"][0][:, 64:] >= 0).any()    # lists are full; k = 100 reaches page 2
        assert (oracle["filter_none"][0] == -1).all()
        for payload in ("sharded", "replicated"):
            got, checks = out[payload]
            assert all(checks.values()), (rank, payload, checks)
            _assert_transcript(got, oracle, ORACLE_KEYS, f"rank {rank}, payload {payload} vs oracle")
            _assert_transcript(got, single, sorted(single), f"rank {rank}, payload {payload} vs single-rank store")


def _nccl_worker(port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, ROOT)
    try:
        import torch
        import torch.distributed as dist

        import verbatim_rag_amd  # noqa: F401
        from tests.full_text_sharded_cases import session
        from verbatim_rag_amd import vector_stores as vs
        from verbatim_rag_amd.distributed import ShardComm

        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        out = {}
        comm = ShardComm(device=0)
        out["backend"] = (comm.backend, comm.on_gpu, comm.exchange_backend)
        out["sum_int64"] = comm.sum_int64([3, 1 << 40]).tolist()
        for name in ("single", "nccl", "gloo"):
            os.makedirs(os.path.join(tmp, name), exist_ok=True)
        out["single"] = session(None, "sharded", os.path.join(tmp, "single"))[:2]
        world1_dir = os.path.join(tmp, "single", "store_w1_sharded")
        # which library calls the RCCL branch makes: lists of up to DEVICE_K stay in HBM, longer ones page through the host
        calls = {"device": 0, "host": 0}
        search_sharded = vs.TextIndex.search_sharded

        def counted(self, queries, k, allow, n_live_total, sum_df, device_out=None):
            calls["device" if device_out is not None else "host"] += 1
            return search_sharded(self, queries, k, allow, n_live_total, sum_df, device_out=device_out)

        vs.TextIndex.search_sharded = counted
        out["nccl"] = session(comm, "sharded", os.path.join(tmp, "nccl"), world1_dir=world1_dir)[:2]
        vs.TextIndex.search_sharded = search_sharded
        out["calls"] = dict(calls)
        gloo = ShardComm(group=dist.new_group(backend="gloo"), device=0)
        out["gloo"] = session(gloo, "sharded", os.path.join(tmp, "gloo"), world1_dir=world1_dir)[:2]
        st = vs.GpuVectorStore(dense_dim=64, sparse_vocab=300, enable_full_text=True, distributed=True)
        out["store_distributed_flag"] = (st._comm.on_gpu, st._world, st._text_sharded)
        st.close()
        q.put(out)
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:
        import traceback

        q.put(f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}")


def test_sharded_full_text_rccl_world1_device_lists(tmp_path):
    import torch.multiprocessing as mp

    from tests.full_text_sharded_cases import ORACLE_KEYS, oracle_session

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_worker, args=(37500 + (os.getpid() % 2000), str(tmp_path), q))
    p.start()
    out = q.get(timeout=900)
    p.join(120)
    assert isinstance(out, dict), out
    assert out["backend"] == ("nccl", True, "vrag_comm")
    assert out["sum_int64"] == [3, 1 << 40]
    assert out["store_distributed_flag"] == (True, 1, True)
    assert out["calls"]["device"] > 0 and out["calls"]["host"] > 0, out["calls"]      # k <= 64 in HBM, k = 100 through the host
    oracle = oracle_session()
    single = out["single"][0]
    for name in ("single", "nccl", "gloo"):
        got, checks = out[name]
        assert all(checks.values()), (name, checks)
        _assert_transcript(got, oracle, ORACLE_KEYS, f"{name} vs oracle")
        _assert_transcript(got, single, sorted(single), f"{name} vs single-rank store")


def test_library_corpus_stats_override_and_device_lists():
    """The two C entry points on their own: two indexes holding the halves of a corpus, each told the corpus-wide (N, sum dl),
    score their rows to the bits of one index over all rows; `vrag_text_index_search_device` leaves the same lists in HBM."""
    import ctypes as C

    import torch

    import verbatim_rag_amd  # noqa: F401
    from tests.full_text_sharded_cases import O
    from verbatim_rag_amd import vector_stores as vs
    from verbatim_rag_amd.distributed import merge_topk

    texts, words, _flat, _lens = O.zipf_corpus(9000, vocab=600, mean_len=14, seed=4)
    whole = vs.TextIndex()
    whole.add(texts, fold=True)
    owners = [np.arange(0, 9000, 2), np.arange(1, 9000, 2)]                 # interleaved rows: both shards see every block
    shards = []
    for rows in owners:
        ix = vs.TextIndex()
        ix.add([texts[i] for i in rows[:3000]], fold=True)
        ix.add([texts[i] for i in rows[3000:]], fold=False)                 # main + tail
        shards.append(ix)
    live = [np.ones(4500, dtype=bool) for _ in owners]
    live[0][::5] = False
    alive = np.ones(9000, dtype=bool)
    alive[owners[0][::5]] = False
    whole.set_live(alive)
    shards[0].set_live(live[0])
    own = [ix.stats() for ix in shards]
    total = (sum(s["live"] for s in own), sum(s["sum_dl"] for s in own))
    assert total == (whole.stats()["live"], whole.stats()["sum_dl"])
    for ix in shards:
        ix.set_corpus_stats(*total)
    assert [ix.stats()["live"] for ix in shards] == [s["live"] for s in own]        # stats() keeps reporting the index's own rows
    queries = [f"common {words[3]} {words[9]}", words[40].upper(), "qqqzzzunknownterm common", f"{words[2]} {words[2]}"]
    analysed = [ix.query_terms(queries) for ix in shards]
    ref = whole.query_terms(queries)
    for got in analysed:                                                    # the same term lists on every shard, N = the total
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert got[4] == total[0] == ref[4]
    assert np.array_equal(analysed[0][3] + analysed[1][3], ref[3])          # df vectors line up and sum to the corpus df
    assert (ref[3] == 0).any()                                              # the unknown term is listed with df = 0

    def sum_df(_df):
        return analysed[0][3] + analysed[1][3]

    table = [torch.from_numpy(rows.astype(np.int64)).cuda() for rows in owners]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k, allow in ((5, None), (64, None), (10, np.arange(9000) % 3 == 0)):
        want_s, want_i = whole.search(queries, k, allow)
        host, dev = [], []
        for ix, rows, tab in zip(shards, owners, table):
            a = allow[rows] if allow is not None else None
            sc, local = ix.search_sharded(queries, k, a, total[0], sum_df)
            host.append((sc, np.where(local >= 0, rows[np.where(local >= 0, local, 0)], -1)))
            d_s = torch.empty((len(queries), k), dtype=torch.float32, device="cuda")
            d_i = torch.empty((len(queries), k), dtype=torch.int64, device="cuda")
            ix.search_sharded(queries, k, a, total[0], sum_df, device_out=(d_s.data_ptr(), d_i.data_ptr(), tab.data_ptr(), len(rows), stream))
            torch.cuda.synchronize()
            dev.append((d_s.cpu().numpy(), d_i.cpu().numpy()))
        for lists in (host, dev):
            ms, mi = merge_topk(np.stack([s for s, _i in lists]), np.stack([i for _s, i in lists]), k)
            assert np.array_equal(mi, want_i), k
            assert np.array_equal(ms, want_s), k
        for (hs, hi), (ds, di) in zip(host, dev):
            assert np.array_equal(hi, di) and np.array_equal(hs, ds)
    # a row map shorter than a hit's row: hits at or beyond n_map come back as missing (-1 / -inf), in place; the others as before
    ix, rows, tab, k = shards[1], owners[1], table[1], 10
    sc, local = ix.search_sharded(queries, k, None, total[0], sum_df)
    hit_rows = np.sort(local[local >= 0])
    short = int(hit_rows[len(hit_rows) // 2])                               # the median hit row: hits on both sides of the map's end
    inside = (local >= 0) & (local < short)
    assert inside.any() and (local >= short).any()
    d_s = torch.empty((len(queries), k), dtype=torch.float32, device="cuda")
    d_i = torch.empty((len(queries), k), dtype=torch.int64, device="cuda")
    ix.search_sharded(queries, k, None, total[0], sum_df, device_out=(d_s.data_ptr(), d_i.data_ptr(), tab.data_ptr(), short, stream))
    torch.cuda.synchronize()
    assert np.array_equal(d_i.cpu().numpy(), np.where(inside, rows[np.where(inside, local, 0)], -1))
    assert np.array_equal(d_s.cpu().numpy().view(np.uint32), np.where(inside, sc, -np.inf).astype(np.float32).view(np.uint32))
    for ix in shards:                                                       # (0, 0): back to the index's own statistics
        ix.set_corpus_stats(0, 0)
        assert ix.query_terms(queries)[4] == ix.stats()["live"]
    alone = vs.TextIndex()
    alone.add([texts[i] for i in owners[1]], fold=True)
    s1, i1 = shards[1].search(queries, 7)
    s2, i2 = alone.search(queries, 7)
    assert np.array_equal(i1, i2) and np.array_equal(s1, s2)
    for ix in shards + [whole, alone]:
        ix.close()
