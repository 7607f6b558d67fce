"""CPU checks of full-text search on a row-sharded store: the statistics exchange restated on the host (integer sums of N,
sum dl and df over the shards give the unsharded corpus's weights, avgdl and K_d bit for bit, and the merged shard lists are
the unsharded list), the constructor's validation, and the scratch budget of the kernels csrc/fulltext.hip gained."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import full_text_oracle as O  # noqa: E402
from full_text_sharded_cases import ShardOracle  # noqa: E402

import verbatim_rag_amd  # noqa: F401,E402
from verbatim_rag_amd import vector_stores as vs  # noqa: E402
from verbatim_rag_amd.distributed import merge_topk, shard_range  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("world", [2, 3, 8])
def test_summed_shard_statistics_give_the_unsharded_bits(world):
    n = 2000
    texts, words, flat_keys, lens = O.zipf_corpus(n, vocab=300, mean_len=10, seed=world)
    row_keys = np.split(flat_keys, np.cumsum(lens)[:-1])
    whole = O.Bm25Oracle.from_arrays(flat_keys, lens)
    rng = np.random.default_rng(world)
    live = rng.random(n) > 0.2
    whole.set_live(live)
    # rows sharded the way the store cuts its insert batches: contiguously per batch, a 1-row batch leaving ranks empty
    owned = [[] for _ in range(world)]
    for a, b in zip([0, 1, 2, 700, 701, n][:-1], [0, 1, 2, 700, 701, n][1:]):
        for r in range(world):
            lo, hi = shard_range(b - a, r, world)
            owned[r] += list(range(a + lo, a + hi))
    owned = [np.asarray(o, dtype=np.int64) for o in owned]
    assert sorted(np.concatenate(owned).tolist()) == list(range(n))
    shards = []
    for o in owned:
        sh = ShardOracle([row_keys[i] for i in o])
        sh.set_live(live[o])
        shards.append(sh)
    n_total = sum(sh.N for sh in shards)
    sum_dl = sum(int(sh.dl[sh.live].sum()) for sh in shards)
    assert n_total == whole.N and sum_dl == int(whole.dl[whole.live].sum())
    for sh in shards:
        sh.set_corpus(n_total, sum_dl)
    whole_avgdl = np.float32(sum_dl / whole.N)
    for sh, o in zip(shards, owned):
        assert sh.avgdl.tobytes() == whole_avgdl.tobytes()
        assert np.array_equal(sh.kd.view(np.uint32), whole.kd[o].view(np.uint32))
    allow = rng.random(n) > 0.5
    for qi in range(40):
        picks = [words[int(j)] for j in rng.zipf(1.3, size=int(rng.integers(1, 5))) if j < len(words)] or [words[1]]
        text = " ".join(picks + (["qqqzzzunknownterm"] if qi % 4 == 0 else []) + (["COMMON"] if qi % 3 == 0 else []))
        qkeys = O.term_keys(text)
        keys, counts, w_whole = whole.query_terms(qkeys)
        # the term list is the query's alone; every shard reports its own df (0 where it does not hold the term)
        df = np.zeros(len(keys), np.int64)
        for sh in shards:
            df += np.array([sh.df(int(k)) for k in keys], np.int64)
        assert df.tolist() == [whole.df(int(k)) for k in keys]
        w = vs.TextIndex.weights(counts.astype(np.int32), df, n_total)
        assert np.array_equal(w.view(np.uint32), w_whole.view(np.uint32))
        for k, mask in ((7, None), (100, None), (7, allow)):
            want_rows, want_sc = whole.search(qkeys, k, mask)
            lists_s = np.full((world, 1, k), -np.inf, np.float32)
            lists_i = np.full((world, 1, k), -1, np.int64)
            for r, (sh, o) in enumerate(zip(shards, owned)):
                rows, sc = sh.search_weighted(keys, w, k, mask[o] if mask is not None else None)
                lists_i[r, 0, : len(rows)] = o[rows]
                lists_s[r, 0, : len(rows)] = sc
            ms, mi = merge_topk(lists_s, lists_i, k)
            m = len(want_rows)
            assert np.array_equal(mi[0, :m], want_rows) and (mi[0, m:] == -1).all()
            assert np.array_equal(ms[0, :m].view(np.uint32), want_sc.view(np.uint32))


def test_constructor_validates_before_it_constructs(monkeypatch):
    """Full text on a sharded store needs the statistics sum: no process group, or a comm without `sum_int64`, is a ValueError
    raised before anything is built."""
    monkeypatch.setattr(vs._lib, "load", lambda: None)
    monkeypatch.setattr(vs._lib, "require_gpu", lambda: None)
    with pytest.raises(ValueError, match="process group"):
        vs.GpuVectorStore(enable_full_text=True, distributed=True)

    class NoSum:
        world, rank, on_gpu = 2, 0, False

    with pytest.raises(ValueError, match="sum_int64"):
        vs.GpuVectorStore(enable_full_text=True, comm=NoSum())

    class WithSum(NoSum):
        def sum_int64(self, local):
            return np.asarray(local, np.int64)

    st = vs.GpuVectorStore(enable_full_text=True, comm=WithSum())
    assert st._text_sharded and st._world == 2
    assert not vs.GpuVectorStore(enable_full_text=True)._text_sharded           # a single-rank store keeps its own route


def _store_worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    try:
        import torch.distributed as dist

        from sharded_store_cases import cpu_stand_ins
        from full_text_sharded_cases import CpuTextIndex, session
        from verbatim_rag_amd.distributed import ShardComm, merge_topk

        dist.init_process_group("gloo", rank=rank, world_size=world)
        out = {}
        with cpu_stand_ins():
            saved = vs.TextIndex
            vs.TextIndex = CpuTextIndex
            try:
                own = os.path.join(tmp, f"rank{rank}")
                os.makedirs(own, exist_ok=True)
                single, checks, world1_dir = session(None, "sharded", own)
                out["single"] = (single, checks)
                for payload in ("sharded", "replicated"):
                    out[payload] = session(ShardComm(merge=merge_topk), payload, tmp, world1_dir=world1_dir)[:2]
            finally:
                vs.TextIndex = saved
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:
        import traceback

        q.put((rank, f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"))


def test_sharded_store_logic_world2_over_gloo_with_host_stand_ins(tmp_path):
    """The store's sharded full-text route -- statistics sums, the mask at the owned rows, global-row decoding, the exchange,
    save / load across world sizes, both payload modes -- with the device indexes replaced by the host restatement: the
    transcript of the scripted session equals the single-rank store's and the oracle's on every rank."""
    import torch.multiprocessing as mp

    from full_text_sharded_cases import ORACLE_KEYS, oracle_session

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 43500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_store_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=900) for _ in procs], key=lambda x: x[0])
    for p in procs:
        p.join(60)
    oracle = oracle_session()
    for rank, out in res:
        assert isinstance(out, dict), out
        single = out["single"][0]
        for name in ("single", "sharded", "replicated"):
            got, checks = out[name]
            assert all(checks.values()), (rank, name, checks)
            for key in ORACLE_KEYS:
                assert np.array_equal(got[key][0], oracle[key][0]) and np.array_equal(got[key][1], oracle[key][1]), (rank, name, key)
            for key in single:
                assert np.array_equal(got[key][0], single[key][0]) and np.array_equal(got[key][1], single[key][1]), (rank, name, key)


def test_sum_int64_over_gloo():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sum_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(30)
    for rank, out in res:
        assert out == ([3 + (1 << 40) * 3, 0 + 1 + 2, 0], []), (rank, out)


def _sum_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    try:
        import torch.distributed as dist

        from verbatim_rag_amd.distributed import ShardComm, merge_topk

        dist.init_process_group("gloo", rank=rank, world_size=world)
        comm = ShardComm(merge=merge_topk)
        local = np.array([1 + (1 << 40), rank, 0], np.int64)          # sums beyond 2^32 and beyond fp32's integers stay exact
        out = (comm.sum_int64(local).tolist(), comm.sum_int64(np.zeros(0, np.int64)).tolist())
        assert local.tolist() == [1 + (1 << 40), rank, 0]             # the caller's array is not reduced in place
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:
        import traceback

        q.put((rank, f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_full_text_kernels_use_no_scratch():
    from test_full_text_host import _resources

    rows = _resources("fulltext.hip")
    assert not [r["name"] for r in rows if "export" in r["name"]]   # the text search exports through csrc/topk.hip's kernel ...
    mine = [r for r in _resources("topk.hip") if "topk_export_keys_kernel" in r["name"]]   # ... which is held to the same
    assert len(mine) == 1, [r["name"] for r in mine]
    # kd_kernel now reads {N, sum dl} through a pointer the host picks (the index's own pair or the corpus-wide one)
    for r in mine + [r for r in rows if "kd_kernel" in r["name"]]:
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
