"""Model-based test of the ROW-SHARDED `GpuVectorStore` (`comm=`): the seeded operation sequences of tests/store_model.py run
SPMD on every rank of a world, every answer compared with the brute-force model, every rank's answers shown to be the same.  No
test functions here: the CPU run (tests/test_sharded_model_host.py, worlds 2 and 3 over gloo and the stand-in shards) and the
GPU run (tests/test_sharded_model_gpu.py, world 2 over gloo on one GPU and world 1 over the `nccl` backend) share it.

`ShardedRunner` extends `store_model.Runner` by subclassing (store_model.py is untouched and keeps its draws): it builds the
store with `comm=` / `payload=`, reopens it with `load(..., comm=...)`, and at every save + load rank 0 alone also opens the
saved directory with no comm (the world -> 1 re-cut) and asks three model-checked queries there.  Every rank runs the same
(case, seed); nothing the store returns feeds the generator, so all ranks draw the same operations, keep the same full `Model`
and compare with `==` on ids, score bits and enhanced texts.  The data of store_model makes dense and sparse scores exact in any
summation order and the BM25 bits are promised equal under summed statistics: no tolerance anywhere.

The model also knows which rank holds which row (an insert of n rows is cut by `shard_range`, a same-world load keeps the cut);
after every query that knowledge is compared with the rank's `st._owned` table, and it is what the coverage conditions of
`COVER_SHARDED` are told from.

SPMD discipline -- a rank must never leave its peers alone in a collective:
  * a comparison never changes which store calls a rank makes: on the first mismatch the rank RECORDS it (message, op log,
    replay line) and goes on issuing the remaining operations of the sequence (later mismatches are not recorded);
  * a `StoreFault` or any other exception ends the rank: it reports the exception on the queue and runs nothing more;
  * the parent (`run_world`) collects one message per rank under a time limit (`WAIT` seconds: a hang guard, not a
    measurement); on an error, a dead worker or a time-out it terminates the remaining workers and raises `WorldFailed` --
    the caller starts nothing more (the GPU module ends the session);
  * workers are fresh `spawn` children; no process that has opened the GPU replaces its program; a world has at most three.

Every rank returns a sha256 digest of everything it received (ids, score bits, texts, enhanced texts, metadata) per operation;
`assert_ranks_agree` compares them across the ranks and names the first operation that differs.
"""
from __future__ import annotations

import contextlib
import dataclasses
import hashlib
import os
import queue
import sys
import time
import traceback
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):          # a replay from a plain interpreter finds the package and store_model
    if _p not in sys.path:
        sys.path.insert(0, _p)

import store_model as M  # noqa: E402
from store_model import vs  # noqa: E402
from verbatim_rag_amd.distributed import shard_range  # noqa: E402

WAIT = 600            # seconds the parent waits for a world (the limit of tests/test_sharded_gpu.py): a hang guard
N_OPS = M.N_OPS
OPS = ("add", "delete", "query", "batch", "save_load", "filter_only")
OP_P = (0.30, 0.10, 0.12, 0.40, 0.04, 0.04)           # store_model's
TINY_SIZE_P = (0.45, 0.40, 0.10, 0.05)                # insert sizes 1, 7, 64, 300: a rank without rows stays so for a while


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    """One configuration of store_model.CONFIGS on a sharded store.  A sharded store refuses IVF_FLAT, int8, compact() and
    auto_compact, so those configurations are not here."""
    name: str
    config: str
    payload: str = "sharded"
    tiny: bool = False                      # start = 2 at world 3: a rank begins with no rows
    worlds: Tuple[int, ...] = (1, 2, 3)

    def cfg(self, world: int) -> M.Config:
        base = M.CONFIGS[self.config]
        if self.tiny:
            return dataclasses.replace(base, start=2, size_p=TINY_SIZE_P)
        if base.start > 4096:               # "large": every rank's shard still crosses the prefilter image's 4 096-row floor
            return dataclasses.replace(base, start=base.start * world)
        return base


CASES: Dict[str, Case] = {c.name: c for c in (
    Case("f32_subset", "f32_subset"),
    Case("f32_noprefilter_dim72", "f32_noprefilter_dim72"),
    Case("f32_bitmap_device_large", "f32_bitmap_device_large"),
    Case("bf16_subset_large", "bf16_subset_large"),                  # GPU only, as its `host=False` says
    Case("bf16_bitmap", "bf16_bitmap"),
    Case("three_way", "three_way"),
    Case("text_only", "text_only"),
    Case("falsy_id", "falsy_id"),
    Case("f32_subset_replicated", "f32_subset", payload="replicated"),
    Case("three_way_replicated", "three_way", payload="replicated"),
    Case("f32_subset_tiny", "f32_subset", tiny=True, worlds=(3,)),
    Case("three_way_tiny", "three_way", tiny=True, worlds=(3,)),
)}


def cases_of(world: int, host: bool) -> List[str]:
    return [c.name for c in CASES.values() if world in c.worlds and (M.CONFIGS[c.config].host or not host)]


# what the sequences of a case must pass through between them (told from the model and its row -> rank table)
COVER_SHARDED = ("insert_smaller_than_world", "one_rank_takes_all", "short_local_list", "cross_rank_tie", "empty_local_subset")


def coverage_wanted(case: Case, world: int, host: bool) -> Tuple[str, ...]:
    cfg = case.cfg(world)
    want = list(M.COVER_ALL) + ["reopen_world1"]
    if world > 1:
        want += COVER_SHARDED
        if cfg.start > 4096:
            # every rank holds thousands of rows, and every filter of store_model that passes k rows at all passes hundreds
            # of them on every rank: no rank's list comes up short there
            want.remove("short_local_list")
        if case.tiny:
            want.append("rank_without_rows_queried")      # the other cases start with hundreds of rows on every rank
        if cfg.dense and cfg.sparse:
            want.append("shared_id_across_ranks")         # a store with one method never fuses
        if cfg.text:
            want.append("text_totals_resummed")
    if cfg.falsy:
        want.append("falsy_id_fusion")
    if dict(M._routes(cfg, host)).get("rrf_route") == "device":
        want.append("rrf_device_batch")
    return tuple(want)


def check_coverage(case: Case, world: int, host: bool, seen: Dict[str, int], wanted=None) -> None:
    missing = [name for name in (wanted or coverage_wanted(case, world, host)) if not seen.get(name)]
    assert not missing, f"{case.name} world {world}: the sequences never passed through {missing} (seen: {seen})"


# ------------------------------------------------------------------------------------------------ the runner
class _NotingModel(M.Model):
    """`Model` that keeps the last question and its answer for the coverage conditions (no second computation)."""
    last = None

    def answer(self, mode, qs, top_k, flt, weights, rrf_k):
        hits = super().answer(mode, qs, top_k, flt, weights, rrf_k)
        self.last = (mode, qs, top_k, flt, weights, hits)
        return hits


def _full(results) -> list:
    """Everything a caller sees of a result list (or of a batch of them)."""
    if results and isinstance(results[0], list):
        return [_full(r) for r in results]
    return [(r.id, float(r.score).hex(), r.text, r.enhanced_text, sorted(r.metadata.items())) for r in results]


class ShardedRunner(M.Runner):
    """One sequence on one rank: `ShardedRunner(case, seed, tmp_dir, host, comm).run_recorded()`; every rank of the world
    runs it with the same arguments (`tmp_dir` shared)."""

    def __init__(self, case: Case, seed: int, tmp_dir: str, host: bool, comm, n_ops: int = N_OPS, modes: Optional[list] = None,
                 op_p: Optional[Tuple[float, ...]] = None):
        self.case, self.comm, self.world, self.rank = case, comm, comm.world, comm.rank
        tmp = os.path.join(str(tmp_dir), f"{case.name}-w{self.world}")
        os.makedirs(tmp, exist_ok=True)
        super().__init__(case.cfg(self.world), seed, tmp, host, n_ops=n_ops, modes=modes)
        self.model = _NotingModel(self.cfg)
        self.op_p = np.asarray(op_p or OP_P, float)
        self.mismatch: Optional[dict] = None
        self.digests: List[Tuple[str, "hashlib._Hash"]] = []
        self._digesting = True
        self._last_change: Optional[set] = None       # ranks whose rows the last insert / delete touched
        self._change_before: Optional[set] = None     # the same, when that was the operation directly before this one

    # -- the store: built and reopened with the comm
    def _kwargs(self) -> dict:
        return dict(M._routes(self.cfg, self.host), comm=self.comm, payload=self.case.payload)

    def _check_route(self, st) -> None:
        want = dict(M._routes(self.cfg, self.host)).get("filter_route", "subset")
        if getattr(self.comm, "on_gpu", False):
            want = "subset"            # the device-resident exchange carries no host lists: the constructor keeps "subset"
        assert st._filter_route == want, (self.case.name, st._filter_route, want)
        assert (st._world, st._rank) == (self.world, self.rank)

    def _new_store(self):
        st = super()._new_store()
        self._check_route(st)
        return st

    # -- answers: digested as received, compared without ever raising
    def _call(self, fn, *a, **kw):
        out = super()._call(fn, *a, **kw)
        if self._digesting and isinstance(out, list):
            at = len(self.log) - 1
            if not self.digests or self.digests[-1][0] != at:
                self.digests.append((at, hashlib.sha256()))
            self.digests[-1][1].update(repr(_full(out)).encode())
        return out

    def replay_line(self) -> str:
        return (f"sharded_model.replay({self.case.name!r}, seed={self.seed}, world={self.world}, host={self.host}, "
                f"backend={self.comm.backend!r}, n_ops={self.n_ops})")

    def _fail(self, what: str, got, want) -> None:
        """Records the first mismatch; never raises (module docstring, SPMD discipline)."""
        if self.mismatch is not None:
            return
        got, want = list(got), list(want)
        at = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
        rows = self.model.rows
        message = (f"case {self.case.name!r} (config {self.cfg.name!r}) seed {self.seed} world {self.world} rank {self.rank} "
                   f"payload {self.case.payload!r} op {len(self.log) - 1}: {self.log[-1]}\n"
                   f"  {what}: {len(got)} hits for {len(want)} expected, first difference at rank {at}\n"
                   f"  got      {got[at:at + 3]}\n  expected {want[at:at + 3]}\n  replay: {self.replay_line()}\n  ops: "
                   + " | ".join(self.log))
        self.mismatch = dict(message=message, what=what, op=self.log[-1], op_index=len(self.log) - 1, at=at, got=got, want=want,
                             log=list(self.log), owner_of={r.enh: int(r.owner) for r in rows},
                             dead=sorted(r.enh for r in rows if not r.alive), rank=self.rank)

    # -- operations: the model learns the owner of every row
    def _add(self, n: int, reuse: bool, bulk: bool) -> None:
        base = len(self.model.rows)
        super()._add(n, reuse, bulk)
        touched = set()
        for r in range(self.world):
            lo, hi = shard_range(n, r, self.world)
            for row in self.model.rows[base + lo:base + hi]:
                row.owner = r
            if hi > lo:
                touched.add(r)
        if len(touched) < self.world:
            self.cover.hit("insert_smaller_than_world")
        self._last_change = touched

    def _delete(self, n: int) -> None:
        rows = self.model.rows
        before = [r.alive for r in rows]
        super()._delete(n)
        self._last_change = {r.owner for r, was in zip(rows, before) if was and not r.alive}

    def _save_load(self) -> None:
        super()._save_load()                          # save (ends in a barrier), close, load with the comm: the cut is kept
        self._check_route(self.store)
        self._last_change = None
        path = os.path.join(self.tmp, f"{self.cfg.name}-{self.seed}-{self.saves - 1}")
        rng, asked = self.rng, []
        for _ in range(3):                            # drawn on every rank: the draws stay aligned
            mode, weights, _w = self.modes[int(rng.choice(len(self.modes), p=self._mode_p))]
            top_k = int(rng.choice(M.TOP_KS))
            flt = int(rng.choice(len(M.FILTERS), p=self._filter_p))
            rrf_k = (60, 10)[int(rng.integers(0, 2))]
            asked.append((mode, weights, top_k, flt, rrf_k, self._queries(1)[0]))
        if self.rank != 0:
            return
        # the world -> 1 re-cut: rank 0 alone, no comm, no collective
        self._digesting = False
        try:
            single = self._call(vs.GpuVectorStore.load, path, **dict(M._routes(self.cfg, self.host)))
            try:
                self._tune(single)
                assert single._world == 1 and len(single._owned) == len(self.model.rows)
                for i, (mode, weights, top_k, flt, rrf_k, q) in enumerate(asked):
                    want = self.model.expected(M.Model.answer(self.model, mode, [q], top_k, flt, weights, rrf_k)[0])
                    d = q["dense"]
                    got = M.got_of(self._call(single.query, dense_query=None if d is None else d.tolist(), sparse_query=q["sparse"],
                                              text_query=q["text"], **self._store_kwargs(mode, weights, top_k, flt, rrf_k)))
                    if got != want:
                        self._fail(f"world -> 1 reopen, query {i} ({mode} k={top_k} f={flt})", got, want)
                self.cover.hit("reopen_world1")
            finally:
                single.close()
        finally:
            self._digesting = True

    # -- after every query: what the model can tell about the ranks
    def _note_sharded(self) -> None:
        mode, qs, top_k, flt, weights, hits = self.model.last
        rows, W, hit = self.model.rows, self.world, self.cover.hit
        if W == 1 or not rows:
            return
        owner = np.asarray([r.owner for r in rows], np.int64)
        alive = np.asarray([r.alive for r in rows], dtype=bool)
        passing = self.model.passing(flt)
        held = np.bincount(owner, minlength=W)
        per = np.bincount(owner[passing], minlength=W)
        if (held == 0).any():
            hit("rank_without_rows_queried")
        if flt != 0 and (per > 0).any() and ((per == 0) & (np.bincount(owner[alive], minlength=W) > 0)).any():
            hit("empty_local_subset")
        if mode == "filter_only":
            return
        limit = top_k if mode in M.METHODS else 2 * top_k
        if len(passing) >= limit and (per < limit).any():
            hit("short_local_list")                          # that rank's list goes into the merge with a -1 tail
        for one in hits:
            on = [int(owner[r]) for r, _s in one]
            if len(on) >= 2 and len(set(on)) == 1 and (per > 0).sum() > 1:
                hit("one_rank_takes_all")
            if mode in M.METHODS and any(a[1] == b[1] and oa != ob for a, b, oa, ob in zip(one, one[1:], on, on[1:])):
                hit("cross_rank_tie")                        # the merge must order them by global row
        fused = self._fused(mode, weights, qs[0]) if mode in ("hybrid", "weighted") else [mode]
        if len(fused) > 1:
            where: Dict[str, set] = {}
            for r, o in zip(rows, owner.tolist()):
                if r.alive:
                    where.setdefault(r.id, set()).add(o)
            if any(len(v) > 1 for v in where.values()):
                hit("shared_id_across_ranks")
        if "full_text" in fused and self.cfg.text and self._change_before and len(self._change_before) < W:
            hit("text_totals_resummed")                      # the last change touched other ranks' rows only, for some rank

    def _check_owned(self) -> None:
        mine = [i for i, r in enumerate(self.model.rows) if r.owner == self.rank]
        got = self.store._owned.data.tolist()
        if got != mine:
            self._fail("row table (_owned)", got, mine)

    def _after_query(self) -> None:
        self._note_sharded()
        self._check_owned()
        self._observe()

    # -- the sequence: store_model's loop with its draws, the sharded notes behind every query
    def _run(self, watch) -> None:
        rng = self.rng
        self._mode_p = np.asarray([w for _m, _x, w in self.modes], float) / sum(w for _m, _x, w in self.modes)
        self._filter_p = np.asarray([w for _e, _p, w in M.FILTERS], float) / sum(w for _e, _p, w in M.FILTERS)
        self.store = self._new_store()
        self.log.append(f"add {self.start}")
        self._add(self.start, reuse=False, bulk=True)
        while len(self.log) < self.n_ops:
            op = OPS[int(rng.choice(len(OPS), p=self.op_p / self.op_p.sum()))]
            self._last_change = None
            if op == "add":
                n = int(rng.choice(M.ADD_SIZES, p=self.cfg.size_p))
                reuse, bulk = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
                reuse = reuse and len(self.log) >= self.cfg.reuse_from
                self.log.append(f"add {n}{' reuse' if reuse else ''}{' bulk' if bulk else ''}")
                self._add(n, reuse, bulk)
            elif op == "delete":
                n = int(rng.choice((1, 5, 60), p=(0.4, 0.4, 0.2)))
                self.log.append(f"delete {n}")
                self._delete(n)
            elif op == "save_load":
                self.log.append("save_load")
                self._save_load()
            elif op == "filter_only":
                self._filter_only()
                self._after_query()
            else:
                self._query_op(batch=op == "batch")
                self._after_query()
            self._change_before = self._last_change
            if watch.failed:
                raise M.StoreFault(f"{self._where()}: {watch.failed[0]}")
        assert self.cover.empty * 4 <= max(self.cover.queries, 1), (self.case.name, self.seed, self.cover.empty, self.cover.queries)

    def run_recorded(self) -> dict:
        """Runs the sequence; what the parent needs of it.  An exception passes through: it ends the rank."""
        t0 = time.perf_counter()
        cover = self.run()
        return dict(case=self.case.name, seed=self.seed, world=self.world, rank=self.rank, payload=self.case.payload,
                    mismatch=self.mismatch, digests=[(at, self.log[at], h.hexdigest()) for at, h in self.digests],
                    seen=dict(cover.seen), queries=cover.queries, empty=cover.empty, rows_max=cover.rows_max,
                    ops=len(self.log), replay=self.replay_line(), seconds=time.perf_counter() - t0)


# ------------------------------------------------------------------------------------------------ defects (negative controls)
def _merge_ties_by_list_order(scores, ids, k):
    """`merge_topk` with equal scores left in list order (rank 0's entries first) instead of by global row."""
    W, Q, kk = scores.shape
    s = np.ascontiguousarray(scores.transpose(1, 0, 2)).reshape(Q, W * kk).astype(np.float32)
    i = np.ascontiguousarray(ids.transpose(1, 0, 2)).reshape(Q, W * kk).astype(np.int64)
    s = np.where(i < 0, -np.inf, s).astype(np.float32)
    order = np.argsort(-s.astype(np.float64), axis=1, kind="stable")[:, :k]
    return np.take_along_axis(s, order, axis=1), np.take_along_axis(i, order, axis=1)


@contextlib.contextmanager
def injected(defect: Optional[str], comm):
    """One defect, by plain attribute replacement, taken back afterwards.  Every one of them leaves the ranks' control flow
    replicated (a defect that sent the ranks into different collectives would hang the world instead of failing a comparison)."""
    store = vs.GpuVectorStore
    undo = []
    if defect == "merge_ties_by_list_order":
        undo.append((comm, "_merge", comm._merge))
        comm._merge = _merge_ties_by_list_order
    elif defect == "union_mask_local":                 # only safe under filter-only queries: a search would branch on the mask
        comm.union_mask = lambda local: np.asarray(local, dtype=bool).copy()
        undo.append((comm, "union_mask", None))
    elif defect == "sum_int64_local":                  # every rank scores with its own statistics
        comm.sum_int64 = lambda local: np.array(local, dtype=np.int64, copy=True).reshape(-1)
        undo.append((comm, "sum_int64", None))
    elif defect == "text_totals_kept_over_delete":
        real_delete = store.delete

        def delete(self, ids):
            kept = self._text_totals
            real_delete(self, ids)
            self._text_totals = kept

        undo.append((store, "delete", real_delete))
        store.delete = delete
    elif defect == "owned_shifted_at_load":
        # rank 1's table says "one row lower" from a load until the store is closed; the file a save writes stays sound
        # (the saved shards must cover every row once, or the next load refuses them on every rank)
        saved_load, real_save = store.__dict__["load"], store.save
        real_load = saved_load.__func__

        def load(cls, path, **kw):
            st = real_load(cls, path, **kw)
            owned = st._owned.data
            if st._comm is not None and st._rank == 1 and len(owned) and owned[0] > 0:
                st._owned = vs._Column(np.int64, first=owned - 1)
                st._shifted = len(owned)              # rows inserted later get their true numbers
            return st

        def save(self, path):
            shifted = getattr(self, "_shifted", 0)
            self._owned.data[:shifted] += 1
            try:
                real_save(self, path)
            finally:
                self._owned.data[:shifted] -= 1

        undo += [(store, "load", saved_load), (store, "save", real_save)]
        store.load, store.save = classmethod(load), save
    elif defect is not None:
        raise ValueError(f"unknown defect {defect!r}")
    try:
        yield
    finally:
        for obj, name, value in undo:
            if value is None:
                delattr(obj, name)                     # an instance attribute that shadowed the method
            else:
                setattr(obj, name, value)


@contextlib.contextmanager
def counting_resident(counts: Dict[str, int]):
    """Counts the dense / sparse searches of at most `DEVICE_K` rows on a store with a comm (`wanted`; rank 0's world -> 1
    reopen has none), the searches that took the device-resident exchange (`resident`) and the exchange payloads handed out in HBM
    (`slots`: one per resident dense / sparse search and one per sharded full-text search with device lists), through wrappers
    of `_device_topk`, `_device_topk_resident` and `_resident_slots`."""
    store = vs.GpuVectorStore
    real_topk, real_resident, real_slots = store._device_topk, store._device_topk_resident, store._resident_slots

    def topk(self, kind, parts, shard_rows, queries, k, rows_dev=None, nprobe=None):
        if self._comm is not None and k <= self.DEVICE_K:
            counts["wanted"] = counts.get("wanted", 0) + 1
        return real_topk(self, kind, parts, shard_rows, queries, k, rows_dev, nprobe)

    def resident(self, parts, rows_dev, q_in, Q, k):
        counts["resident"] = counts.get("resident", 0) + 1
        return real_resident(self, parts, rows_dev, q_in, Q, k)

    def slots(self, Q, k):
        counts["slots"] = counts.get("slots", 0) + 1
        return real_slots(self, Q, k)

    store._device_topk, store._device_topk_resident, store._resident_slots = topk, resident, slots
    try:
        yield
    finally:
        store._device_topk, store._device_topk_resident, store._resident_slots = real_topk, real_resident, real_slots


# ------------------------------------------------------------------------------------------------ worker and parent
def worker(rank: int, world: int, port: int, q, spec: dict) -> None:
    """One rank.  `spec`: backend ("gloo" / "nccl"), host (stand-in shards and the host merge), jobs [(case, seed)], tmp (a
    directory all ranks share) and optionally defect, modes, op_p, n_ops."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    if spec["backend"] == "nccl":
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")         # as tests/test_nccl_gpu.py starts its world
    try:
        import torch
        import torch.distributed as dist

        from verbatim_rag_amd.distributed import ShardComm, merge_topk

        if spec["backend"] == "nccl":
            torch.cuda.set_device(0)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        host = spec["host"]
        comm = ShardComm(merge=merge_topk) if host else ShardComm(device=0)
        results = []
        with (M.stand_ins() if host else contextlib.nullcontext()), injected(spec.get("defect"), comm):
            for name, seed in spec["jobs"]:
                counts: Dict[str, int] = {}
                with counting_resident(counts):
                    runner = ShardedRunner(CASES[name], seed, spec["tmp"], host, comm, n_ops=spec.get("n_ops", N_OPS),
                                           modes=spec.get("modes"), op_p=spec.get("op_p"))
                    results.append(dict(runner.run_recorded(), counts=counts))
        q.put((rank, "done", dict(results=results, backend=comm.backend, on_gpu=comm.on_gpu, exchange_backend=comm.exchange_backend)))
        dist.barrier()
        comm.close()
        dist.destroy_process_group()
    except BaseException as exc:   # reported at once: the parent must not wait for its time limit
        q.put((rank, "error", f"rank {rank}: {type(exc).__name__}: {exc}\n{traceback.format_exc()}"))


class WorldFailed(RuntimeError):
    """A rank reported an exception, died or did not answer in time; the remaining workers have been terminated."""


def run_world(world: int, spec: dict, port_base: int = 35500, wait: float = WAIT) -> List[dict]:
    """Spawns the world, returns the ranks' reports in rank order."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = port_base + (os.getpid() % 2000)
    procs = [ctx.Process(target=worker, args=(r, world, port, q, spec)) for r in range(world)]
    for p in procs:
        p.start()
    out: Dict[int, dict] = {}
    deadline = time.monotonic() + wait
    try:
        while len(out) < world:
            try:
                rank, kind, body = q.get(timeout=2.0)
            except queue.Empty:
                gone = [(r, p.exitcode) for r, p in enumerate(procs) if r not in out and p.exitcode is not None]
                if gone:
                    raise WorldFailed(f"world {world}: workers ended without a report (rank, exit code): {gone}") from None
                if time.monotonic() > deadline:
                    raise WorldFailed(f"world {world}: no report within {wait} s from ranks {sorted(set(range(world)) - set(out))}") from None
                continue
            if kind == "error":
                raise WorldFailed(f"world {world}: {body}")
            out[rank] = body
    except WorldFailed:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(30)
        raise
    for p in procs:
        p.join(60)
        if p.is_alive():
            p.terminate()
    return [out[r] for r in range(world)]


def assert_ranks_agree(reports: List[dict]) -> None:
    """Every rank received the same answers, operation by operation; names the first operation that differs."""
    first = reports[0]["results"]
    for rank, rep in enumerate(reports[1:], start=1):
        assert len(rep["results"]) == len(first)
        for a, b in zip(first, rep["results"]):
            assert (a["case"], a["seed"]) == (b["case"], b["seed"])
            if a["digests"] != b["digests"]:
                at = next((x for x, y in zip(a["digests"], b["digests"]) if x != y), None)
                raise AssertionError(f"case {a['case']!r} seed {a['seed']} world {a['world']} payload {a['payload']!r}: rank 0 and "
                                     f"rank {rank} received different answers, first at op {at[0] if at else 'count'}: "
                                     f"{at[1] if at else (len(a['digests']), len(b['digests']))}\n  replay: {a['replay']}")


def by_case(reports: List[dict]) -> Dict[str, List[List[dict]]]:
    """case -> per sequence, the ranks' records."""
    out: Dict[str, List[List[dict]]] = {}
    for i, rec in enumerate(reports[0]["results"]):
        out.setdefault(rec["case"], []).append([rep["results"][i] for rep in reports])
    return out


def merged_seen(sequences: List[List[dict]]) -> Dict[str, int]:
    """Coverage counts of a case over its sequences.  Told from the model, they are the same on every rank -- except what only
    rank 0 does (the world -> 1 reopen) and the rank-local transitions of store_model: the maximum over the ranks."""
    seen: Dict[str, int] = {}
    for ranks in sequences:
        for name in {n for r in ranks for n in r["seen"]}:
            seen[name] = seen.get(name, 0) + max(r["seen"].get(name, 0) for r in ranks)
    return seen


def replay(case: str, seed: int, world: int, host: bool = True, backend: str = "gloo", n_ops: int = N_OPS, tmp: Optional[str] = None,
           **spec) -> List[dict]:
    """One sequence again, in a fresh world; prints what each rank recorded."""
    import tempfile

    reports = run_world(world, dict(backend=backend, host=host, jobs=[(case, seed)], tmp=tmp or tempfile.mkdtemp(prefix="vrag_sharded_"),
                                    n_ops=n_ops, **spec))
    for rep in reports:
        rec = rep["results"][0]
        print(rec["mismatch"]["message"] if rec["mismatch"] else f"rank {rec['rank']}: no mismatch; seen {rec['seen']}")
    return reports
