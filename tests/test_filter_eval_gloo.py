"""`filter_eval="device"` through the store's wiring without a GPU: the shards are the CPU stand-ins of
tests/sharded_store_cases.py and the `RowFilter` is a stand-in that answers from the numpy interpreter of tests/filter_cases.py
(and insists on what the real handle insists on: every row uploaded once, in order, before it is evaluated).  Single rank, then
world 2 over gloo: sharded and replicated payloads give the single-rank masks."""
import contextlib
import logging
import os
import sys

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from filter_cases import interpret, random_rows
from verbatim_rag_amd import vector_stores as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ["year >= 2020", 'year >= 2010 and source != "web"', "(year < 2000 or year > 2025) and not peer == true",
           'source < "b" or tag in [5, "5", true]', "misc != 1", 'not (score <= 0 or source == "")', 'source == "web"', None]


class CpuRowFilter:
    """Stand-in for `shards.RowFilter` (tests only)."""

    made = 0

    def __init__(self, device=0):
        type(self).made += 1
        self.kinds, self.payload, self.evals = [], [], 0

    def add_column(self):
        self.kinds.append(np.zeros(0, np.uint8))
        self.payload.append(np.zeros(0, np.uint64))
        return len(self.kinds) - 1

    def append(self, col, kinds, payload):
        assert len(kinds) == len(payload) and len(kinds) > 0
        self.kinds[col] = np.concatenate([self.kinds[col], kinds])
        self.payload[col] = np.concatenate([self.payload[col], payload])

    def rows(self, col):
        return len(self.kinds[col])

    def eval_program(self, program, columns, n_rows):
        assert program.over_limit() is None and len(columns) == len(program.keys)
        for (col, meta), key in zip(columns, program.keys):
            assert meta.key == key and meta.exact and len(meta) == n_rows
            assert np.array_equal(self.kinds[col], meta.kinds) and np.array_equal(self.payload[col], meta.payload)   # what was uploaded
        self.evals += 1
        return interpret(program, [meta for _col, meta in columns])[:n_rows]

    def close(self):
        pass


@contextlib.contextmanager
def stand_ins():
    from sharded_store_cases import cpu_stand_ins

    saved = vs.RowFilter
    vs.RowFilter = CpuRowFilter
    try:
        with cpu_stand_ins():
            yield
    finally:
        vs.RowFilter = saved


def _session(comm=None, payload="sharded", filter_eval="device"):
    """Inserts in three batches with deletes in between; the mask of every filter after each step."""
    rows = random_rows(230, seed=3)
    rng = np.random.default_rng(2)
    dense = np.where(rng.random((len(rows), 64)) < 0.5, 0.5, -0.5).astype(np.float32)
    st = vs.GpuVectorStore(dense_dim=64, enable_sparse=False, sparse_vocab=None, comm=comm, payload=payload, filter_eval=filter_eval)
    out = []
    for a, b in ((0, 1), (1, 150), (150, 230)):
        st.add_vectors([f"r{i}" for i in range(a, b)], dense[a:b].tolist(), None, [f"t{i}" for i in range(a, b)], [""] * (b - a), rows[a:b])
        for flt in FILTERS:
            m = st._mask(flt)
            out.append(None if m is None else m.tolist())
        st.delete([f"r{i}" for i in range(a, b, 7)])
        out.append(st._mask(FILTERS[1]).tolist())
    return out, st


def test_store_wiring_single_rank_equals_the_host_route(caplog):
    with stand_ins():
        want, host = _session(filter_eval="host")
        got, dev = _session(filter_eval="device")
        assert got == want
        assert host._metadata.row_filter is None and not host._metadata.columns
        assert sorted(dev._metadata.columns) == ["misc", "peer", "score", "source", "tag", "year"]       # the lookup filter built none of its own
        assert dev._metadata.row_filter.evals == 3 * 6 + 3 and all(dev._metadata.row_filter.rows(c) == 230 for c in dev._metadata.row_filter_cols.values())
        assert any(m is not None and any(m) and not all(m) for m in want)
        # fallbacks: a NaN, a program over the limits -- answered on the host, said once per filter string, never an error
        evals = dev._metadata.row_filter.evals
        long = " or ".join(f"year == {i}" for i in range(65))
        for st in (host, dev):
            st.add_vectors(["nan"], [[0.5] * 64], None, ["t"], [""], [{"score": float("nan"), "year": 2021}])
        with caplog.at_level(logging.INFO, logger="verbatim_rag_amd.vector_stores"):
            for _ in range(2):
                for flt in ("score > 0.5 or year > 2020", long, "year > 2020"):
                    assert np.array_equal(dev._mask(flt), host._mask(flt)), flt
                dev._drop_subsets()
        said = [r.getMessage() for r in caplog.records if "evaluated on the host" in r.getMessage()]
        assert len(said) == 2 and "NaN" in said[0] and "65 leaves" in said[1], said
        assert dev._metadata.row_filter.evals == evals + 2                                                     # "year > 2020", twice
        made = CpuRowFilter.made
        dev.close()
        assert dev._metadata.row_filter is None and not dev._metadata.row_filter_cols
        assert np.array_equal(dev._mask("year > 2019"), host._mask("year > 2019")) and CpuRowFilter.made == made + 1   # uploaded again
    with stand_ins(), pytest.raises(ValueError, match="filter_eval must be 'host' or 'device'"):
        vs.GpuVectorStore(dense_dim=64, enable_sparse=False, sparse_vocab=None, filter_eval="gpu")


def _mask_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import torch.distributed as dist

        import verbatim_rag_amd  # noqa: F401
        from test_filter_eval_gloo import _session, stand_ins
        from verbatim_rag_amd.distributed import ShardComm, merge_topk

        dist.init_process_group("gloo", rank=rank, world_size=world)
        with stand_ins():
            single, _st = _session(comm=None, filter_eval="host")
            ok = True
            for payload in ("sharded", "replicated"):
                got, st = _session(comm=ShardComm(merge=merge_topk), payload=payload)
                held = len(st._meta)
                if got != single:
                    ok = f"payload={payload}: the masks differ from the single-rank host route"
                elif not st._metadata.row_filter or st._metadata.row_filter.evals == 0:
                    ok = f"payload={payload}: the device route did not run"
                elif (payload == "sharded") != (held < 230):
                    ok = f"payload={payload}: rank {rank} holds {held} metadata rows"
        q.put((rank, ok))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as exc:   # never leave the parent waiting for its timeout
        import traceback

        q.put((rank, f"{type(exc).__name__}: {exc}\n{traceback.format_exc()}"))


def test_sharded_and_replicated_payloads_give_the_single_rank_masks_world2_gloo():
    from test_distributed_gloo import _run_world

    assert _run_world(_mask_worker) == [(0, True), (1, True)]
