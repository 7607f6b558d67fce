"""The operation sequences of tests/store_model.py against `GpuVectorStore` on the device: two seeds per configuration, every
answer `==` the brute-force model in ids and score bits, and the same coverage conditions as the CPU run.

What the configurations are meant to reach is in `store_model.CONFIGS[...].route`.  The launch log of the harness library
covers the pass kernels of the unfiltered dense and sparse searches only (not the tiled search, the filtered searches, IVF or
SQ8: include/vrag_amd_debug.h), so the four configurations in `LOGGED` run their resident and subset shards through that
library and assert the kernels they took; the others rest on the configuration table.

A failing library call (or a search leg the store dropped after one) ends the session: nothing more is launched."""
import ctypes as C

import numpy as np
import pytest

import store_model as M
from store_model import vs
from verbatim_rag_amd import _lib

pytestmark = pytest.mark.gpu

SEEDS = {name: (0, 1) for name in M.CONFIGS}
SEEDS["f32_ivf_large"] = (0, 2)        # the pair whose sequences pass through every transition between them (sparse fold: seed 2)


class _Logged:
    """Opens the shard in the harness library, whose searches write the launch log."""

    def _open(self, create, *args):
        self._lib = _lib.load_debug()
        self._h = C.c_void_p()
        _lib.check_debug(create, getattr(self._lib, create)(*args, C.byref(self._h)))


class LoggedDense(_Logged, vs.DenseShard):
    pass


class LoggedSparse(_Logged, vs.SparseShard):
    pass


def _read_log(dbg):
    names = {v: n for n, v in _lib.DEBUG_TOPK_LAUNCH_IDS.items()}
    cap = 4096
    buf = (C.c_int32 * (3 * cap))()
    count, ovf = C.c_int32(-1), C.c_int32(-1)
    _lib.check_debug("vrag_debug_topk_launch_log_read", dbg.vrag_debug_topk_launch_log_read(buf, cap, C.byref(count), C.byref(ovf)))
    e = np.ctypeslib.as_array(buf)[: 3 * min(count.value, cap)].reshape(-1, 3)
    return {names[int(i)] for i, _a, _b in e}


_PF = {"PF_PREFIX", "PF_COLLECT", "PF_COLLECT_MULTI", "PF_RESCORE_LIST", "PF_RESCORE", "PF_COMBINE"}
_SPARSE = [{"SPARSE"}, {"SPARSE_MULTI"}]       # one query, a batch
# Per configuration: groups of kernels of which the unfiltered searches must have launched at least one each, and kernels they
# must not have launched.  From the route planner (csrc/topk.hip dense_plan): the prefilter image answers fp32 shards of at
# least 4 096 rows for k <= 16 and nothing below that size; bf16 rows never run an fp32 kernel; the exact kernels need
# dim % 32 == 0.
LOGGED = {
    "f32_subset": ([{"DENSE_F32"}] + _SPARSE, _PF | {"DENSE_BF16", "MFMA", "MFMA2"}),
    "f32_noprefilter_dim72": ([{"DENSE_F32"}] + _SPARSE, _PF | {"DENSE_BF16", "MFMA", "MFMA2", "EXACT", "EXACT2"}),
    "f32_bitmap_device_large": ([_PF, {"DENSE_F32", "EXACT", "EXACT2"}] + _SPARSE, {"DENSE_BF16"}),
    "bf16_subset_large": ([{"DENSE_BF16"}] + _SPARSE, _PF | {"DENSE_F32"}),
}


def _run(name, tmp_path, monkeypatch):
    cfg = M.CONFIGS[name]
    dbg = None
    if name in LOGGED:
        dbg = _lib.load_debug()
        monkeypatch.setattr(vs, "DenseShard", LoggedDense)
        monkeypatch.setattr(vs, "SparseShard", LoggedSparse)
        dbg.vrag_debug_topk_launch_log_reset()
    total, launched = M.Coverage(), set()
    for seed in SEEDS[name]:
        try:
            total.merge(M.Runner(cfg, seed, tmp_path, host=False).run())
        except M.StoreFault as e:
            pytest.exit(f"store model: {e}", returncode=3)
        if dbg is not None:
            launched |= _read_log(dbg)
            dbg.vrag_debug_topk_launch_log_reset()
    return total, launched


@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_sequences_match_the_model_on_the_device(name, tmp_path, monkeypatch):
    total, launched = _run(name, tmp_path, monkeypatch)
    print(f"{name}: rows up to {total.rows_max}, transitions {dict(sorted(total.seen.items()))}, launches {sorted(launched)}")
    M.check_coverage(M.CONFIGS[name], total, host=False)
    if M.CONFIGS[name].start > 4096:
        assert total.rows_max > 6000
    if name in LOGGED:
        groups, never = LOGGED[name]
        assert all(group & launched for group in groups) and not (never & launched), sorted(launched)


@pytest.mark.parametrize("n_q", [2, 70])
@pytest.mark.parametrize("weights", [None, {"dense": 0.7, "sparse": 0.3}], ids=["hybrid", "weighted"])
@pytest.mark.parametrize("rrf_route", ["host", "device"])
def test_rows_that_share_an_id_fuse_as_one_candidate(n_q, weights, rrf_route):
    """60 rows over 20 ids: `query_batch` == per-query `query` == the model, whichever fusion route is configured."""
    cfg = M.CONFIGS["f32_subset"]
    rng = np.random.default_rng(5)
    dense = M.unit_rows(rng, 60, cfg.dim)
    rows = [M.Row(f"id{i % 20}", i, dense[i], M.sparse_row(rng, 6), f"text {i}", [], M.metadata_of(i)) for i in range(60)]
    model = M.Model(cfg)
    model.add(rows)
    queries = [{"dense": q, "sparse": M.sparse_row(rng, 5)} for q in M.unit_rows(rng, n_q, cfg.dim)]
    kw = dict(top_k=5, hybrid_weights=weights) if weights else dict(top_k=5, search_type="hybrid")
    want = [model.expected(hits) for hits in model.answer("weighted" if weights else "hybrid", queries, 5, 0, weights, 60)]
    st = vs.GpuVectorStore(dense_dim=cfg.dim, sparse_vocab=M.VOCAB, rrf_route=rrf_route)
    try:
        st.add_vectors([r.id for r in rows], dense, [r.sparse for r in rows], [r.text for r in rows], [r.enh for r in rows],
                       [r.meta for r in rows])
        batch = st.query_batch(dense_queries=[q["dense"].tolist() for q in queries], sparse_queries=[q["sparse"] for q in queries], **kw)
        single = [st.query(dense_query=q["dense"].tolist(), sparse_query=q["sparse"], **kw) for q in queries]
    except _lib.VragError as e:
        pytest.exit(f"store model: {e}", returncode=3)
    finally:
        st.close()
    assert [M.got_of(r) for r in single] == want
    assert [M.got_of(r) for r in batch] == want
