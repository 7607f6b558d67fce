"""Batched weighted RRF on the GPU (`vrag_rrf_fuse`, csrc/fuse.hip; `rrf_fuse_rows_device`; `GpuVectorStore(rrf_route="device")`)
against the numpy statement `rrf_merge_rows` and the fixtures captured from the reference: rows equal and distances equal as
float64 BITS everywhere -- there is no tolerance in this file.  Shapes are the smallest that cross a boundary of the kernels:
one wave (l_total <= 64), the first size past it, powers of two and one more, the store's and the ABI's maximum, and more
queries than compute units."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ("dense", "sparse", "full_text")
WEIGHTS = {"dense": 0.5, "sparse": 0.3, "full_text": 0.2}      # two methods: shares 0.625 / 0.375


def _vs():
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd import vector_stores

    return vector_stores


def _same(got, want, tag=None):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[0].shape == want[0].shape, tag
    assert np.array_equal(got[0], want[0]), tag
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), tag


def _both(lists, top_k, weights=WEIGHTS, rrf_k=60, tag=None):
    vs = _vs()
    want = vs.rrf_merge_rows(lists, top_k, weights, rrf_k)
    _same(vs.rrf_fuse_rows_device(lists, top_k, weights, rrf_k), want, tag)
    return want


def _random_lists(rng, nq, lens, base=0):
    """Per query and method: rows drawn without replacement from one pool of 1.5 x the longest list (the methods overlap
    heavily), about 20 % of the entries -1; query 0 has a hole in the first and the last position of every list."""
    pool = int(1.5 * max(lens)) + 1
    lists = {}
    for m, n in zip(METHODS, lens):
        rows = np.stack([rng.choice(pool, n, replace=False) for _ in range(nq)]).astype(np.int64) + base
        if n >= 3:                   # (shorter lists stay whole: a hole would leave nothing to fuse)
            rows[rng.random((nq, n)) < 0.2] = -1
            rows[0, 0] = rows[0, -1] = -1
        lists[m] = rows
    return lists


def _all_holes(lists, q):
    for rows in lists.values():
        rows[q] = -1


def _few_distinct(lists, q, top_k):
    """Query q keeps top_k - 1 distinct rows (none when top_k == 1): the answer ends in padding."""
    keep = np.unique(np.concatenate([r[q] for r in lists.values()]))
    keep = keep[keep >= 0][: top_k - 1]
    for rows in lists.values():
        rows[q, ~np.isin(rows[q], keep)] = -1


CASES = [(1, (1, 1), 1), (3, (5, 5), 3), (7, (10, 10, 10), 5), (5, (32, 32), 16), (5, (33, 32), 10), (4, (20, 7, 13), 40),
         (2, (128, 128), 128), (2, (129, 128), 64), (2, (1024, 1024, 1024), 512), (1, (2048, 2048), 1024), (301, (10, 10), 5)]
NEAR_2_32 = {(3, (5, 5), 3), (5, (33, 32), 10)}      # ids shifted to end at 2^32 - 1: one case per kernel


# ------------------------------------------------------------------ 1. the reference's own numbers
def test_reference_fixtures_replayed_on_the_device():
    vs = _vs()
    with open(os.path.join(G, "host_fixtures.json")) as f:
        cases = json.load(f)["rrf"]
    assert len(cases) >= 5
    for c in cases:
        by_method = {"dense": c["dense"], "sparse": c["sparse"]}
        if c["full_text"] is not None:
            by_method["full_text"] = c["full_text"]
        number, names, coded = {}, [], {}
        for m, ids in by_method.items():            # ids numbered in first-seen order, as merge_hybrid_results does
            row = np.full((1, len(ids)), -1, np.int64)
            for pos, key in enumerate(ids):
                if key not in number:
                    number[key] = len(names)
                    names.append(key)
                row[0, pos] = number[key]
            coded[m] = row
        rows, dist = vs.rrf_fuse_rows_device(coded, c["top_k"], c["weights"], rrf_k=c["rrf_k"])
        live = rows[0] >= 0
        assert [names[r] for r in rows[0][live]] == c["ids"]
        assert dist[0][live].tolist() == c["distances"]                  # float64, bit-exact
        assert (dist[0][~live] == 0).all()


# ------------------------------------------------------------------ 2. against rrf_merge_rows
@pytest.mark.parametrize("nq,lens,top_k", CASES, ids=[f"{q}x{'+'.join(map(str, ln))}-top{k}" for q, ln, k in CASES])
def test_device_equals_numpy(nq, lens, top_k):
    rng = np.random.default_rng(1000 + nq + sum(lens))
    pool = int(1.5 * max(lens)) + 1
    base = (1 << 32) - pool if (nq, lens, top_k) in NEAR_2_32 else 0
    if nq >= 3:
        lists = _random_lists(rng, nq, lens, base)
        _all_holes(lists, nq - 1)
        _few_distinct(lists, nq - 2, top_k)
        if base:
            assert max(int(r.max()) for r in lists.values()) >= (1 << 32) - 8
        want = _both(lists, top_k, tag="batch")
        assert (want[0][nq - 1] == -1).all() and (want[0][nq - 2] == -1).sum() >= 1
        return
    # one or two queries: the two special queries take query 0 of a batch of their own, same geometry
    lists = _random_lists(rng, nq, lens, base)
    _both(lists, top_k, tag="random")
    lists = _random_lists(rng, nq, lens, base)
    _few_distinct(lists, 0, top_k)
    want = _both(lists, top_k, tag="few distinct rows")
    assert (want[0][0] == -1).sum() >= 1
    lists = _random_lists(rng, nq, lens, base)
    _all_holes(lists, 0)
    want = _both(lists, top_k, tag="no candidate")
    assert (want[0][0] == -1).all() and (want[1][0] == 0).all()


def test_top_k_beyond_the_lists_is_padded_and_empty_batches_make_no_call():
    vs = _vs()
    rng = np.random.default_rng(3)
    lists = _random_lists(rng, 4, (6, 5))
    want = _both(lists, 30, tag="top_k > l_total")
    assert (want[0][:, 11:] == -1).all()
    _both(lists, 3, weights={"dense": 2.0, "sparse": 1.0}, rrf_k=0.5, tag="fractional rrf_k")
    _both(lists, 3, weights={}, tag="no weight on any method: equal shares")
    empty = {"dense": np.zeros((0, 4), np.int64), "sparse": np.zeros((0, 4), np.int64)}
    rows, dist = vs.rrf_fuse_rows_device(empty, 3, WEIGHTS)
    assert rows.shape == (0, 3) and dist.shape == (0, 3)


# ------------------------------------------------------------------ 3. exact ties
@pytest.mark.parametrize("n,top_k", [(10, 6), (40, 20)], ids=["wave", "block"])
def test_exact_ties_keep_first_seen_order(n, top_k):
    a = np.arange(n, dtype=np.int64) + 100
    b = a.reshape(-1, 2)[:, ::-1].reshape(-1)                     # mirrored ranks: A at (0, 1), B at (1, 0), ...
    lists = {"dense": np.stack([a, a]), "sparse": np.stack([b, b])}
    weights = {"dense": 1.0, "sparse": 1.0}
    want = _vs().rrf_merge_rows(lists, top_k, weights)
    d = want[1][0]
    assert (d[0::2] == d[1::2]).all() and len(d) >= 2           # every pair of the expected answer is an exact tie
    assert want[0][0].tolist() == a[:top_k].tolist()              # and the row seen first comes first
    _both(lists, top_k, weights=weights)


# ------------------------------------------------------------------ 4. accumulation order
def test_scores_accumulate_in_method_order():
    vs = _vs()
    rng = np.random.default_rng(7)
    nq, n = 64, 20
    lists = {m: np.stack([rng.choice(24, n, replace=False) for _ in range(nq)]).astype(np.int64) for m in METHODS}
    fwd = vs.rrf_merge_rows(lists, 3 * n, WEIGHTS, 60)
    rev = vs.rrf_merge_rows({m: lists[m] for m in reversed(METHODS)}, 3 * n, WEIGHTS, 60)
    differ = 0
    for q in range(nq):
        back = {int(r): x for r, x in zip(rev[0][q], rev[1][q]) if r >= 0}
        differ += sum(back[int(r)] != x for r, x in zip(fwd[0][q], fwd[1][q]) if r >= 0)
    # the order of the additions shows in the last bit of about a quarter of the scores; 1.0 - score keeps it for few of them
    # (its ulp is 32 times the score's), hence 64 queries: 7 distances of this batch differ
    assert differ > 0
    _both(lists, 3 * n)
    _both(lists, 7)


# ------------------------------------------------------------------ 5. a row twice in one list
@pytest.mark.parametrize("n", [8, 50], ids=["wave", "block"])
@pytest.mark.parametrize("third", [False, True])
def test_duplicates_inside_one_list_are_summed(n, third):
    first = np.arange(n, dtype=np.int64)
    first[5] = first[2]                                           # row 2 at ranks 2 and 5 of the first list
    second = np.arange(n, dtype=np.int64) + n
    if third:
        second[1] = 2
    lists = {"dense": first[None].copy(), "sparse": second[None].copy()}
    want = _both(lists, n)
    assert (want[0][0] == 2).sum() == 1


# ------------------------------------------------------------------ 6. device pointers, a caller's stream
@pytest.mark.parametrize("nq,lens,top_k", [(5, (33, 32), 10), (2, (129, 128), 64)])
def test_device_form_on_a_torch_stream(nq, lens, top_k):
    import torch

    vs = _vs()
    from verbatim_rag_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(21)
    lists = _random_lists(rng, nq, lens)
    want = vs.rrf_fuse_rows_device(lists, top_k, WEIGHTS)
    share = vs.normalize_weights(dict.fromkeys(lists), WEIGHTS)
    cand = np.ascontiguousarray(np.concatenate(list(lists.values()), axis=1))
    gains = np.concatenate([share[m] * (1.0 / (60 + np.arange(r.shape[1], dtype=np.float64) + 1)) for m, r in lists.items()])
    d_rows, d_gains = torch.from_numpy(cand).cuda(), torch.from_numpy(gains).cuda()
    o_rows = torch.full((nq, top_k), -7, dtype=torch.int64, device="cuda")
    o_dist = torch.full((nq, top_k), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    _lib.check("vrag_rrf_fuse", lib.vrag_rrf_fuse(d_rows.data_ptr(), d_gains.data_ptr(), nq, sum(lens), top_k, o_rows.data_ptr(),
                                                  o_dist.data_ptr(), 1, torch.cuda.current_device(), C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    _same((o_rows.cpu().numpy(), o_dist.cpu().numpy()), want)
    assert np.array_equal(d_rows.cpu().numpy(), cand) and np.array_equal(d_gains.cpu().numpy(), gains)    # inputs untouched


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors_report_and_write_nothing():
    from verbatim_rag_amd import _lib

    lib = _lib.load()
    rows = np.arange(4097, dtype=np.int64)[None].copy()
    gains = np.full(4097, 0.01)
    out_r, out_d = np.full(4097, -7, np.int64), np.full(4097, -7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(rows_=rows, gains_=gains, nq=1, l=8, k=4, out_r_=out_r, out_d_=out_d):
        st = lib.vrag_rrf_fuse(p(rows_) if rows_ is not None else None, p(gains_) if gains_ is not None else None, nq, l, k,
                               p(out_r_) if out_r_ is not None else None, p(out_d_) if out_d_ is not None else None, 0, 0, None)
        return st, _lib.last_error()

    assert call()[0] == 0 and out_r[:4].tolist() == [0, 1, 2, 3]           # the well-formed call these are variations of
    out_r[:], out_d[:] = -7, -7.0
    for kw, text in ((dict(l=4097, k=4), "l_total"), (dict(k=0), "top_k"), (dict(l=8, k=9), "top_k"), (dict(rows_=None), "null"),
                     (dict(gains_=None), "null"), (dict(out_r_=None), "null"), (dict(out_d_=None), "null"), (dict(nq=0), "nq")):
        st, msg = call(**kw)
        assert st == -1 and text in msg and "vrag_rrf_fuse" in msg, (kw, st, msg)
    big = rows.copy()
    big[0, 3] = 1 << 32
    st, msg = call(rows_=big)
    assert st == -1 and "row id 4294967296" in msg
    big[0, 3] = (1 << 32) - 1                                              # the largest id the contract admits
    assert call(rows_=big)[0] == 0 and out_r[3] == (1 << 32) - 1
    out_r[:], out_d[:] = -7, -7.0
    for bad in (-0.25, np.inf, np.nan):
        g = gains.copy()
        g[5] = bad
        st, msg = call(gains_=g)
        assert st == -1 and "gain 5" in msg, (bad, msg)
    assert (out_r == -7).all() and (out_d == -7.0).all()                   # no failed call wrote anything
    with pytest.raises(_lib.VragError, match="l_total"):
        _vs().rrf_fuse_rows_device({"dense": np.zeros((1, 4097), np.int64)}, 3, {"dense": 1.0})


# ------------------------------------------------------------------ 8. the store option
N, DIM, VOCAB, NQ = 2000, 64, 512, 64


def _store_rows(rng, ids):
    n = len(ids)
    dense = (rng.integers(0, 2, (n, DIM)) * 2 - 1).astype(np.float32) / np.float32(np.sqrt(DIM))
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 12, replace=False), rng.integers(1, 64, 12) / 64)} for _ in range(n)]
    texts = [f"row {i} topic{i % 37} shared words" for i in range(n)]
    metas = [{"document_id": f"d{i % 50}", "half": i % 2, "n": i} for i in range(n)]
    return dense, sparse, texts, metas


def _dump(per_q):
    return [[(r.id, r.score, r.text, r.enhanced_text, sorted(r.metadata.items())) for r in rs] for rs in per_q]


def _pair_of_stores(ids, seed):
    from verbatim_rag_amd.vector_stores import GpuVectorStore

    dense, sparse, texts, metas = _store_rows(np.random.default_rng(seed), ids)
    stores = []
    for route in ("host", "device"):
        st = GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, enable_full_text=True, rrf_route=route)
        st.add_vectors(ids, dense, sparse, texts, [f"enh {i}" for i in range(len(ids))], metas)
        st.delete([ids[i] for i in (3, 500, 501, 1999)])
        stores.append(st)
    picks = np.random.default_rng(seed + 1).choice(len(ids), NQ, replace=False)
    queries = dict(dense_queries=[dense[i].tolist() for i in picks], sparse_queries=[sparse[i] for i in picks],
                   text_queries=[f"topic{i % 37} shared" for i in picks])
    return stores[0], stores[1], queries


def _close(st):
    if st._dense is not None:
        st._dense.close()
    for shard, _base, _n in st._sparse_parts:
        shard.close()
    if st._text is not None:
        st._text.close()
    for parts, _rows_, _dev in list(st._subsets.values()):
        for shard, _base in parts:
            shard.close()


@pytest.fixture()
def fused(monkeypatch):
    """Every call of `rrf_fuse_rows_device` the store makes (it keeps working): (methods, columns per method, error)."""
    vs = _vs()
    real, calls = vs.rrf_fuse_rows_device, []

    def recorder(rows_by_method, *a, **kw):
        calls.append([list(rows_by_method), [r.shape[1] for r in rows_by_method.values()], None])
        try:
            return real(rows_by_method, *a, **kw)
        except Exception as e:      # query_batch answers a failed default batch per query: a failure must not pass unseen
            calls[-1][2] = e
            raise

    monkeypatch.setattr(vs, "rrf_fuse_rows_device", recorder)
    return calls


def test_store_device_route_equals_host_route(fused):
    host, dev, q = _pair_of_stores([f"id{i}" for i in range(N)], 31)
    three = {"dense": 0.5, "sparse": 0.3, "full_text": 0.2}
    cases = [dict(dense_queries=q["dense_queries"], sparse_queries=q["sparse_queries"], search_type="hybrid", top_k=5),
             dict(top_k=4, hybrid_weights=three, **q), dict(top_k=4, hybrid_weights=three, filter='metadata["half"] == 1', **q)]
    try:
        assert host.rrf_route == "host" and dev.rrf_route == "device" and dev._all_ids_truthy
        assert NQ >= dev.RRF_DEVICE_MIN_QUERIES                                  # a batch the device route takes
        for n_case, kw in enumerate(cases):
            want = host.query_batch(**kw)
            assert not fused                                                  # the default route stays on the host
            got = dev.query_batch(**kw)
            methods = ["dense", "sparse"] if n_case == 0 else ["dense", "sparse", "full_text"]
            assert fused == [[methods, [2 * kw["top_k"]] * len(methods), None]], n_case
            fused.clear()
            assert len(got) == NQ and all(len(g) == kw["top_k"] for g in got)
            assert _dump(got) == _dump(want), n_case                          # ids equal, scores == as float64
            rest = {k: v for k, v in kw.items() if not k.endswith("_queries")}
            singles = [dev.query(dense_query=kw["dense_queries"][i], sparse_query=kw["sparse_queries"][i],
                                 text_query=kw.get("text_queries", [None] * NQ)[i], **rest) for i in range(NQ)]
            assert _dump(singles) == _dump(got), n_case
            assert not fused                                                  # `query` fuses on the host
    finally:
        _close(host), _close(dev)


def test_store_with_a_falsy_id_takes_the_per_query_path_on_both_routes(fused):
    host, dev, q = _pair_of_stores([f"id{i}" if i != 17 else "" for i in range(N)], 33)
    try:
        assert not dev._all_ids_truthy and not host._all_ids_truthy
        kw = dict(dense_queries=q["dense_queries"], sparse_queries=q["sparse_queries"], search_type="hybrid", top_k=5)
        assert _dump(dev.query_batch(**kw)) == _dump(host.query_batch(**kw))
        assert not fused
    finally:
        _close(host), _close(dev)
