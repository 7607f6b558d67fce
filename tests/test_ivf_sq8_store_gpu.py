"""`GpuVectorStore(dense_dtype="int8", index_type="IVF_SQ8")` through `query` / `query_batch`: with nprobe >= nlist it returns the
FLAT int8 store's ids and score bits (dense and hybrid); with a small nprobe every hit carries its row's SQ8 score in (score desc,
row asc) order; lists over 64 rows and filtered queries left short are answered FLAT-exactly; `compact()` remaps the overlay;
save / load keeps the index settings and the answers; small stores stay FLAT; grouping is refused.

Data: 6000 x 64 rows in 32 clusters, every entry +-1/8 (a cluster's sign pattern with a tenth of the signs flipped): unit length in
fp32, so the store's normalisation changes nothing, every code is +-127 and every scale 1 / (8 * 127) in fp32 -- tests/sq8_ref.py
over the rows as given states the score every route must return, and ties are frequent."""
import json
import os

import numpy as np
import pytest

import sq8_ref as R

pytestmark = pytest.mark.gpu

N, DIM, VOCAB, NLIST, CLUSTERS = 6000, 64, 2000, 64, 32
ALL = ({"nprobe": NLIST}, {"params": {"nprobe": NLIST + 9}})


def _rows(rng, n, first, centres):
    flip = rng.random((n, DIM)) < 0.1
    dense = (centres[rng.integers(0, CLUSTERS, n)] * np.where(flip, -1, 1)).astype(np.float32) / np.float32(np.sqrt(DIM))
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 12, replace=False), rng.integers(1, 64, 12) / 64)} for _ in range(n)]
    ids = [f"id{i}" for i in range(first, first + n)]
    texts = [f"row {i}" for i in range(first, first + n)]
    metas = [{"document_id": f"d{i % 500}", "half": i % 2, "n": i} for i in range(first, first + n)]
    return ids, dense, sparse, texts, metas


def _close(st):
    if st is None:
        return
    if st._dense is not None:
        st._dense.close()
    for shard, _base, _n in st._sparse_parts:
        shard.close()
    for parts, _rows_, _dev in list(st._subsets.values()):
        for shard, _base in parts:
            shard.close()


def _dump(per_q):
    return [[(r.id, np.float32(r.score).view(np.uint32).item(), r.text, sorted(r.metadata.items())) for r in rs] for rs in per_q]


def _check_flat_scores_and_order(results, ref_scores, picks):
    """Every hit's score is its row's SQ8 score against the query (the FLAT store's, bit for bit); (score desc, row asc) order."""
    for rs, q in zip(results, picks):
        rows = np.array([int(r.id[2:]) for r in rs])
        scores = np.array([r.score for r in rs], np.float32)
        assert np.array_equal(scores.view(np.uint32), ref_scores[q, rows].view(np.uint32))
        assert all((scores[j] > scores[j + 1]) or (scores[j] == scores[j + 1] and rows[j] < rows[j + 1]) for j in range(len(rs) - 1))


def test_ivf_sq8_store(tmp_path):
    from verbatim_rag_amd.vector_stores import GpuVectorStore, Sq8Shard, ivf_effective_nlist

    rng = np.random.default_rng(29)
    centres = rng.integers(0, 2, (CLUSTERS, DIM)) * 2 - 1
    ids, dense, sparse, texts, metas = _rows(rng, N, 0, centres)
    kw = dict(dense_dim=DIM, sparse_vocab=VOCAB, dense_dtype="int8")
    flat = GpuVectorStore(**kw)
    ivf = GpuVectorStore(index_type="IVF_SQ8", nlist=NLIST, nprobe=4, **kw)
    small = GpuVectorStore(index_type="IVF_SQ8", nlist=NLIST, **kw)
    loaded = survivors = None
    try:
        for st in (flat, ivf):
            st.add_vectors(ids, dense, sparse, texts, [""] * N, metas)
        small.add_vectors(ids[:1000], dense[:1000], sparse[:1000], texts[:1000], [""] * 1000, metas[:1000])
        picks = [int(i) for i in rng.choice(N, 20, replace=False)]
        dq, sq = [dense[i].tolist() for i in picks], [sparse[i] for i in picks]
        cr, sr = R.quantize(dense)
        ref = R.scores(cr[picks], sr[picks], cr, sr)             # [query, row]: the rows are unit length, a query is its row
        stats = ivf.ivf_stats()
        assert flat.ivf_stats() is None and stats is not None and isinstance(ivf._dense, Sq8Shard) and ivf._dense.ivf is not None
        assert stats["nlist"] == ivf_effective_nlist(N, NLIST) == NLIST and stats["rows"] == stats["trained_rows"] == N
        assert 0 < stats["largest_list"] < N

        # nprobe >= nlist, both spellings: the FLAT int8 store's results, whole
        cases = [dict(dense_queries=dq, search_type="dense", top_k=5), dict(dense_queries=dq, search_type="dense", top_k=64),
                 dict(dense_queries=dq, sparse_queries=sq, search_type="hybrid", top_k=5),
                 dict(dense_queries=dq, sparse_queries=sq, top_k=7, hybrid_weights={"dense": 0.7, "sparse": 0.3})]
        for case in cases:
            want = _dump(flat.query_batch(**case))
            for params in ALL:
                assert _dump(ivf.query_batch(search_params=params, **case)) == want, (case["top_k"], params)
        for i in (0, 19):
            for one in (dict(dense_query=dq[i], search_type="dense", top_k=5), dict(dense_query=dq[i], sparse_query=sq[i], top_k=5)):
                for params in ALL:
                    assert _dump([ivf.query(search_params=params, **one)]) == _dump([flat.query(**one)]), (i, params)
        _check_flat_scores_and_order(flat.query_batch(dense_queries=dq, search_type="dense", top_k=64), ref, range(len(picks)))

        # nprobe = 4 (the store's own) and 2: the FLAT score of every row it found, sorted; the overlay is what answers
        for params in (None, {"nprobe": 2}):
            got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params=params)
            _check_flat_scores_and_order(got, ref, range(len(picks)))
            assert all(len(rs) == 10 and rs[0].score == ref[q, picks[q]] for q, rs in enumerate(got))
        overlay, unit = ivf._dense.ivf, np.asarray(dq, np.float32)
        sc, rows_ = overlay.search(unit, 10, 4)
        got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=10)
        assert [[(r.id, r.score) for r in rs] for rs in got] == \
            [[(f"id{r}", float(v)) for r, v in zip(rr, ss) if r >= 0] for rr, ss in zip(rows_.tolist(), sc.tolist())]
        two = _dump(ivf.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params={"nprobe": 2}))

        # answered FLAT-exactly: lists over 64 rows, and a filter that leaves the IVF answer short
        assert _dump(ivf.query_batch(dense_queries=dq, search_type="dense", top_k=70, search_params={"nprobe": 1})) == \
            _dump(flat.query_batch(dense_queries=dq, search_type="dense", top_k=70))
        flt = 'metadata["document_id"] == "d41"'                  # 12 rows pass
        got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter=flt, search_params={"nprobe": 1})
        assert _dump(got) == _dump(flat.query_batch(dense_queries=dq, search_type="dense", top_k=5, filter=flt))
        assert all(len(rs) == 5 and all(r.metadata["document_id"] == "d41" for r in rs) for rs in got)

        # grouping is refused as it is for IVF_FLAT
        with pytest.raises(ValueError, match="grouping search .*index_type='IVF_SQ8'"):
            ivf.query(dense_query=dq[0], search_type="dense", top_k=3, search_params={"group_by_field": "document_id"})

        # under IVF_MIN_ROWS rows: FLAT
        assert small.ivf_stats() is None
        assert _dump(small.query_batch(dense_queries=dq, search_type="dense", top_k=5, search_params={"nprobe": 1})) == \
            _dump(small.query_batch(dense_queries=dq, search_type="dense", top_k=5))

        # save / load keeps the settings and, training being deterministic, the answers
        ivf.save(str(tmp_path / "ivf"))
        head = json.load(open(os.path.join(tmp_path, "ivf", "store.json")))
        assert (head["index_type"], head["dense_dtype"], head["nlist"], head["nprobe"]) == ("IVF_SQ8", "int8", NLIST, 4)
        loaded = GpuVectorStore.load(str(tmp_path / "ivf"))
        assert (loaded.index_type, loaded.dense_dtype, loaded.nlist, loaded.nprobe) == ("IVF_SQ8", "int8", NLIST, 4)
        assert loaded.ivf_stats() == ivf.ivf_stats()
        assert _dump(loaded.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params={"nprobe": 2})) == two

        # rows deleted, then compact(): the overlay is remapped; nprobe >= nlist equals a FLAT int8 store built from the survivors
        gone = [f"id{i}" for i in range(0, N, 3)]
        ivf.delete(gone)
        assert ivf.compact() == len(gone)
        keep = np.ones(N, bool)
        keep[::3] = False
        at = np.nonzero(keep)[0]
        stats = ivf.ivf_stats()
        assert stats["rows"] == len(at) and stats["trained_rows"] == N and stats["nlist"] == NLIST
        survivors = GpuVectorStore(**kw)
        survivors.add_vectors([ids[i] for i in at], dense[at], [sparse[i] for i in at], [texts[i] for i in at], [""] * len(at), [metas[i] for i in at])
        for case in cases[:3]:
            assert _dump(ivf.query_batch(search_params=ALL[0], **case)) == _dump(survivors.query_batch(**case)), case["top_k"]
        got = ivf.query_batch(dense_queries=dq, search_type="dense", top_k=10, search_params={"nprobe": 4})
        _check_flat_scores_and_order(got, ref, range(len(picks)))
        assert not {r.id for rs in got for r in rs} & set(gone)
    finally:
        for st in (flat, ivf, small, loaded, survivors):
            _close(st)
