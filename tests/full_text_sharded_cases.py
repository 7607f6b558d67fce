"""Shared by the sharded full-text tests: one scripted session against a `GpuVectorStore(enable_full_text=True)` -- uneven
insert batches (a single row, so one rank's share is empty; a store of fewer rows than ranks; a tail segment and a fold),
single / batched / long / filtered queries, deletes, the three-leg weighted hybrid search, save / load -- whose transcript
must not depend on how the rows are sharded, and the same transcript from the host restatement (tests/full_text_oracle.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import full_text_oracle as O  # noqa: E402

N, DIM, VOCAB = 3000, 64, 300
CUTS = [0, 1, 2, 1200, 1201, 1250, N]      # batches of 1 (fewer rows than ranks), 1, 1198, 1, 49 (a tail segment), 1750 (a fold)
QUERY_AT = (1, 1200, 1250, N)              # row counts at which the store is queried while it grows
TAIL_MIN = 100
FILTER, FILTER_NONE = 'metadata["g"] == 1', 'metadata["g"] == 7'
WEIGHTS = {"dense": 0.5, "sparse": 0.3, "full_text": 0.2}
ORACLE_KEYS = tuple(f"n{b}" for b in QUERY_AT) + ("one", "batch70", "k100", "k100_one", "filter", "filter_none", "deleted",
                                                   "deleted_filter", "reload", "reload_world1")


def corpus():
    texts, words, _flat, _lens = O.zipf_corpus(N, vocab=400, mean_len=12, seed=21)
    rng = np.random.default_rng(21)
    # dyadic dense rows of norm 4 and dyadic sparse weights: the dense / sparse scores of the hybrid legs are exact sums, so
    # they do not depend on how a shard's kernel orders them
    dense = np.where(rng.random((N, DIM)) < 0.5, 0.5, -0.5).astype(np.float32)
    dense[:, 0] = 0.5
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(VOCAB, 8, replace=False), rng.integers(1, 64, 8) / 64)} for _ in range(N)]
    return texts, words, dense, sparse


def queries(words):
    rng = np.random.default_rng(5)
    out = []
    for i in range(70):                                            # more than 64: a batch beyond one merge pass of queries
        picks = [words[int(j)] for j in rng.zipf(1.3, size=int(rng.integers(1, 5))) if j < len(words)] or [words[1]]
        if i % 5 == 0:
            picks.append(picks[0].upper())                          # a repeated term
        if i % 7 == 0:
            picks.append("qqqzzzunknownterm")                        # held by no shard: df = 0 everywhere
        if i % 11 == 0:
            picks.append("COMMON")
        out.append(" ".join(picks) + "?")
    out[0] = f"common {words[3]} {words[7]}"
    return out


def pack(result_lists, k):
    """`SearchResult` lists -> (`ids [Q, k]` int64 row numbers from the "id<row>" strings, -1 padded; `scores [Q, k]` float64,
    -inf padded: fp32 scores widen exactly)."""
    ids = np.full((len(result_lists), k), -1, np.int64)
    scores = np.full((len(result_lists), k), -np.inf, np.float64)
    for q, res in enumerate(result_lists):
        assert len(res) <= k
        for j, r in enumerate(res):
            ids[q, j] = int(r.id[2:])
            scores[q, j] = r.score
    return ids, scores


def _pack_oracle(hits, k):
    ids = np.full((len(hits), k), -1, np.int64)
    scores = np.full((len(hits), k), -np.inf, np.float64)
    for q, (rows, sc) in enumerate(hits):
        ids[q, : len(rows)] = rows
        scores[q, : len(rows)] = sc.astype(np.float64)
    return ids, scores


def oracle_session():
    """The full-text entries of `session` from the host restatement."""
    texts, words, _dense, _sparse = corpus()
    qs = queries(words)
    keys = [O.term_keys(t) for t in texts]
    qk = [O.term_keys(q) for q in qs]
    out = {}
    for b in QUERY_AT:
        o = O.Bm25Oracle(keys[:b])
        out[f"n{b}"] = _pack_oracle([o.search(k_, 5) for k_ in qk[:4]], 5)
    o = O.Bm25Oracle(keys)
    out["one"] = _pack_oracle([o.search(qk[0], 7)], 7)
    out["batch70"] = _pack_oracle([o.search(k_, 5) for k_ in qk], 5)
    out["k100"] = _pack_oracle([o.search(k_, 100) for k_ in qk[:3]], 100)
    out["k100_one"] = _pack_oracle([o.search(qk[0], 100)], 100)
    g1 = np.arange(N) % 3 == 1
    out["filter"] = _pack_oracle([o.search(k_, 10, g1) for k_ in qk[:3]], 10)
    out["filter_none"] = _pack_oracle([o.search(qk[0], 10, np.zeros(N, dtype=bool))], 10)
    live = np.ones(N, dtype=bool)
    live[::4] = False
    o.set_live(live)                                               # N / avgdl / df follow the deletes
    out["deleted"] = _pack_oracle([o.search(k_, 6) for k_ in qk[:8]], 6)
    out["deleted_filter"] = _pack_oracle([o.search(k_, 6, g1) for k_ in qk[:3]], 6)
    out["reload"] = out["reload_world1"] = out["deleted"]
    return out


def session(comm, payload, tmp, world1_dir=None):
    """Runs the scripted session; returns (transcript, checks, directory this store was saved to).  `world1_dir`: a store
    saved by a single-rank session, loaded here at this comm's world size."""
    from verbatim_rag_amd import vector_stores as vs

    texts, words, dense, sparse = corpus()
    qs = queries(words)
    st = vs.GpuVectorStore(dense_dim=DIM, sparse_vocab=VOCAB, enable_full_text=True, comm=comm, payload=payload)
    st.TEXT_TAIL_MIN = TAIL_MIN
    world = comm.world if comm is not None else 1
    out, checks, segments = {}, {}, []
    ft = dict(search_type="full_text")
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        st.add_vectors([f"id{i}" for i in range(a, b)], dense[a:b], sparse[a:b], texts[a:b], [f"enh {i}" for i in range(a, b)],
                       [{"g": i % 3} for i in range(a, b)])
        if b in QUERY_AT:
            out[f"n{b}"] = pack([st.query(text_query=q, top_k=5, **ft) for q in qs[:4]], 5)
            segments.append(st._text.stats()["segments"] if st._text is not None else 0)
    # 1 row: the rank that holds it has one segment; 1200: folded; 1250: a tail behind the main segment; 3000: folded again
    checks["tail_then_fold"] = segments[1:] == [1, 2, 1] and segments[0] in ((1,) if world == 1 else (0, 1))
    out["one"] = pack([st.query(text_query=qs[0], top_k=7, **ft)], 7)
    out["batch70"] = pack(st.query_batch(text_queries=qs, top_k=5, **ft), 5)
    out["k100"] = pack(st.query_batch(text_queries=qs[:3], top_k=100, **ft), 100)
    out["k100_one"] = pack([st.query(text_query=qs[0], top_k=100, **ft)], 100)
    out["filter"] = pack([st.query(text_query=q, top_k=10, filter=FILTER, **ft) for q in qs[:3]], 10)
    out["filter_none"] = pack([st.query(text_query=qs[0], top_k=10, filter=FILTER_NONE, **ft)], 10)
    st.delete([f"id{i}" for i in range(0, N, 4)])
    out["deleted"] = pack(st.query_batch(text_queries=qs[:8], top_k=6, **ft), 6)
    out["deleted_filter"] = pack(st.query_batch(text_queries=qs[:3], top_k=6, filter=FILTER, **ft), 6)
    # the three-leg weighted hybrid search against merge_hybrid_results of the per-method lists, the full-text list being the oracle's
    live = np.ones(N, dtype=bool)
    live[::4] = False
    oracle = O.Bm25Oracle([O.term_keys(t) for t in texts])
    oracle.set_live(live)
    k = 6
    ok = True
    for i in (3, 17):
        dq, sq, tq = dense[i].tolist(), sparse[i], f"{words[5]} common {words[i]}"
        alive = st._mask(None)                                     # the rows left after the deletes
        rbm = {"dense": st._search("dense", dq, 2 * k, alive), "sparse": st._search("sparse", sq, 2 * k, alive),
               "full_text": [{"id": f"id{r}", "distance": float(s), "_row": int(r)} for r, s in zip(*oracle.search(O.term_keys(tq), 2 * k))]}
        want = [(h["id"], h["distance"]) for h in vs.merge_hybrid_results(rbm, k, WEIGHTS, 60)]
        one = st.query(dense_query=dq, sparse_query=sq, text_query=tq, top_k=k, hybrid_weights=WEIGHTS)
        batch = st.query_batch(dense_queries=[dq, dq], sparse_queries=[sq, sq], text_queries=[tq, tq], top_k=k, hybrid_weights=WEIGHTS)
        ok = ok and all([(r.id, r.score) for r in got] == want for got in (one, batch[0], batch[1]))
        out[f"hybrid{i}"] = pack([one, batch[0], batch[1]], k)
    checks["hybrid_equals_merge_of_per_method_lists"] = ok
    saved = os.path.join(tmp, f"store_w{world}_{payload}")
    st.save(saved)
    back = vs.GpuVectorStore.load(saved, comm=comm, payload=payload)
    checks["reload_full_text_on"] = bool(back.enable_full_text and len(back) == int(live.sum()))
    out["reload"] = pack(back.query_batch(text_queries=qs[:8], top_k=6, **ft), 6)
    back.close()
    if world1_dir is not None:
        back = vs.GpuVectorStore.load(world1_dir, comm=comm, payload=payload)
        out["reload_world1"] = pack(back.query_batch(text_queries=qs[:8], top_k=6, **ft), 6)
        back.close()
    else:
        out["reload_world1"] = out["reload"]
    st.close()
    return out, checks, saved


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


class ShardOracle(O.Bm25Oracle):
    """A shard's rows scored with the corpus-wide statistics and caller-given weights: the host statement of what
    `vrag_text_index_set_corpus_stats` makes the device do.  The one restatement both sharded test files use."""

    def set_corpus(self, n_live_total: int, sum_dl_total: int) -> None:
        self.N = n_live_total
        self.avgdl = np.float32(sum_dl_total / n_live_total) if n_live_total else np.float32(0)   # fp32(float64 / float64)
        if self.avgdl > 0:
            self.kd = self.k1 * ((np.float32(1) - self.b) + self.b * (self.dl.astype(np.float32) / self.avgdl))
        else:
            self.kd = np.full(self.n, self.k1, np.float32)

    def search_weighted(self, keys, w, k, allow=None):
        """(rows, scores) for (ascending keys, fp32 weights): score > 0, live, allowed (rows beyond `allow` are not)."""
        acc = np.zeros(self.n, np.float32)
        k1p1 = self.k1 + np.float32(1)
        for key, wt in zip(np.asarray(keys).tolist(), np.asarray(w).tolist()):
            rows, tf = self.postings(key)
            if len(rows):
                tff = tf.astype(np.float32)
                acc[rows] = acc[rows] + np.float32(wt) * ((tff * k1p1) / (tff + self.kd[rows]))
        ok = (acc > 0) & self.live
        if allow is not None:
            known = np.zeros(self.n, dtype=bool)
            known[: len(allow)] = np.asarray(allow, dtype=bool)[: self.n]
            ok &= known
        rows = np.nonzero(ok)[0]
        order = np.lexsort((rows, -acc[rows]))[:k]
        return rows[order], acc[rows[order]]


class CpuTextIndex:
    """Stand-in for `TextIndex` on boxes without a GPU (tests only): the same interface answered by `ShardOracle`, with the
    segment bookkeeping of `vrag_text_index_add`."""

    weights = staticmethod(lambda counts, df, n_live: (counts.astype(np.float64) * np.log(
        1.0 + (float(n_live) - df.astype(np.float64) + 0.5) / (df.astype(np.float64) + 0.5))).astype(np.float32))   # TextIndex.weights

    def __init__(self, k1=1.2, b=0.75, device=0):
        self.k1, self.b = k1, b
        self.rows, self.live, self.corpus, self.segments, self._o = [], np.zeros(0, dtype=bool), (0, 0), 0, None

    def add(self, texts, fold):
        self.rows += [O.term_keys(t) for t in texts]
        self.live = np.concatenate([self.live, np.ones(len(texts), dtype=bool)])
        self.segments = 1 if (fold or self.segments == 0) else 2
        self._o = None

    def set_live(self, alive):
        self.live = np.asarray(alive, dtype=bool).copy()
        self._o = None

    def set_corpus_stats(self, n_live_total, sum_dl_total):
        self.corpus = (int(n_live_total), int(sum_dl_total))
        self._o = None

    def _oracle(self):
        if self._o is None:
            self._o = ShardOracle(self.rows, self.k1, self.b)
            self._o.set_live(self.live)
            if self.corpus[0]:
                self._o.set_corpus(*self.corpus)
        return self._o

    def stats(self):
        own = O.Bm25Oracle(self.rows, self.k1, self.b)
        return {"rows": len(self.rows), "live": int(self.live.sum()), "sum_dl": int(own.dl[self.live].sum()) if len(self.rows) else 0,
                "segments": self.segments, "postings": len(own.p_row)}

    def query_terms(self, queries):
        o = self._oracle()
        indptr, keys, counts, df = [0], [], [], []
        for text in queries:
            k_, c_ = np.unique(np.asarray(O.term_keys(text), dtype=np.uint64), return_counts=True)
            keys += k_.tolist()
            counts += c_.tolist()
            df += [o.df(int(x)) for x in k_]
            indptr.append(len(keys))
        return np.asarray(indptr, np.int64), np.asarray(keys, np.uint64), np.asarray(counts, np.int32), np.asarray(df, np.int64), o.N

    def _score(self, indptr, keys, w, k, allow):
        o = self._oracle()
        Q = len(indptr) - 1
        scores = np.full((Q, k), -np.inf, np.float32)
        ids = np.full((Q, k), -1, np.int64)
        for q in range(Q):
            rows, sc = o.search_weighted(keys[indptr[q]:indptr[q + 1]], w[indptr[q]:indptr[q + 1]], k, allow)
            ids[q, : len(rows)] = rows
            scores[q, : len(rows)] = sc
        return scores, ids

    def search_sharded(self, queries, k, allow, n_live_total, sum_df, device_out=None):
        assert device_out is None
        indptr, keys, counts, df, _n = self.query_terms(queries)
        w = self.weights(counts, np.asarray(sum_df(df), dtype=np.int64), n_live_total)
        return self._score(indptr, keys, w, k, allow)

    def search(self, queries, k, allow=None):
        indptr, keys, counts, df, n_live = self.query_terms(queries)
        return self._score(indptr, keys, self.weights(counts, df, n_live), k, allow)

    def close(self):
        pass
