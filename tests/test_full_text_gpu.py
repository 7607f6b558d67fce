"""Full-text (BM25) search on the device (csrc/fulltext.hip, GpuVectorStore(enable_full_text=True)) against the host
restatement in tests/full_text_oracle.py: term keys, ids and fp32 scores equal bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import full_text_oracle as O  # noqa: E402

import verbatim_rag_amd  # noqa: F401,E402
from verbatim_rag_amd import vector_stores as vs  # noqa: E402
from verbatim_rag_amd.index import HotPathIndex  # noqa: E402

pytestmark = pytest.mark.gpu


def _check_tokens(texts):
    counts, keys = vs.tokenize_keys(texts)
    want = [O.term_keys(t) for t in texts]
    assert counts.tolist() == [len(w) for w in want]
    assert keys.tolist() == [k for w in want for k in w]


def test_tokenizer_matches_the_oracle():
    _check_tokens(O.EDGE_STRINGS)
    _check_tokens(["Hello, World! hello-WORLD", "İstanbul ΣΑΣ a_b ½x Straße ǅemal", "x" * 5000, "9 ½ ² ① ٣", "été"])
    rng = np.random.default_rng(1)
    texts = [O.random_unicode_text(rng, int(rng.integers(0, 200))) for _ in range(3000)]
    _check_tokens(texts)


def test_tokenizer_one_megabyte_documents():
    rng = np.random.default_rng(2)
    big = O.random_unicode_text(rng, 520_000)
    assert len(big.encode("utf-8")) > 1 << 20
    one_token = "Ab" * (1 << 19)                                   # a single 1 MB token
    _check_tokens(["a b", big, "tail", one_token, ""])


@pytest.fixture(scope="module")
def zipf():
    texts, words, flat_keys, lens = O.zipf_corpus(200_000, seed=3)
    ix = vs.TextIndex()
    ix.add(texts, fold=True)
    oracle = O.Bm25Oracle.from_arrays(flat_keys, lens)
    yield texts, words, ix, oracle
    ix.close()


def _queries(words, n, rng):
    out = []
    for i in range(n):
        picks = [words[int(j)] for j in rng.zipf(1.3, size=int(rng.integers(1, 6))) if j < len(words)] or [words[1]]
        if i % 5 == 0:
            picks.append(picks[0].upper())                       # a repeated term (count 2)
        if i % 7 == 0:
            picks.append("qqqzzzunknownterm")                     # unknown: contributes nothing
        if i % 11 == 0:
            picks.append("COMMON")                                # present in nearly every row
        out.append(" ".join(picks) + "?")
    return out


def _assert_batch(ix, oracle, queries, k, allow=None):
    scores, ids = ix.search(queries, k, allow)
    for q, text in enumerate(queries):
        rows, sc = oracle.search(O.term_keys(text), k, allow)
        m = len(rows)
        np.testing.assert_array_equal(ids[q, :m], rows, err_msg=f"query {q} {text!r} k={k}")
        np.testing.assert_array_equal(scores[q, :m], sc, err_msg=f"query {q} {text!r} k={k}")
        assert (ids[q, m:] == -1).all() and np.isneginf(scores[q, m:]).all()


@pytest.mark.parametrize("nq", [1, 7, 256])
def test_search_equals_the_oracle(zipf, nq):
    texts, words, ix, oracle = zipf
    rng = np.random.default_rng(nq)
    queries = _queries(words, nq, rng)
    for k in (1, 5, 64, 1024):
        _assert_batch(ix, oracle, queries, k)


def test_search_edge_queries(zipf):
    texts, words, ix, oracle = zipf
    scores, ids = ix.search(["qqqzzzunknownterm", "", "...", "common"], 5)
    assert (ids[:3] == -1).all()
    rows, sc = oracle.search(O.term_keys("common"), 5)
    assert ids[3].tolist() == rows.tolist() and scores[3].tolist() == sc.tolist()
    _assert_batch(ix, oracle, ["common common COMMON", "Common " + words[2] + " " + words[2]], 1024)
    st = ix.stats()
    assert st["rows"] == len(texts) and st["live"] == len(texts) and st["segments"] == 1


def test_liveness_and_allow_bitmap(zipf):
    texts, words, ix, oracle = zipf
    rng = np.random.default_rng(9)
    live = rng.random(len(texts)) > 0.3
    allow = rng.random(len(texts)) > 0.5
    try:
        ix.set_live(live)
        oracle.set_live(live)
        queries = _queries(words, 7, rng)
        _assert_batch(ix, oracle, queries, 64, allow)
        _assert_batch(ix, oracle, queries, 300)
    finally:
        ix.set_live(np.ones(len(texts), dtype=bool))
        oracle.set_live(np.ones(len(texts), dtype=bool))


# ------------------------------------------------------------------------------------------ the store
def _corpus(n, seed, dim=64, vocab=300):
    texts, words, flat_keys, lens = O.zipf_corpus(n, vocab=400, mean_len=12, seed=seed)
    rng = np.random.default_rng(seed)
    dense = rng.standard_normal((n, dim)).astype(np.float32)
    sparse = [{int(t): float(v) for t, v in zip(rng.choice(vocab, 8, replace=False), rng.integers(1, 64, 8) / 64)} for _ in range(n)]
    return texts, words, dense, sparse


def _store(texts, dense, sparse, **kw):
    st = vs.GpuVectorStore(dense_dim=dense.shape[1], sparse_vocab=300, enable_full_text=True, **kw)
    n = len(texts)
    st.add_vectors([f"id{i}" for i in range(n)], dense, sparse, texts, [f"enh {i}" for i in range(n)],
                   [{"g": i % 3} for i in range(n)])
    return st


def _oracle_of(texts, live=None):
    o = O.Bm25Oracle([O.term_keys(t) for t in texts])
    if live is not None:
        o.set_live(live)
    return o


def _expect(st, oracle, query, k, allow=None):
    rows, sc = oracle.search(O.term_keys(query), k, allow)
    return [(st._ids[r], float(s)) for r, s in zip(rows.tolist(), sc.tolist())]


def _got(results):
    return [(r.id, r.score) for r in results]


def test_store_query_and_query_batch():
    texts, words, dense, sparse = _corpus(3000, 5)
    st = _store(texts, dense, sparse)
    oracle = _oracle_of(texts)
    qs = [f"{words[1]} {words[7]}", f"common {words[3]}", words[20].upper(), "nothing-like-this-zz"]
    for q in qs:
        assert _got(st.query(text_query=q, top_k=7, search_type="full_text")) == _expect(st, oracle, q, 7)
    assert [_got(r) for r in st.query_batch(text_queries=qs, top_k=7, search_type="full_text")] == [_expect(st, oracle, q, 7) for q in qs]
    r = st.query(text_query="", top_k=3, search_type="full_text")                # empty text: the filter-only query
    assert [x.id for x in r] == ["id0", "id1", "id2"]


def test_store_filter_and_deletes():
    texts, words, dense, sparse = _corpus(3000, 6)
    st = _store(texts, dense, sparse)
    dead = [f"id{i}" for i in range(0, 3000, 4)]
    st.query(text_query="common", top_k=3, search_type="full_text")             # statistics before the delete
    st.delete(dead)
    live = np.ones(3000, dtype=bool)
    live[::4] = False
    oracle = _oracle_of(texts, live)                                            # df / N / avgdl over the live rows
    g1 = np.arange(3000) % 3 == 1
    for q in (f"{words[2]} {words[9]}", "common", words[40]):
        got = _got(st.query(text_query=q, top_k=10, search_type="full_text", filter='metadata["g"] == 1'))
        assert got == _expect(st, oracle, q, 10, g1)
        assert _got(st.query(text_query=q, top_k=10, search_type="full_text")) == _expect(st, oracle, q, 10)


def test_store_insert_after_query_tail_then_fold():
    texts, words, dense, sparse = _corpus(1500, 7)
    st = vs.GpuVectorStore(dense_dim=64, sparse_vocab=300, enable_full_text=True)
    st.TEXT_TAIL_MIN = 100
    whole = _store(texts, dense, sparse)
    q = f"common {words[4]} {words[11]}"

    def add(a, b):
        st.add_vectors([f"id{i}" for i in range(a, b)], dense[a:b], sparse[a:b], texts[a:b], [f"enh {i}" for i in range(a, b)],
                       [{"g": i % 3} for i in range(a, b)])

    add(0, 1000)
    assert _got(st.query(text_query=q, top_k=5, search_type="full_text")) == _expect(st, _oracle_of(texts[:1000]), q, 5)
    add(1000, 1100)                                                             # a tail segment behind the main one
    assert _got(st.query(text_query=q, top_k=5, search_type="full_text")) == _expect(st, _oracle_of(texts[:1100]), q, 5)
    assert st._text.stats()["segments"] == 2
    add(1100, 1150)                                                             # joins the tail
    assert _got(st.query(text_query=q, top_k=5, search_type="full_text")) == _expect(st, _oracle_of(texts[:1150]), q, 5)
    assert st._text.stats()["segments"] == 2
    add(1150, 1500)                                                             # the tail outgrows a quarter: one segment
    got = _got(st.query(text_query=q, top_k=50, search_type="full_text"))
    assert st._text.stats()["segments"] == 1
    assert got == _expect(st, _oracle_of(texts), q, 50) == _got(whole.query(text_query=q, top_k=50, search_type="full_text"))


def test_store_three_way_hybrid():
    texts, words, dense, sparse = _corpus(2000, 8)
    st = _store(texts, dense, sparse)
    oracle = _oracle_of(texts)
    weights = {"dense": 0.5, "sparse": 0.3, "full_text": 0.2}
    for i in (3, 17):
        dq, sq, tq = dense[i].tolist(), sparse[i], f"{words[5]} common {words[i]}"
        k = 6
        rbm = {"dense": st._search("dense", dq, 2 * k, None), "sparse": st._search("sparse", sq, 2 * k, None),
               "full_text": [{"id": st._ids[r], "distance": float(s), "_row": int(r)} for r, s in zip(*oracle.search(O.term_keys(tq), 2 * k))]}
        want = [(h["id"], h["distance"]) for h in vs.merge_hybrid_results(rbm, k, weights, 60)]
        assert _got(st.query(dense_query=dq, sparse_query=sq, text_query=tq, top_k=k, hybrid_weights=weights)) == want
        batch = st.query_batch(dense_queries=[dq], sparse_queries=[sq], text_queries=[tq], top_k=k, hybrid_weights=weights)
        assert _got(batch[0]) == want


def test_store_text_only_save_load_and_hot_path_index(tmp_path):
    texts, words, dense, sparse = _corpus(1200, 9)
    with pytest.raises(ValueError):
        vs.GpuVectorStore(enable_dense=False, enable_sparse=False)
    with pytest.raises(ValueError):
        vs.GpuVectorStore(enable_full_text=True, distributed=True)
    st = vs.GpuVectorStore(dense_dim=None, enable_dense=False, enable_sparse=False, enable_full_text=True, bm25_k1=1.5, bm25_b=0.6)
    n = len(texts)
    st.add_vectors([f"id{i}" for i in range(n)], None, None, texts, [""] * n, [{} for _ in range(n)])
    oracle = O.Bm25Oracle([O.term_keys(t) for t in texts], k1=1.5, b=0.6)
    q = f"{words[3]} {words[8]} common"
    before = _got(st.query(text_query=q, top_k=8, search_type="full_text"))
    assert before == _expect(st, oracle, q, 8)
    st.save(str(tmp_path / "s"))
    back = vs.GpuVectorStore.load(str(tmp_path / "s"))
    assert back.enable_full_text and back.bm25_k1 == 1.5 and back.bm25_b == 0.6
    assert _got(back.query(text_query=q, top_k=8, search_type="full_text")) == before
    idx = HotPathIndex(back)                                                   # no providers: full-text (index.py:58-64)
    assert _got(idx.query(q, k=8)) == before
    qs = [q, words[2], f"{words[6]} {words[6]}"]
    assert [_got(r) for r in idx.query_batch(qs, k=4)] == [_expect(back, oracle, x, 4) for x in qs]
