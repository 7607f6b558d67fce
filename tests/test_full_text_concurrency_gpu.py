"""Full-text search under concurrent readers and a writer, filters that predate inserts, and malformed UTF-8 given straight to
the C ABI (csrc/fulltext.hip)."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import full_text_oracle as O  # noqa: E402

import verbatim_rag_amd  # noqa: F401,E402
from verbatim_rag_amd import _lib  # noqa: E402
from verbatim_rag_amd import vector_stores as vs  # noqa: E402

pytestmark = pytest.mark.gpu


def _raw_tokens(docs):
    """vrag_text_tokenize on raw byte strings (no Python str in between)."""
    lib = _lib.load()
    blob = b"".join(docs)
    off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    counts = np.zeros(len(docs), np.int32)
    keys = np.zeros(max(1, len(blob)), np.uint64)
    n = C.c_int64()
    _lib.check("vrag_text_tokenize", lib.vrag_text_tokenize(blob, off.ctypes.data_as(C.POINTER(C.c_int64)), len(docs), 0, len(keys),
                                                            counts.ctypes.data_as(C.POINTER(C.c_int32)), keys.ctypes.data, C.byref(n)))
    return counts.tolist(), keys[: n.value].tolist()


def test_malformed_utf8_decodes_to_replacement_characters():
    k = lambda s: O.fnv1a64(s.encode())   # noqa: E731
    cases = [
        (b"\xc1\x81bc", ["bc"]),                      # overlong 'A' (C1 lead): U+FFFD, not a letter
        (b"\xc0\xafx", ["x"]),                        # overlong '/'
        (b"a\xe0\x80\x81b", ["a", "b"]),              # overlong three-byte form
        (b"a\xed\xa0\x80b", ["a", "b"]),              # an encoded surrogate
        (b"a\xf4\x90\x80\x80b", ["a", "b"]),          # above U+10FFFF
        (b"a\xf8b\x80c", ["a", "b", "c"]),            # bytes that start nothing
        (b"\xc3\xa9t\xc3\xa9", ["été"]),    # well-formed stays well-formed
        (b"ab\xe2\x82", ["ab"]),                      # truncated at the end
    ]
    counts, keys = _raw_tokens([c for c, _ in cases])
    assert counts == [len(w) for _, w in cases]
    assert keys == [k(t) for _, w in cases for t in w]


def test_rows_beyond_the_allow_bitmap_are_not_returned():
    texts = [f"alpha beta row{i} " + ("gamma " * (i % 5)) for i in range(3000)]
    ix = vs.TextIndex()
    ix.add(texts, fold=True)
    oracle = O.Bm25Oracle([O.term_keys(t) for t in texts])
    allow = np.arange(1000) % 2 == 0                       # built when the index held 1000 rows
    scores, ids = ix.search(["gamma alpha"], 1024, allow)
    full = np.zeros(3000, dtype=bool)
    full[:1000] = allow
    rows, sc = oracle.search(O.term_keys("gamma alpha"), 1024, full)
    m = len(rows)
    assert m == 500 and ids[0, :m].tolist() == rows.tolist() and scores[0, :m].tolist() == sc.tolist()
    assert (ids[0, m:] == -1).all()
    ix.close()


def test_concurrent_full_text_queries_inserts_and_deletes():
    """Readers (full-text with and without a filter, batched, weighted hybrid) while a writer inserts and deletes: no call
    fails, every hit passes the filter, and afterwards the store answers like the oracle over its final rows."""
    texts, words, _keys, _lens = O.zipf_corpus(6000, vocab=300, mean_len=10, seed=21)
    rng = np.random.default_rng(4)
    dense = rng.standard_normal((6000, 32)).astype(np.float32)
    st = vs.GpuVectorStore(dense_dim=32, enable_sparse=False, enable_full_text=True)
    st.TEXT_TAIL_MIN = 200

    def add(a, b):
        st.add_vectors([f"id{i}" for i in range(a, b)], dense[a:b], None, texts[a:b], [""] * (b - a), [{"g": i % 3} for i in range(a, b)])

    add(0, 2000)
    errors, stop = [], threading.Event()
    flt = 'metadata["g"] == 1'

    def reader(seed):
        r = np.random.default_rng(seed)
        try:
            while not stop.is_set():
                q = f"{words[int(r.integers(0, 50))]} common {words[int(r.integers(0, 300))]}"
                for res in (st.query(text_query=q, top_k=8, search_type="full_text", filter=flt),
                            *st.query_batch(text_queries=[q, q.upper()], top_k=5, search_type="full_text", filter=flt)):
                    assert all(int(x.id[2:]) % 3 == 1 for x in res), [x.id for x in res]
                hy = st.query(dense_query=dense[int(r.integers(0, 2000))].tolist(), text_query=q, top_k=5,
                              hybrid_weights={"dense": 0.5, "full_text": 0.5}, filter=flt)
                assert hy and all(int(x.id[2:]) % 3 == 1 for x in hy)
        except Exception as e:   # noqa: BLE001 -- reported below
            errors.append(repr(e))

    threads = [threading.Thread(target=reader, args=(s,)) for s in range(4)]
    for t in threads:
        t.start()
    try:
        for a in range(2000, 6000, 250):
            add(a, a + 250)
            st.delete([f"id{i}" for i in range(a - 2000, a - 1900, 7)])
    finally:
        stop.set()
        for t in threads:
            t.join()
    assert not errors, errors[:3]
    live = st._alive.data.copy()
    oracle = O.Bm25Oracle([O.term_keys(t) for t in texts])
    oracle.set_live(live)
    g1 = np.arange(6000) % 3 == 1
    for q in (f"{words[3]} common", words[17], f"{words[1]} {words[2]} {words[40]}"):
        rows, sc = oracle.search(O.term_keys(q), 10, g1)
        want = [(f"id{r}", float(s)) for r, s in zip(rows.tolist(), sc.tolist())]
        assert [(x.id, x.score) for x in st.query(text_query=q, top_k=10, search_type="full_text", filter=flt)] == want
