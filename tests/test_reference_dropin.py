"""The drop-in claim against the reference's recorded behaviour: the REFERENCE's own `VerbatimIndex`, `VerbatimRAG` and
`VerbatimTransform` were run over this package's store / providers / extractor by tests/golden/gen_golden_dropin.py, and
what they returned -- and every call they made into this package's store and extractor, with its arguments and result --
is stored in tests/golden/dropin_fixtures.json.  This package's restatement of the same pipeline (`HotPathIndex` +
`StaticVerbatimPipeline`) must return exactly what the reference returned, and the recorded calls, replayed on this
package's objects, must return what they returned then.  Device classes are replaced by CPU stand-ins (oracle-backed
shards, a logit function of the token ids): what is under test is every Python-level seam between the two code bases --
argument names, return types, `SearchResult` fields, dict keys, scores, highlight offsets, citations."""
import asyncio
import enum
import json
import os
import types

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from test_fast_packer import RecordingEngine
from test_store_host_logic import _Dense, _Sparse
from verbatim_rag_amd import vector_stores as vs

G = os.path.join(os.path.dirname(__file__), "golden")
QUESTIONS = ("Where is the tall tower?", "How many stairs do visitors climb?")
INDEX_QUERIES = (dict(text="Where is the tall tower?", k=5), dict(text="Visitors climb stairs", k=3, search_type="sparse"),
                 dict(text="city", k=4, search_type="dense", filter='metadata["document_id"] == "d1"'),
                 dict(text="Where is it?", k=5, hybrid_weights={"dense": 0.7, "sparse": 0.3}, rrf_k=20))


class Dense:
    def embed_text(self, t):
        v = np.zeros(64, np.float32)
        v[len(t) % 64] = 1.0
        v[(len(t) * 7) % 64] += 0.5
        return v.tolist()

    def embed_batch(self, ts):
        return [self.embed_text(t) for t in ts]

    def get_dimension(self):
        return 64


class Sparse:
    def embed_text(self, t):
        return {(len(w) * 13 + ord(w[0])) % 300: 1.0 + 0.25 * (len(w) % 3) for w in t.split()[:12]}

    def embed_batch(self, ts):
        return [self.embed_text(t) for t in ts]

    def get_dimension(self):
        return 300


def cpu_stand_ins(setattr_):
    """Routes GpuVectorStore to the CPU shards (`setattr_` is monkeypatch.setattr, or plain setattr in the generator)."""
    setattr_(vs._lib, "load", lambda: None)
    setattr_(vs._lib, "require_gpu", lambda: None)
    setattr_(vs, "DenseShard", _Dense)
    setattr_(vs, "SparseShard", _Sparse)


def tower_docs(n):
    return [f"The tower number {i} is tall. It stands in city {i % 4}. Visitors climb {i + 3} stairs! Was it built in {1800 + i}?" for i in range(n)]


def corpus(n, document_ids):
    """(store, this package's index over it, extractor): the corpus both pipelines ran on."""
    from tokenizers import Tokenizer

    from verbatim_rag_amd.extractors import GpuModelSpanExtractor
    from verbatim_rag_amd.index import HotPathIndex

    docs = tower_docs(n)
    metas = [dict({"document_id": f"d{i % 3}"} if document_ids else {}, title=f"Doc {i}", source=f"s{i}.md") for i in range(n)]
    store = vs.GpuVectorStore(dense_dim=64, sparse_vocab=300)
    ours = HotPathIndex(store, dense_provider=Dense(), sparse_provider=Sparse())
    ours.add_chunks([f"c{i}" for i in range(n)], docs, metadatas=metas)
    ext = GpuModelSpanExtractor(engine=RecordingEngine(), tokenizer=Tokenizer.from_file(os.path.join(G, "tokenizer.json")), threshold=0.5)
    return store, ours, ext


def hits(results):
    return [[x.id, x.score, x.text, x.metadata] for x in results]


class PairEngine:                                           # cross-encoder stand-in: score = overlap with the question
    max_seqs, max_tokens, max_seq_len, pair_labels = 64, 8192, 512, 1
    shape = types.SimpleNamespace(cls_token_id=1, sep_token_id=2)

    def pair_logits(self, seqs, types_):
        return np.asarray([[float(sum(t) % 17)] for t in seqs], np.float32)


def _as_json(x):
    return json.loads(json.dumps(x))


def encode(x):
    """JSON form of what crosses a seam: arrays, enum members, dicts with non-string keys and result objects are tagged so
    `decode` rebuilds them (an enum member comes back as a member of a stand-in enum with the same value, a result object
    as a plain namespace carrying the same fields)."""
    if isinstance(x, enum.Enum):
        return {"__enum__": encode(x.value)}
    if isinstance(x, np.ndarray):
        return {"__nd__": x.tolist(), "dtype": str(x.dtype)}
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, dict):
        if all(isinstance(k, str) for k in x):
            return {k: encode(v) for k, v in x.items()}
        return {"__kv__": [[encode(k), encode(v)] for k, v in x.items()]}
    if isinstance(x, (list, tuple)):
        return [encode(v) for v in x]
    if hasattr(x, "model_dump"):
        return {"__obj__": encode(x.model_dump())}
    if hasattr(x, "__dict__"):
        return {"__obj__": encode(vars(x))}
    return x


def decode(x):
    if isinstance(x, list):
        return [decode(v) for v in x]
    if isinstance(x, dict):
        if "__nd__" in x:
            return np.asarray(x["__nd__"], dtype=x["dtype"])
        if "__enum__" in x:
            return enum.Enum("Recorded", {"MEMBER": decode(x["__enum__"])}).MEMBER
        if "__kv__" in x:
            return {decode(k): decode(v) for k, v in x["__kv__"]}
        if "__obj__" in x:
            return types.SimpleNamespace(**decode(x["__obj__"]))
        return {k: decode(v) for k, v in x.items()}
    return x


class Recorder:
    """Stands in for `target` and logs every method call made on it: name, arguments and result, encoded."""

    def __init__(self, target):
        self._target, self.calls = target, []

    def __getattr__(self, name):
        attr = getattr(self._target, name)
        if not callable(attr):
            return attr

        def call(*args, **kwargs):
            out = attr(*args, **kwargs)
            self.calls.append({"method": name, "args": encode(list(args)), "kwargs": encode(kwargs), "result": encode(out)})
            return out

        return call


def replay(target, calls):
    """Makes the recorded calls on `target`; each must return what it returned when recorded.  -> the results."""
    got = []
    for c in calls:
        out = getattr(target, c["method"])(*decode(c["args"]), **decode(c["kwargs"]))
        assert _as_json(encode(out)) == c["result"], (c["method"], c["kwargs"])
        got.append(out)
    return got


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(G, "dropin_fixtures.json")) as f:
        return json.load(f)


def test_pipeline_matches_the_recorded_reference_pipeline(recorded, monkeypatch):
    from verbatim_rag_amd.pipeline import StaticVerbatimPipeline

    cpu_stand_ins(monkeypatch.setattr)
    _store, ours, ext = corpus(30, document_ids=True)
    assert [r["kw"] for r in recorded["index_queries"]] == _as_json(list(INDEX_QUERIES))
    for kw, rec in zip(INDEX_QUERIES, recorded["index_queries"]):
        got = _as_json(hits(ours.query(**kw)))
        assert got == rec["results"] and 0 < len(got) <= kw["k"]

    pipe = StaticVerbatimPipeline(ours, ext, k=5)
    for question in QUESTIONS:
        mine = pipe.query(question)
        assert _as_json(mine.model_dump()) == recorded["pipeline_k5"][question]
        assert len(mine.documents) == 5 and any(d.highlights for d in mine.documents)
        for d in mine.documents:
            assert all(d.content[h.start:h.end] == h.text for h in d.highlights)
    assert _as_json([r.model_dump() for r in pipe.query_batch(list(QUESTIONS))]) == [recorded["pipeline_k5"][q] for q in QUESTIONS]


def test_reranked_pipeline_and_async_extraction_match_the_recorded_reference(recorded, monkeypatch):
    """`reranker=` hook (the reference's core.py:125-140) and the async extractor entry the reference's `query_async` awaits."""
    from tokenizers import Tokenizer

    from verbatim_rag_amd.extractors import CoalescingSpanExtractor
    from verbatim_rag_amd.pipeline import StaticVerbatimPipeline
    from verbatim_rag_amd.rerankers import GpuCrossEncoderReranker

    cpu_stand_ins(monkeypatch.setattr)
    _store, ours, ext = corpus(20, document_ids=False)
    question = QUESTIONS[0]
    sync = _as_json(StaticVerbatimPipeline(ours, ext, k=4).query(question).model_dump())
    assert sync == recorded["pipeline_k4"]

    results = ours.query(text=question, k=4)
    spans = ext.extract_spans(question, results)
    assert any(spans.values()) and asyncio.run(ext.extract_spans_async(question, results)) == spans
    co = CoalescingSpanExtractor(ext, max_wait_ms=1.0)          # the per-query interface in front of the batch path
    try:
        assert asyncio.run(co.extract_spans_async(question, results)) == spans
        assert _as_json(StaticVerbatimPipeline(ours, co, k=4).query(question).model_dump()) == sync
    finally:
        co.close()

    # dict contexts, one of them text only, coerced by the reference's VerbatimTransform and IndexProvider
    # (transform.py:86-112, providers.py:40-84) into minimal result objects (id, text, score, metadata; the text-only one
    # with an empty title): this extractor gets them as recorded, as plain namespaces, and must return the spans it
    # returned then
    calls = recorded["transform_extract_calls"]
    assert [c["method"] for c in calls] == ["extract_spans", "extract_spans"]
    minimal = calls[0]["args"][1]
    assert all(set(r["__obj__"]) == {"id", "text", "score", "metadata"} for r in minimal) and minimal[1]["__obj__"]["metadata"]["title"] == ""
    assert all(any(spans.values()) for spans in replay(ext, calls))

    rr = GpuCrossEncoderReranker(PairEngine(), Tokenizer.from_file(os.path.join(G, "tokenizer.json")), rerank_k=3)
    reranked = _as_json(StaticVerbatimPipeline(ours, ext, k=4, reranker=rr).query(question).model_dump())
    assert reranked == recorded["pipeline_k4_reranked"]
    assert [d["content"] for d in reranked["documents"]] != [d["content"] for d in sync["documents"]]


def test_store_serves_the_recorded_reference_ingest_path(recorded, monkeypatch, tmp_path):
    """`VerbatimIndex.add_documents` (index.py:318-411: the reference's chunker, `_prepare_chunk_metadata`,
    `_generate_embeddings`, `_store_chunks` -> `store.add_vectors(ids=, dense_vectors=, sparse_vectors=, texts=,
    enhanced_texts=, metadatas=)`, `_store_document_metadata` -> `store.add_documents(records)`), then queries, a `document_id`
    filter built the reference's way, the accessors built on the store (index.py:657-760), a document miss: every store call
    it made is replayed on a fresh store, and the reads once more on that store saved and loaded."""
    cpu_stand_ins(monkeypatch.setattr)
    rec = recorded["ingest"]
    calls, doc_id = rec["calls"], rec["document_id"]
    assert {"add_vectors", "add_documents", "query", "get_document"} <= {c["method"] for c in calls}
    store = vs.GpuVectorStore(dense_dim=64, sparse_vocab=300)
    got = replay(store, calls)
    assert len(store._ids) >= 6 and all(isinstance(v, (str, int, float, bool, type(None), list, dict)) for md in store._meta for v in md.values())
    filtered = [g for c, g in zip(calls, got) if c["method"] == "query" and doc_id in str(c["kwargs"].get("filter"))]
    assert filtered and all(h.metadata["document_id"] == doc_id for hs in filtered for h in hs) and all(filtered)
    rec_doc = store.get_document(doc_id)
    assert rec_doc is not None and rec_doc["id"] == doc_id and rec_doc["title"].startswith("Doc ") and store.get_document("nope") is None

    store.save(str(tmp_path / "idx"))
    again = vs.GpuVectorStore.load(str(tmp_path / "idx"))
    replay(again, [c for c in calls if c["method"] in ("query", "get_document")])
    assert again.get_document(doc_id) == rec_doc
