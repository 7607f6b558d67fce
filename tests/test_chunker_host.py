"""Host side of the markdown chunker and of HotPathIndex.add_documents, against what the REFERENCE returned
(tests/golden/chunker_fixtures.json, written by tests/golden/gen_golden_chunker.py): the restatement of rules R1-R8 the GPU
tests compare the kernel with (tests/chunk_ref.py), the product's size stages, and the document ingest of the index with fake
chunker / providers / store.  Nothing here needs a GPU."""
import hashlib
import json
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import chunk_ref  # noqa: E402


def digest(chunks):
    h = lambda s: hashlib.sha1(s.encode("utf-8", "surrogatepass")).hexdigest()[:10]
    return [[len(raw), h(raw), len(enhanced), h(enhanced)] for raw, enhanced in chunks]


@pytest.fixture(scope="module")
def fixtures():
    with open(os.path.join(HERE, "golden", "chunker_fixtures.json")) as f:
        return json.load(f)


def check_run(run, got, where):
    if "want" in run:
        assert [list(t) for t in got] == run["want"], where
    else:
        assert digest(got) == run["want_digest"], where


def test_fixture_file_covers_the_cases_it_should(fixtures):
    cases = fixtures["chunker"]
    texts = {c["text"] for c in cases}
    assert {"", "#", "# ", "#\n", "\n\n\n", "#\n## B\ntext\n# C\n"} <= texts
    assert any("\ud800" in t for t in texts) and any("\r\n" in t for t in texts) and any("####### " in t for t in texts)
    assert sum(1 for c in cases if len(c["runs"]) == 5) >= 20                      # the sized synthetic documents
    assert max(len(c["runs"][0].get("want", [])) for c in cases) >= 6
    assert os.path.getsize(os.path.join(HERE, "golden", "chunker_fixtures.json")) < 200_000


def test_chunk_ref_equals_every_structural_fixture(fixtures):
    n = 0
    for c in fixtures["chunker"]:
        for run in c["runs"]:
            if run["min"] is None and run["max"] is None:
                check_run(run, chunk_ref.chunk_ref(c["text"], tuple(c["levels"]), c["preamble"]), repr(c["text"][:60]))
                n += 1
    assert n >= 250


def test_chunk_ref_tables_are_consistent_with_its_tuples():
    """The record tables (what the kernel is compared with) rebuild the tuples; five ancestors, pops and dropped blocks."""
    text = "pre\n# 1\n## 2\n### 3\n#### 4\n##### 5\n###### 6\ndeep\n## B\n"
    data = chunk_ref.encode(text)
    headers, chunks = chunk_ref.tables(data, (1, 2, 3, 4, 5, 6), True)
    assert [h[1] for h in headers] == [1, 2, 3, 4, 5, 6, 2]
    assert chunks[0] == [0, 0, 4, -1, 0, -1, -1, -1, -1, -1]
    assert chunks[6][3:] == [5, 5, 0, 1, 2, 3, 4] and chunks[7][3:] == [6, 1, 0, -1, -1, -1, -1]
    assert b"".join(data[c[1]:c[2]] for c in chunks) == data
    headers, chunks = chunk_ref.tables(data, (2, 6), False)
    assert [c[3] for c in chunks] == [1, 5, 6] and chunks[1][4:] == [5, 0, 1, 2, 3, 4]
    assert headers[0][2:7] == [4, 7, 6, 7, 8]                       # line [4, 7), title [6, 7), block up to the next header


def test_size_stages_equal_every_sized_fixture(fixtures):
    from verbatim_rag_amd.chunker_providers import apply_size_limits

    n = split = merged = 0
    for c in fixtures["chunker"]:
        structural = chunk_ref.structural(c["text"], tuple(c["levels"]), c["preamble"])
        for run in c["runs"]:
            if run["min"] is None and run["max"] is None:
                continue
            got = apply_size_limits(structural, c["text"], run["min"], run["max"])
            check_run(run, got, f"{c['text'][:40]!r} min={run['min']} max={run['max']}")
            n += 1
            split += len(got) > len(structural)
            merged += len(got) < len(structural)
    assert n >= 80 and split >= 10 and merged >= 10


def test_size_stages_quirks():
    """The reference's quirks, stated outright: the second enhanced text's prefix lands in the middle of a merged chunk; a
    sub-chunk's ancestors are `## title` lines; a protected table is not split; a merged chunk over a dropped block is placed
    at -1."""
    from verbatim_rag_amd.chunker_providers import apply_size_limits

    got = apply_size_limits([("# A\n", "# A\n", ["A"]), ("## B\nbody\n", "# A\n\n## B\nbody\n", ["A", "B"])], "# A\n## B\nbody\n", 8, None)
    assert got == [("# A\n## B\nbody\n", "# A\n# A\n\n## B\nbody\n")]
    raw = "### C\n\n" + "x" * 30 + "\n\n" + "y" * 30 + "\n"
    got = apply_size_limits([(raw, "# A\n## B\n\n" + raw, ["A", "B", "C"])], "# A\n## B\n" + raw, None, 40)
    assert got == [("### C\n\n" + "x" * 30, "## A\n## B\n\n### C\n\n" + "x" * 30), ("\n\n" + "y" * 30 + "\n", "## A\n## B\n\n\n\n" + "y" * 30 + "\n")]
    table = "| a | b |\n|---|---|\n\n| c | d |\n"                       # one table region per block of | lines; the break between them is free
    fence = "```\nline\n\nline\n```\n"
    doc = "# T\n" + fence
    assert apply_size_limits([(doc, doc, ["T"])], doc, None, 5) == [(doc, doc)]                  # the only break is inside the fence
    doc = "# T\n" + table
    assert len(apply_size_limits([(doc, doc, ["T"])], doc, None, 5)) == 2


class FakeChunker:
    """The reference's structural chunks through chunk_ref: add_documents sees a chunker with `chunk` only."""

    def __init__(self):
        self.calls = []

    def chunk(self, text):
        self.calls.append(text)
        return chunk_ref.chunk_ref(text)


class BatchChunker(FakeChunker):
    def chunk_batch(self, texts):
        self.calls.append(list(texts))
        return [chunk_ref.chunk_ref(t) for t in texts]


class Recorder:
    enable_full_text = False

    def __init__(self):
        self.calls = []

    def add_vectors(self, ids, dense_vectors, sparse_vectors, texts, enhanced_texts, metadatas):
        self.calls.append(["add_vectors", {"ids": list(ids), "dense": dense_vectors and list(dense_vectors), "sparse": sparse_vectors and list(sparse_vectors), "texts": list(texts),
                                           "enhanced_texts": list(enhanced_texts),
                                           "metadatas": [list(map(list, m.items())) for m in metadatas]}])

    def add_documents(self, documents):
        self.calls.append(["add_documents", [list(map(list, d.items())) for d in documents]])


class Provider:
    def __init__(self, name, store):
        self.name, self.store = name, store

    def embed_batch(self, texts):
        self.store.calls.append([self.name, digest([(t, "") for t in texts])])
        return [len(t) for t in texts]


class Doc:
    """An object document (the mapping form is the fixture's own dict)."""

    def __init__(self, d, content_type):
        self.id, self.title, self.source, self.raw_content, self.metadata = d["id"], d["title"], d["source"], d["content"], dict(d["metadata"])
        self.content_type = content_type
        self.chunks = []


class Kind:
    value = "markdown"


@pytest.mark.parametrize("form", ["mapping", "object", "batch_chunker"])
def test_add_documents_equals_the_reference_bulk_ingest(fixtures, form):
    from verbatim_rag_amd.index import HotPathIndex

    fx = fixtures["index"]
    assert any(kw["kw"]["batch_chunks"] == 2 for kw in fx["runs"])            # cuts inside a document
    for run in fx["runs"]:
        store = Recorder()
        chunker = BatchChunker() if form == "batch_chunker" else FakeChunker()
        idx = HotPathIndex(store, Provider("embed_dense", store), Provider("embed_sparse", store), chunker_provider=chunker)
        if form == "object":
            docs = [Doc(d, Kind()) for d in fx["documents"]]
        else:
            docs = [{**d, "content_type": fx["content_type"]} for d in fx["documents"]]
        counter = iter(range(10 ** 6))
        idx.add_documents(iter(docs), id_factory=lambda: next(counter), **run["kw"])
        assert store.calls == run["calls"], run["kw"]
        if form == "batch_chunker":                                            # once per batch_docs documents
            step = run["kw"]["batch_docs"]
            assert chunker.calls == [[d["content"] for d in fx["documents"][a:a + step]] for a in range(0, len(docs), step)]
        else:
            assert chunker.calls == [d["content"] for d in fx["documents"]]


def test_add_documents_defaults_and_rejections():
    from verbatim_rag_amd.index import HotPathIndex

    store = Recorder()
    idx = HotPathIndex(store, Provider("embed_dense", store), chunker_provider=FakeChunker())
    idx.add_documents([{"id": "a", "content": "# T\nx\n", "metadata": None}])
    call = store.calls[1][1]
    assert re.fullmatch(r"[0-9a-f]{8}-[0-9a-f]{4}-4[0-9a-f]{3}-[89ab][0-9a-f]{3}-[0-9a-f]{12}", call["ids"][0])   # uuid4
    assert call["sparse"] is None and call["dense"] == [len(call["enhanced_texts"][0])]
    assert call["enhanced_texts"] == ["# T\nx\n\n\n---\nDocument: Unknown"]
    assert dict(call["metadatas"][0])["content_type"] is None and store.calls[2][1][0][3] == ["content_type", None]
    with pytest.raises(ValueError, match="add_chunks"):
        idx.add_documents([{"id": "b", "content": "x", "chunks": [object()]}])
    idx.add_documents([])
    assert len(store.calls) == 3

    class NoDocs:
        enable_full_text = False

        def __init__(self):
            self.rows = []

        def add_vectors(self, ids, *rest):
            self.rows += ids

    plain = NoDocs()                                                           # a store without add_documents: chunk rows only
    HotPathIndex(plain, Provider("embed_dense", Recorder()), chunker_provider=FakeChunker()).add_documents([{"id": "a", "content": ""}])
    assert len(plain.rows) == 1                                                # an empty document is one empty chunk


def test_constructor_creates_no_chunker_and_needs_no_gpu(monkeypatch):
    import verbatim_rag_amd.chunker_providers as cp
    from verbatim_rag_amd.index import HotPathIndex

    made = []
    monkeypatch.setattr(cp.GpuMarkdownChunker, "__init__", lambda self, *a, **k: made.append(1))
    store = Recorder()
    idx = HotPathIndex(store, Provider("embed_dense", store))
    assert idx.chunker_provider is None and not made
    monkeypatch.setattr(cp.GpuMarkdownChunker, "chunk_batch", lambda self, texts: [chunk_ref.chunk_ref(t) for t in texts], raising=True)
    idx.add_documents([{"id": "a", "content": "x"}])                           # the first call makes the default chunker
    assert made == [1] and isinstance(idx.chunker_provider, cp.GpuMarkdownChunker)
    idx.add_documents([{"id": "b", "content": "y"}])
    assert made == [1]


def test_gpu_chunker_has_no_cpu_fallback(gpu_available):
    from verbatim_rag_amd.chunker_providers import ChunkerProvider, GpuMarkdownChunker

    c = GpuMarkdownChunker(min_chunk_size=10)
    assert isinstance(c, ChunkerProvider) and c.split_levels == (1, 2, 3, 4) and c.include_preamble and c.max_chunk_size is None
    if not gpu_available:
        with pytest.raises(RuntimeError, match="no HIP device"):
            c.chunk("# a\nb\n")


def test_symbol_is_declared_exported_and_bound():
    from verbatim_rag_amd import _lib

    with open(os.path.join(ROOT, "include", "vrag_amd.h")) as f:
        hdr = f.read()
    assert re.search(r"\bint vrag_chunk_markdown\(", hdr) and "vrag_md_header;" in hdr and "vrag_md_chunk;" in hdr
    assert re.search(r"#define VRAG_ABI_VERSION 6\b", hdr)
    assert "vrag_chunk_markdown" in _lib.SIGNATURES and len(_lib.SIGNATURES["vrag_chunk_markdown"][1]) == 13
    assert _lib.load().vrag_chunk_markdown.argtypes is not None
    with open(os.path.join(ROOT, "verbatim-rag_amd", "build.py")) as f:
        assert '"chunk.hip"' in f.read()


def test_entry_point_argument_errors_come_before_the_device():
    """Bad arguments are VRAG_ERR_INVALID with or without a GPU; good ones without a GPU are VRAG_ERR_NO_DEVICE."""
    import ctypes as C

    import numpy as np

    from verbatim_rag_amd import _lib

    lib = _lib.load()
    text = b"# a\nb\n"
    buf = (C.c_char * len(text)).from_buffer_copy(text)
    hdr, chk = np.zeros((4, 8), np.int32), np.zeros((4, 10), np.int32)
    nh, nc = C.c_int64(-1), C.c_int64(-1)
    dco = np.zeros(3, np.int64)

    def call(off, n_docs=1, levels=0b11110, hcap=4, ccap=4):
        off = np.asarray(off, np.int64)
        return lib.vrag_chunk_markdown(C.cast(buf, C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), n_docs, levels, 1, hcap,
                                       hdr.ctypes.data_as(C.c_void_p), ccap, chk.ctypes.data_as(C.c_void_p), C.byref(nh), C.byref(nc),
                                       dco.ctypes.data_as(C.POINTER(C.c_int64)), 0)

    assert call([0, 6], levels=1) == -1 and "split_levels" in _lib.last_error()
    assert call([0, 6], levels=1 << 7) == -1
    assert call([1, 6]) == -1 and "doc_off[0]" in _lib.last_error()
    assert call([0, 6, 3], n_docs=2) == -1
    assert call([0, 6], n_docs=0) == -1
    assert call([0, 6], hcap=-1) == -1
    assert call([0, (512 << 20) + 1]) == -1 and "at most" in _lib.last_error()
    if lib.vrag_device_count() == 0:
        assert call([0, 6]) == -4
