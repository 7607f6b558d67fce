#!/usr/bin/env python3
"""Generates tests/golden/chunker_fixtures.json by running the REFERENCE's own `MarkdownChunkerProvider.chunk` and
`VerbatimIndex.add_documents_bulk` (over a recording store and recording providers).  Nothing of the reference travels: only
the texts fed to it and what it returned / handed to the store.  Run where a reference checkout is present:
`python tests/golden/gen_golden_chunker.py <reference checkout>`.

`synth_markdown` (seeded markdown with paragraphs, tables, captions, code fences and repeated sections) is also what
tools/probes/chunker_probe.py builds its corpora from."""
from __future__ import annotations

import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

ALPHABET = ["#", " ", "\n", "\t", "a", "b", "|", "`", "\r", "\u00a0", "\u3000", "é", "😀", "\x0b", "\x1c", "\u0085", "-"]
WEIGHTS = [6, 4, 5, 1, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
CONFIGS = [((1, 2, 3, 4), True), ((2, 3), False), ((1, 2, 3, 4, 5, 6), True)]
SIZES = [(None, None), (200, None), (None, 400), (150, 500), (50, 120)]

EDGES = [
    "#\n## B\ntext\n# C\n",                                  # a swallowed header
    "####### seven\ntext\n###### six\n",                     # 7 hashes are no header
    "text\n#", "#", "# ", "#\n", "", "\n\n\n", "##",
    "# A\r\ntext\r\n## B\r\nmore\r\n",                       # \r ends no line
    "#\u00a0nbsp\n##\u3000wide\n###\x1cfs\n#\u0085nel\n#\u200bzero width is no space\n",
    "# Title with trailing   \t \u3000\nbody\n",
    "# 1\n## 2\n### 3\n#### 4\n##### 5\n###### 6\ndeep\n",    # five ancestors (with all six levels split)
    "# A\n### C\n## B\n#### D\n# E\n## F\n",                  # levels that pop
    "intro\n# A\n##### five\ndropped text\n## B\n###### six\n### C\n",   # levels outside split_levels: ancestors and dropped blocks
    "preamble only\n\n## H\ntext",
    "## starts at zero\ntext\n",
    "lone \ud800 surrogate\n# H \udfff\nx\n",
    "#\n\n\n   \n# swallowed too\nreal title\n# next\n",
    "no header here\n #not\nx# not\n\\# not\n",
    "# a\n# a\n# a\n",
    "#\t\ttabs\n#\x0b\x0c\n## end",
    "é😀\n# é😀 \n## 😀\nüü\n",
]


def _words(rng: random.Random, n: int) -> str:
    pool = ["tower", "bridge", "river", "the", "of", "Zürich", "naïve", "data", "model", "heat", "x1", "中文", "and", "result"]
    return " ".join(rng.choice(pool) for _ in range(n))


def _table(rng: random.Random, number: int) -> str:
    rows = ["| name | value |", "|------|:-----:|"] + [f"| {_words(rng, 1)} | {rng.randrange(100)} |" for _ in range(rng.randrange(1, 5))]
    body = "\n".join(rows) + "\n"
    kind = rng.randrange(4)
    if kind == 0:
        return f"Table {number}: {_words(rng, 3)}\n\n{body}"
    if kind == 1:
        return f"{body}\nTable {number}. {_words(rng, 3)}\n"
    if kind == 2:
        return f"Table {number}: {_words(rng, 2)}\n{body}"
    return body


def _fence(rng: random.Random) -> str:
    return "```python\nx = 1\n\n\n# not a header? it is one to the chunker\ny = 2\n\nprint(x)\n```\n"


def synth_markdown(rng: random.Random, approx_bytes: int) -> str:
    """Markdown of about `approx_bytes`: sections of levels 1-6, paragraphs, tables, code fences, repeated sections."""
    parts = [_words(rng, rng.randrange(3, 12)) + "\n\n"] if rng.random() < 0.7 else []
    size = sum(len(p) for p in parts)
    level, tables, sections = 1, 0, []
    while size < approx_bytes:
        if sections and rng.random() < 0.12:
            section = rng.choice(sections)                  # a repeated identical section
        else:
            level = max(1, min(6, level + rng.choice([-2, -1, 0, 0, 1, 1])))
            body = [f"{'#' * level} {_words(rng, rng.randrange(1, 4))}" + rng.choice(["", "", " ", "  \t"]) + "\n"]
            if rng.random() < 0.8:
                body.append("\n")
            for _ in range(rng.randrange(0, 4)):
                pick = rng.random()
                if pick < 0.65:
                    body.append(_words(rng, rng.randrange(4, 40)) + rng.choice([".\n\n", ".\n\n\n", ".\n"]))
                elif pick < 0.85:
                    tables += 1
                    body.append(_table(rng, tables) + "\n")
                else:
                    body.append(_fence(rng) + "\n")
            section = "".join(body)
            sections.append(section)
        parts.append(section)
        size += len(section.encode("utf-8"))
    return "".join(parts)


def random_string(rng: random.Random, max_len: int = 40) -> str:
    return "".join(rng.choices(ALPHABET, WEIGHTS, k=rng.randrange(0, max_len + 1)))


def digest(chunks) -> list:
    """A chunk list too long to store: per chunk the lengths and a hash of each text."""
    h = lambda s: hashlib.sha1(s.encode("utf-8", "surrogatepass")).hexdigest()[:10]
    return [[len(raw), h(raw), len(enhanced), h(enhanced)] for raw, enhanced in chunks]


INDEX_DOCS = [
    {"id": "d0", "title": "Towers", "source": "towers.md", "content": "intro\n\n# A\n\ntext a\n\n## B\n\ntext b\n\n## C\n\ntext c\n",
     "metadata": {"doc_type": "report", "year": 2021, "user_id": "u1", "dataset_id": "ds", "userId": "u2", "lead_author": "X"}},
    {"id": "d1", "title": "", "source": "", "content": "# Only\nbody\n", "metadata": {}},
    {"id": "d2", "title": "Empty", "source": "empty.md", "content": "", "metadata": {"note": None}},
    {"id": "d3", "title": "No source", "source": "", "content": "plain text without headers", "metadata": {"title": "overlaid"}},
    {"id": "d0", "title": "Towers again", "source": "dup.md", "content": "# Dup\nx\n", "metadata": {}},
    {"id": "d5", "title": "", "source": "s5.md", "content": "# 1\n## 2\n### 3\ntext\n## 4\n# 5\n", "metadata": {"k": [1, 2]}},
]
INDEX_RUNS = [{"batch_chunks": 2000, "batch_docs": 500}, {"batch_chunks": 2, "batch_docs": 2}, {"batch_chunks": 3, "batch_docs": 4}]


def main(ref: str) -> None:
    sys.path[:0] = [HERE]
    import gen_golden

    gen_golden.REF = os.path.abspath(ref)
    gen_golden._install_stubs()
    from verbatim_rag.chunker_providers import MarkdownChunkerProvider
    from verbatim_rag.document import Document, DocumentType
    from verbatim_rag.index import VerbatimIndex

    def run(text, levels, preamble, lo=None, hi=None):
        return [list(t) for t in MarkdownChunkerProvider(levels, preamble, lo, hi).chunk(text)]

    cases = []
    for text in EDGES:
        for levels, preamble in CONFIGS:
            cases.append({"text": text, "levels": levels, "preamble": preamble,
                          "runs": [{"min": None, "max": None, "want": run(text, levels, preamble)}]})
    rng = random.Random(20240)
    for i in range(201):
        text = random_string(rng)
        levels, preamble = CONFIGS[i % 3]
        cases.append({"text": text, "levels": levels, "preamble": preamble,
                      "runs": [{"min": None, "max": None, "want": run(text, levels, preamble)}]})
    for i in range(20):
        text = synth_markdown(random.Random(500 + i), 600 + 40 * i)
        levels, preamble = CONFIGS[0] if i % 4 else CONFIGS[2]
        cases.append({"text": text, "levels": levels, "preamble": preamble,
                      "runs": [{"min": lo, "max": hi, "want_digest": digest(run(text, levels, preamble, lo, hi))} for lo, hi in SIZES]})

    class Recorder:
        enable_full_text = False

        def __init__(self):
            self.calls, self.positions = [], {}

        def add_vectors(self, ids, dense_vectors, sparse_vectors, texts, enhanced_texts, metadatas):
            pos = [self.positions.setdefault(i, len(self.positions)) for i in ids]
            self.calls.append(["add_vectors", {"ids": pos, "dense": list(dense_vectors), "sparse": list(sparse_vectors), "texts": list(texts),
                                               "enhanced_texts": list(enhanced_texts),
                                               "metadatas": [list(map(list, m.items())) for m in metadatas]}])

        def add_documents(self, documents):
            self.calls.append(["add_documents", [list(map(list, d.items())) for d in documents]])

    class Provider:
        def __init__(self, name, store):
            self.name, self.store = name, store

        def embed_batch(self, texts):
            self.store.calls.append([self.name, digest([(t, "") for t in texts])])   # the texts come again in add_vectors
            return [len(t) for t in texts]

    runs = []
    for kw in INDEX_RUNS:
        store = Recorder()
        idx = VerbatimIndex(vector_store=store, dense_provider=Provider("embed_dense", store), sparse_provider=Provider("embed_sparse", store),
                            chunker_provider=MarkdownChunkerProvider())
        docs = [Document(id=d["id"], title=d["title"], source=d["source"], content_type=DocumentType.MARKDOWN, raw_content=d["content"],
                         metadata=dict(d["metadata"])) for d in INDEX_DOCS]
        idx.add_documents_bulk(docs, **kw)
        runs.append({"kw": kw, "calls": store.calls})
    # ten small documents through the reference's index into THIS package's store (CPU stand-ins for its shards): what a
    # filter-only query per document and get_document return afterwards
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_reference_dropin as D

    D.cpu_stand_ins(setattr)
    store = D.vs.GpuVectorStore(dense_dim=64, sparse_vocab=300)
    small = [Document(id=f"doc-{i}", title=f"Doc {i}" if i % 3 else "", source=f"s{i}.md" if i % 2 else "", content_type=DocumentType.MARKDOWN,
                      raw_content=synth_markdown(random.Random(800 + i), 150 + 30 * i) if i != 7 else "",
                      metadata={"year": 2000 + i, "doc_type": "note"} if i % 4 else {}) for i in range(10)]
    VerbatimIndex(vector_store=store, dense_provider=D.Dense(), sparse_provider=D.Sparse(),
                  chunker_provider=MarkdownChunkerProvider()).add_documents_bulk(small, batch_chunks=7, batch_docs=4)
    stored = []
    for d in small:
        rows = store.query(top_k=1000, filter=f'metadata["document_id"] == "{d.id}"')
        stored.append({"document": {"id": d.id, "title": d.title, "source": d.source, "content": d.raw_content, "metadata": d.metadata},
                       "rows": [[r.text, r.enhanced_text, r.metadata] for r in rows], "record": store.get_document(d.id)})
    # the documents as the reference's Document class holds them (it names an untitled document after its source)
    documents = [{"id": d.id, "title": d.title, "source": d.source, "content": d.raw_content, "metadata": d.metadata} for d in docs]
    out = {"chunker": cases, "index": {"documents": documents, "content_type": "markdown", "runs": runs},
           "store": {"batch_chunks": 7, "batch_docs": 4, "content_type": "markdown", "documents": stored}}
    path = os.path.join(HERE, "chunker_fixtures.json")
    with open(path, "w") as f:
        json.dump(out, f, ensure_ascii=True, separators=(",", ":"))
    print(f"{path}: {os.path.getsize(path)} bytes, {len(cases)} chunker cases")


if __name__ == "__main__":
    main(sys.argv[1])
