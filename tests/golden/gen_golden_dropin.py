#!/usr/bin/env python3
"""Generates tests/golden/dropin_fixtures.json by running the REFERENCE's own `VerbatimIndex` and `VerbatimRAG` over this
package's store / providers / extractor (CPU stand-ins, the corpora of tests/test_reference_dropin.py).  Nothing of the
reference travels: only what its pipeline returned, and the calls it made into this package's store and extractor (method,
arguments, result), are written.  Run where a reference checkout is present:
`python tests/golden/gen_golden_dropin.py <reference checkout>`.  `rapidfuzz` / `openai` are stubbed as in gen_golden.py."""
from __future__ import annotations

import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(ref: str) -> None:
    import gen_golden

    gen_golden.REF = os.path.abspath(ref)
    gen_golden._install_stubs()
    from verbatim_rag.core import VerbatimRAG
    from verbatim_rag.index import VerbatimIndex

    import test_reference_dropin as D
    from verbatim_rag_amd.rerankers import GpuCrossEncoderReranker

    D.cpu_stand_ins(setattr)
    out = {}
    store, _ours, ext = D.corpus(30, document_ids=True)
    theirs = VerbatimIndex(vector_store=store, dense_provider=D.Dense(), sparse_provider=D.Sparse())
    out["index_queries"] = [{"kw": kw, "results": D.hits(theirs.query(**kw))} for kw in D.INDEX_QUERIES]
    rag = VerbatimRAG(index=theirs, k=5, extractor=ext, template_mode="static", llm_client=types.SimpleNamespace())
    out["pipeline_k5"] = {q: rag.query(q).model_dump() for q in D.QUESTIONS}

    store, _ours, ext = D.corpus(20, document_ids=False)
    theirs = VerbatimIndex(vector_store=store, dense_provider=D.Dense(), sparse_provider=D.Sparse())
    rag = VerbatimRAG(index=theirs, k=4, extractor=ext, template_mode="static", llm_client=types.SimpleNamespace())
    out["pipeline_k4"] = rag.query(D.QUESTIONS[0]).model_dump()
    rr = GpuCrossEncoderReranker(D.PairEngine(), ext.tokenizer, rerank_k=3)
    rag = VerbatimRAG(index=theirs, k=4, extractor=ext, template_mode="static", llm_client=types.SimpleNamespace(), reranker=rr)
    out["pipeline_k4_reranked"] = rag.query(D.QUESTIONS[0]).model_dump()

    from verbatim_core.transform import VerbatimTransform
    from verbatim_rag.providers import IndexProvider

    seen = D.Recorder(ext)
    tr = VerbatimTransform(llm_client=types.SimpleNamespace(), extractor=seen, template_mode="static")
    docs = D.tower_docs(2)
    tr.transform(D.QUESTIONS[0], [{"content": docs[0], "title": "T0", "source": "s0"}, {"text": docs[1]}])
    tr.transform(D.QUESTIONS[0], IndexProvider(theirs).retrieve(D.QUESTIONS[0], k=3))
    out["transform_extract_calls"] = seen.calls

    from verbatim_rag.schema import DocumentSchema

    store = D.Recorder(D.vs.GpuVectorStore(dense_dim=64, sparse_vocab=300))
    idx = VerbatimIndex(vector_store=store, dense_provider=D.Dense(), sparse_provider=D.Sparse())
    idx.add_documents([DocumentSchema(content=f"# Title {i}\n\nThe tower number {i} is tall. It stands in city {i}.\n\n## Section\n\n"
                                              f"Visitors climb {i + 3} stairs!", title=f"Doc {i}", source=f"s{i}.md") for i in range(6)])
    doc_id = idx.query(text="The tower is tall", k=4)[0].metadata["document_id"]
    idx.query(text="The tower is tall", k=10, filter=f'metadata["document_id"] == "{doc_id}"')
    idx.get_all_chunks(limit=5)
    idx.get_all_documents(limit=3)
    idx.get_chunks_by_document(doc_id)
    idx.inspect()
    idx.get_document(doc_id)
    idx.get_document("nope")
    out["ingest"] = {"document_id": doc_id, "calls": store.calls}
    assert "verbatim_rag.index" in sys.modules
    with open(os.path.join(HERE, "dropin_fixtures.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
