"""Glue between providers and the store for the hot path: the query dispatch of VerbatimIndex
(verbatim_rag/index.py:552-655), the batched embed-then-insert of chunks (:200-223,259-288; 2000-chunk embed batches) and the
bulk ingest of documents (`add_documents`, :128-198,225-257,290-316,340-411) in front of it: documents are chunked by a chunker
provider -- by default chunker_providers.GpuMarkdownChunker, whose structural pass runs on the device for a whole batch of
documents -- wrapped in the reference's document footer, embedded and stored.  The pydantic DocumentSchema flattening
(:73-126), the chonkie chunker and documents that bring their own chunks stay with the reference; `add_chunks` takes ready chunks.

The dispatch is one planning step (`_plan`) shared by the single-query and the cross-query entry points: it turns
(search_type, hybrid_weights, which providers exist) into "which providers embed the text" plus the keyword arguments the
store receives -- the contract pinned by the `index_query_trace` fixture, which records what the reference hands to
`VectorStore.query` for every combination.
"""
from __future__ import annotations

import uuid
from collections.abc import Mapping
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence

from .vector_stores import SearchResult, VectorStore

# search_type "auto": resolved from the providers the index was built with (index.py:609-619)
_AUTO = {(True, True): "hybrid", (True, False): "dense", (False, True): "sparse"}


@dataclass
class _Plan:
    embed_dense: bool = False
    embed_sparse: bool = False
    pass_text: bool = True                  # the store sees the query text (full-text capable stores use it)
    batchable: bool = False                 # the store's query_batch can answer it in one pass per method
    store_kwargs: Dict[str, Any] = field(default_factory=dict)


_FOOTER_SKIPS = {"user_id", "dataset_id", "userId"}   # never embedded (index.py:190-196)


@dataclass
class _Doc:
    """What add_documents reads from a document, whatever its type."""
    id: str
    title: str
    source: str
    content: str
    content_type: Optional[str]
    metadata: Dict[str, Any]

    @classmethod
    def of(cls, document: Any) -> "_Doc":
        def get(name, default=None):
            if isinstance(document, Mapping):
                return document.get(name, default)
            return getattr(document, name, default)

        if get("chunks"):
            raise ValueError("add_documents chunks the documents itself; pass documents that bring their own chunks to add_chunks")
        content = get("raw_content")
        if content is None:
            content = get("content")
        content_type = get("content_type")
        doc_id = get("id")
        return cls(id=str(uuid.uuid4()) if doc_id is None else doc_id, title=get("title") or "", source=get("source") or "",
                   content=content or "", content_type=getattr(content_type, "value", content_type), metadata=get("metadata") or {})

    def footer(self) -> str:
        """What follows the chunker's enhanced text in the embedded text (index.py:185-198)."""
        parts = ["", "", "---", f"Document: {self.title or 'Unknown'}"]
        if self.source:
            parts.append(f"Source: {self.source}")
        parts += [f"{key.replace('_', ' ').title()}: {value}" for key, value in self.metadata.items() if key not in _FOOTER_SKIPS]
        return "\n".join(parts)

    def chunk_metadata(self, number: int) -> Dict[str, Any]:
        """index.py:240-257, in that key order; the document's own metadata is laid over it."""
        return {"document_id": self.id, "title": self.title, "source": self.source, "doc_type": self.metadata.get("doc_type"),
                "content_type": self.content_type or None, "chunk_type": "paragraph", "chunk_number": number, "page_number": 0,
                **self.metadata}


class HotPathIndex:
    EMBED_BATCH = 2000  # index.py:343

    def __init__(self, vector_store: VectorStore, dense_provider=None, sparse_provider=None, chunker_provider=None):
        if dense_provider is None and sparse_provider is None:  # index.py:58-64
            if not bool(getattr(vector_store, "enable_full_text", False)):
                raise ValueError("At least one embedding provider (dense or sparse) must be provided")
        self.vector_store = vector_store
        self.dense_provider = dense_provider
        self.sparse_provider = sparse_provider
        self.chunker_provider = chunker_provider   # None: a GpuMarkdownChunker(), made by the first add_documents (index.py:69)

    # ------------------------------------------------------------------ ingest
    def _generate_embeddings(self, texts: List[str]):
        """index.py:200-223."""
        dense = self.dense_provider.embed_batch(texts) if self.dense_provider else None
        sparse = self.sparse_provider.embed_batch(texts) if self.sparse_provider else None
        return dense, sparse

    def add_chunks(self, ids: Sequence[str], texts: Sequence[str], enhanced_texts: Optional[Sequence[str]] = None,
                   metadatas: Optional[Sequence[Dict[str, Any]]] = None) -> None:
        """Embeddings are computed on the *enhanced* text, raw text is stored for extraction
        (index.py:152-164,470-486)."""
        enhanced_texts = list(enhanced_texts) if enhanced_texts is not None else list(texts)
        metadatas = list(metadatas) if metadatas is not None else [{} for _ in ids]
        for a in range(0, len(ids), self.EMBED_BATCH):
            b = min(len(ids), a + self.EMBED_BATCH)
            dense, sparse = self._generate_embeddings(enhanced_texts[a:b])
            self.vector_store.add_vectors(list(ids[a:b]), dense, sparse, list(texts[a:b]), enhanced_texts[a:b],
                                          metadatas[a:b])

    def _chunk_documents(self, texts: List[str]) -> List[List[Any]]:
        if self.chunker_provider is None:
            from .chunker_providers import GpuMarkdownChunker

            self.chunker_provider = GpuMarkdownChunker()
        batch = getattr(self.chunker_provider, "chunk_batch", None)
        return batch(texts) if batch is not None else [self.chunker_provider.chunk(t) for t in texts]

    def add_documents(self, documents: Iterable[Any], batch_chunks: int = 2000, batch_docs: int = 500,
                      id_factory: Optional[Callable[[], str]] = None) -> None:
        """Documents in, stored rows out: VerbatimIndex.add_documents_bulk (index.py:340-411) with the chunker called once per
        `batch_docs` documents (`chunk_batch`: one device call for the default chunker).  A document is a mapping or an object
        with id, title, source, raw_content (or content), metadata and optionally content_type; one that brings its own chunks
        belongs to `add_chunks`.  Chunks are embedded (enhanced text) and inserted as soon as `batch_chunks` of them have
        gathered, in the middle of a document if need be; the document records go to the store's `add_documents`, if it has
        one, once per `batch_docs` documents, deduplicated by id."""
        new_id = id_factory or (lambda: str(uuid.uuid4()))
        ids: List[str] = []
        texts: List[str] = []
        enhanced_texts: List[str] = []
        metadatas: List[Dict[str, Any]] = []

        def flush_chunks():
            if ids:
                dense, sparse = self._generate_embeddings(enhanced_texts)
                self.vector_store.add_vectors(list(ids), dense, sparse, list(texts), list(enhanced_texts), list(metadatas))
                for column in (ids, texts, enhanced_texts, metadatas):
                    column.clear()

        def flush_documents(docs: List["_Doc"]):
            records: Dict[str, Dict[str, Any]] = {}
            for doc in docs:
                records.setdefault(doc.id, {"id": doc.id, "title": doc.title, "source": doc.source, "content_type": doc.content_type,
                                            "raw_content": "", "metadata": doc.metadata})
            if records and hasattr(self.vector_store, "add_documents"):   # index.py:299-316
                self.vector_store.add_documents(list(records.values()))

        group: List[_Doc] = []

        def flush_group(last: bool = False):
            chunked = self._chunk_documents([doc.content for doc in group]) if group else []
            for doc, chunks in zip(group, chunked):
                footer = doc.footer()
                head = f"# {doc.title}\n\n\n" if doc.title else ""
                for number, (raw, enhanced) in enumerate(chunks):
                    ids.append(new_id())
                    texts.append(raw)
                    enhanced_texts.append(head + enhanced + footer)
                    metadatas.append(doc.chunk_metadata(number))
                    if len(ids) >= batch_chunks:
                        flush_chunks()
            if last:                        # the reference stores the last chunks before the last document records
                flush_chunks()
            flush_documents(group)
            group.clear()

        for document in documents:
            group.append(_Doc.of(document))
            if len(group) >= batch_docs:
                flush_group()
        flush_group(last=True)

    # ------------------------------------------------------------------ query dispatch
    def _plan(self, search_type: str, filter, search_params, hybrid_weights, rrf_k) -> _Plan:
        common = {"filter": filter, "search_params": search_params}
        have_d, have_s = bool(self.dense_provider), bool(self.sparse_provider)
        if hybrid_weights is not None:      # the weights name the methods; search_type is ignored (index.py:590-607)
            return _Plan(embed_dense="dense" in hybrid_weights and have_d, embed_sparse="sparse" in hybrid_weights and have_s,
                         batchable=True, store_kwargs={**common, "hybrid_weights": hybrid_weights, "rrf_k": rrf_k})
        if search_type == "auto":
            search_type = _AUTO.get((have_d, have_s))
            if search_type is None:
                if not getattr(self.vector_store, "enable_full_text", False):
                    raise ValueError("No search method available")
                search_type = "full_text"
        if search_type == "full_text":      # no embeddings, no rrf_k (index.py:622-631); the store's query_batch answers a batch
            return _Plan(batchable=True, store_kwargs={**common, "search_type": "full_text"})
        return _Plan(embed_dense=search_type in ("dense", "hybrid") and have_d,
                     embed_sparse=search_type in ("sparse", "hybrid") and have_s,
                     batchable=search_type in ("dense", "sparse", "hybrid"),
                     store_kwargs={**common, "search_type": search_type, "rrf_k": rrf_k})

    def query(self, text: Optional[str] = None, k: int = 5, search_type: str = "auto", filter: Optional[str] = None,
              search_params: Optional[Dict[str, Any]] = None, hybrid_weights: Optional[Dict[str, float]] = None,
              rrf_k: int = 60) -> List[SearchResult]:
        """Same hand-off to the store as the reference's VerbatimIndex.query (index.py:552-655)."""
        if not text:                        # browse / filter-only (index.py:579-588)
            return self.vector_store.query(dense_query=None, sparse_query=None, text_query=None, top_k=k, filter=filter,
                                           search_params=search_params)
        plan = self._plan(search_type, filter, search_params, hybrid_weights, rrf_k)
        dense = self.dense_provider.embed_text(text) if plan.embed_dense else None
        sparse = self.sparse_provider.embed_text(text) if plan.embed_sparse else None
        return self.vector_store.query(dense_query=dense, sparse_query=sparse, text_query=text, top_k=k, **plan.store_kwargs)

    # ------------------------------------------------------------------ cross-query batching
    @staticmethod
    def _embed_queries(provider, texts: List[str]):
        fn = getattr(provider, "embed_queries", None)
        return fn(texts) if fn is not None else [provider.embed_text(t) for t in texts]

    def query_batch(self, texts: Sequence[str], k: int = 5, search_type: str = "auto", filter: Optional[str] = None,
                    search_params: Optional[Dict[str, Any]] = None, hybrid_weights: Optional[Dict[str, float]] = None,
                    rrf_k: int = 60) -> List[List[SearchResult]]:
        """`[query(t, k, ...) for t in texts]` for many concurrent queries: the query embeddings go through the
        providers as shared batches (`embed_queries` when the provider has it) and the store answers them in one
        `query_batch` call when it has one; anything else takes `query`, one text at a time."""
        texts = list(texts)
        store_batch = getattr(self.vector_store, "query_batch", None)
        one_by_one = store_batch is None or not texts or any(not t for t in texts)
        plan = None if one_by_one else self._plan(search_type, filter, search_params, hybrid_weights, rrf_k)
        if plan is None or not plan.batchable:
            return [self.query(t, k, search_type, filter, search_params, hybrid_weights, rrf_k) for t in texts]
        dense = self._embed_queries(self.dense_provider, texts) if plan.embed_dense else None
        sparse = self._embed_queries(self.sparse_provider, texts) if plan.embed_sparse else None
        return store_batch(dense_queries=dense, sparse_queries=sparse, text_queries=texts, top_k=k, **plan.store_kwargs)
