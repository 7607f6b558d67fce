"""GPU cross-encoder reranker behind the reference's `Reranker` interface.

Kept: `Reranker.rerank(question, results) -> List[SearchResult]` / `rerank_async`, `BaseReranker`'s `rerank_k` /
`text_field` handling and the head/tail split (verbatim_rag/rerankers.py:14-41), the ordering rule of
`SentenceTransformersReranker.rerank` (`sorted(zip(scores, head), reverse=True)`, :128-134); the caller is
`VerbatimRAG._apply_reranker` (verbatim_rag/core.py:125-140).  Replaced: sentence-transformers `CrossEncoder.predict`
(third-party, absent here) by the HIP encoders on packed `[CLS] q [SEP] d [SEP]` pairs: the BERT-family encoder +
pooler/classifier head with token types 0 / 1 (`cross-encoder/ms-marco-MiniLM-L-6-v2` is a 6-layer, 384-wide, 12-head
BERT: head_dim 32, run on the head_dim-64 kernels with zero-padded heads), or the ModernBERT encoder + the
ModernBertForSequenceClassification head (cls / mean pooling, dense, GELU, LayerNorm, classifier; e.g.
`gte-reranker-modernbert-base`, 8 192-token context).  Scores are the classifier logits; CrossEncoder applies a monotone
activation (identity or sigmoid) to a single label, which does not change the order.  `rerank_batch` reranks several
questions' results through shared device batches (the serving path of `StaticVerbatimPipeline.query_batch`).
"""
from __future__ import annotations

import asyncio
from abc import ABC, abstractmethod
from typing import Any, List, Optional, Sequence, Tuple

from .checked_engine import CheckedEngines, greedy_batches

# Longest sequence the fused QKV + attention kernel takes (csrc/qkv_attn.h kFusedMaxSeq): a device batch holding one longer
# sequence runs every layer on the separate attention kernel, so rerank_batch never mixes the two lengths in one batch.
FUSED_ATTENTION_MAX_LEN = 512


class Reranker(ABC):
    @abstractmethod
    def rerank(self, question: str, results: List[Any]) -> List[Any]:
        raise NotImplementedError

    async def rerank_async(self, question: str, results: List[Any]) -> List[Any]:
        return await asyncio.to_thread(self.rerank, question, results)


class BaseReranker(Reranker):
    def __init__(self, rerank_k: int = 50, text_field: str = "text"):
        self.rerank_k = rerank_k
        self.text_field = text_field

    def _split_results(self, results: List[Any]):
        return results[: self.rerank_k], results[self.rerank_k:]

    def _get_texts(self, results: List[Any]) -> List[str]:
        if self.text_field == "enhanced_text":
            return [r.enhanced_text or r.text for r in results]
        return [r.text for r in results]


def pack_pair(q_ids: Sequence[int], d_ids: Sequence[int], cls_id: int, sep_id: int, max_length: int) -> Tuple[List[int], List[int]]:
    """`[CLS] q [SEP] d [SEP]` with token types 0 / 1, truncated to `max_length` the way HF fast tokenizers truncate a
    pair with `truncation=True` (strategy `longest_first`, tokenizers `utils/truncation.rs`): with budget =
    max_length - 3 special tokens, the shorter side keeps min(len, budget // 2 when both overflow) and the longer side
    takes the rest; on equal lengths the first sequence counts as the shorter one."""
    n1, n2 = len(q_ids), len(d_ids)
    budget = max_length - 3
    if n1 + n2 > budget:
        swap = n1 > n2
        if swap:
            n1, n2 = n2, n1
        n2 = n1 if n1 > budget else max(n1, budget - n1)
        if n1 + n2 > budget:
            n1 = budget // 2
            n2 = n1 + budget % 2
        if swap:
            n1, n2 = n2, n1
    q, d = list(q_ids[:n1]), list(d_ids[:n2])
    ids = [cls_id] + q + [sep_id] + d + [sep_id]
    types = [0] * (len(q) + 2) + [1] * (len(d) + 1)
    return ids, types


class GpuCrossEncoderReranker(BaseReranker):
    """SentenceTransformersReranker (verbatim_rag/rerankers.py:109-134) on a `BertEncoderEngine` with a pair head or an
    `EncoderEngine` (ModernBERT) with a sequence-classification head: both expose `pair_labels` and
    `pair_logits(sequences, type_ids)`.  Every `pair_logits` call goes through `CheckedEngines.run` (checked_engine.py): an
    fp16 engine that clamped an operand is replaced by a bf16 one and the batch scored again when `from_directory` built
    it; a reranker that was handed its engine raises instead of returning clamped scores."""

    def __init__(self, engine: Any, tokenizer: Any, rerank_k: int = 50, text_field: str = "text", max_length: int = 512):
        super().__init__(rerank_k=rerank_k, text_field=text_field)
        if not getattr(engine, "pair_labels", 0):
            raise ValueError("engine has no pair head (BertForSequenceClassification / ModernBertForSequenceClassification weights)")
        self.tokenizer = tokenizer
        self._max_length = max_length
        self._checked = CheckedEngines([engine], on_swap=self._bind)    # from_directory adds the bf16 rebuild
        self._bind()

    def _bind(self) -> None:
        """What the reranker keeps of its engine; derived again when the engine is replaced."""
        self.engine = self._checked.engines[0]
        self.max_length = min(self._max_length, self.engine.max_seq_len)

    @classmethod
    def from_directory(cls, model_path: str, device: int = 0, rerank_k: int = 50, max_length: Optional[int] = None,
                       operand_dtype: Optional[str] = None, tokenizer: str = "host", **kw) -> "GpuCrossEncoderReranker":
        """`SentenceTransformersReranker(model_name)` (rerankers.py:109-134) for a checkpoint on disk: a
        `BertForSequenceClassification` (e.g. a downloaded `cross-encoder/ms-marco-MiniLM-L-6-v2`; defaults: 512 tokens,
        the loader's fp16 operands) or a `ModernBertForSequenceClassification` (e.g. `gte-reranker-modernbert-base`;
        defaults: the checkpoint's `max_position_embeddings` as CrossEncoder takes it, bf16 operands -- a pooled logit feeds
        an ordering, like the sentence classifier's).  `tokenizer="gpu"`: WordPiece (BERT checkpoints)
        or byte-level BPE (ModernBERT checkpoints) on the device, same ids."""
        import json
        import os

        from .embedding_providers import load_checked_directory

        with open(os.path.join(model_path, "config.json")) as f:
            cfg = json.load(f)
        load_kw = {}
        if cfg.get("model_type") == "modernbert":
            max_length = max_length or int(cfg.get("max_position_embeddings", 8192))
            load_kw["operand_dtype"] = operand_dtype or "bf16"
        else:
            max_length = max_length or 512
            if operand_dtype:
                load_kw["operand_dtype"] = operand_dtype
        engine, tokenizer, rebuild = load_checked_directory(model_path, device=device, max_seq_len=max_length, tokenizer=tokenizer, **load_kw)
        self = cls(engine, tokenizer, rerank_k=rerank_k, max_length=max_length, **kw)
        self._checked.rebuild = rebuild
        return self

    def _ids(self, text: str) -> List[int]:
        enc = self.tokenizer.encode(text, add_special_tokens=False)
        return list(enc.ids if hasattr(enc, "ids") else enc)

    def _ids_batch(self, texts: Sequence[str]) -> List[List[int]]:
        """`[_ids(t) for t in texts]`; one device batch when the tokenizer is a device tokenizer."""
        from .device_tokenizer import DeviceTokenizer

        if isinstance(self.tokenizer, DeviceTokenizer):
            return self.tokenizer.ids_batch(list(texts), max_length=2 ** 31 - 1, add_special_tokens=False)
        return [self._ids(t) for t in texts]

    def score(self, question: str, texts: Sequence[str]) -> List[float]:
        sh = self.engine.shape
        q, *docs = self._ids_batch([question, *texts])
        packed = [pack_pair(q, d, sh.cls_token_id, sh.sep_token_id, self.max_length) for d in docs]
        scores: List[float] = []
        for start, end in greedy_batches([len(p[0]) for p in packed], self.engine.max_seqs, self.engine.max_tokens):
            if end == start:
                raise ValueError("a single pair exceeds the engine workspace")
            scores.extend(float(x) for x in self._pair_logits(packed, range(start, end))[:, 0])
        return scores

    def _pair_logits(self, packed: List[Tuple[List[int], List[int]]], idx: Sequence[int]):
        """One device batch, `packed[i] for i in idx`, on the current engine with the fp16 clamp report honoured."""
        ids, types = [packed[i][0] for i in idx], [packed[i][1] for i in idx]
        return self._checked.run(lambda engine: engine.pair_logits(ids, types))

    def rerank(self, question: str, results: List[Any]) -> List[Any]:
        head, tail = self._split_results(results)
        if not head:
            return results
        scores = self.score(question, self._get_texts(head))
        ranked = [r for _, r in sorted(zip(scores, head), reverse=True)]   # rerankers.py:133
        return ranked + tail

    def _device_batches(self, packed: List[Tuple[List[int], List[int]]]) -> List[List[int]]:
        """Indices of `packed` in device batches: ordered by packed length (similar lengths share a batch), cut at the
        engine's max_seqs / max_tokens, and at the fused-attention limit -- pairs longer than FUSED_ATTENTION_MAX_LEN
        go to batches of their own, so one long pair never pushes a batch of short ones off the fused kernel."""
        order = sorted(range(len(packed)), key=lambda i: len(packed[i][0]))
        batches: List[List[int]] = []
        cur: List[int] = []
        tok = 0
        for i in order:
            n = len(packed[i][0])
            if n > self.engine.max_tokens:
                raise ValueError("a single pair exceeds the engine workspace")
            crosses = bool(cur) and len(packed[cur[-1]][0]) <= FUSED_ATTENTION_MAX_LEN < n
            if cur and (crosses or len(cur) >= self.engine.max_seqs or tok + n > self.engine.max_tokens):
                batches.append(cur)
                cur, tok = [], 0
            cur.append(i)
            tok += n
        if cur:
            batches.append(cur)
        return batches

    def score_batch(self, questions: Sequence[str], texts_per_question: Sequence[Sequence[str]]) -> List[List[float]]:
        """`[score(q, texts) for q, texts in ...]` with every question's pairs in shared device batches (`_device_batches`)."""
        questions, texts_per_question = list(questions), list(texts_per_question)
        if len(questions) != len(texts_per_question):
            raise ValueError(f"{len(questions)} questions but {len(texts_per_question)} result lists")
        sh = self.engine.shape
        packed, owner = [], []
        for qi, (question, texts) in enumerate(zip(questions, texts_per_question)):
            if not texts:
                continue
            q, *docs = self._ids_batch([question, *texts])
            for d in docs:
                packed.append(pack_pair(q, d, sh.cls_token_id, sh.sep_token_id, self.max_length))
                owner.append(qi)
        scores = [0.0] * len(packed)
        for idx in self._device_batches(packed):
            for i, x in zip(idx, self._pair_logits(packed, idx)[:, 0]):
                scores[i] = float(x)
        per_q: List[List[float]] = [[] for _ in questions]
        for qi, sc in zip(owner, scores):
            per_q[qi].append(sc)
        return per_q

    def rerank_batch(self, questions: Sequence[str], results_per_question: Sequence[List[Any]]) -> List[List[Any]]:
        """`[rerank(q, r) for q, r in zip(questions, results_per_question)]` -- same `rerank_k` head / tail split,
        `text_field` and ordering rule -- with every question's pairs scored in shared device batches."""
        results_per_question = list(results_per_question)
        splits = [self._split_results(results) for results in results_per_question]
        per_q = self.score_batch(questions, [self._get_texts(head) for head, _tail in splits])
        out = []
        for results, (head, tail), sc in zip(results_per_question, splits, per_q):
            if not head:
                out.append(results)
                continue
            out.append([r for _, r in sorted(zip(sc, head), reverse=True)] + tail)   # rerankers.py:133
        return out
