#!/usr/bin/env python3
"""ModernBERT cross-encoder reranking on a base-shape random-init checkpoint (ModernBERT-base encoder + the
ModernBertForSequenceClassification head, bf16 operands: the `GpuCrossEncoderReranker.from_directory` defaults), one JSON line:
  one_q_50x512_ms     -- `rerank` of one question's 50 pairs of 512 tokens (median wall time)
  batch_pairs_per_s   -- `rerank_batch` of --questions (64) questions x 50 pairs of 512 tokens
  one_q_50x2048_ms    -- `rerank` of 50 pairs of 2 048 tokens (separate attention kernel)
  head_share          -- the `head` profile class over all device time of one profiled `rerank_batch` pass (set_profiling on;
                         the timed passes run without events)
Texts are space-separated token ids, parsed before the timed passes (a shim tokenizer): host tokenisation stays out of the
numbers; pair packing and batching stay in."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class IdTokenizer:
    """Texts are space-separated ids, parsed once (`prime`); encode is then a lookup."""

    def __init__(self):
        self.cache = {}

    def prime(self, texts):
        for t in texts:
            self.cache[t] = [int(x) for x in t.split()]

    def encode(self, text, add_special_tokens=False):
        ids = self.cache.get(text)
        return ids if ids is not None else [int(x) for x in text.split()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--questions", type=int, default=64)
    ap.add_argument("--pooling", default="mean", choices=["cls", "mean"])
    args = ap.parse_args()
    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd.engine import EncoderEngine, ModernBertShape
    from verbatim_rag_amd.rerankers import GpuCrossEncoderReranker
    from verbatim_rag_amd.vector_stores import SearchResult
    from verbatim_rag_amd.weights import random_init

    shape = ModernBertShape.base()
    H = shape.hidden_size
    rng = np.random.default_rng(0)
    eng = EncoderEngine(shape, random_init(shape, 1234), max_tokens=65536, max_seqs=512, max_seq_len=2048, max_ranges=512,
                        operand_dtype="bf16")
    eng.set_seq_head((rng.standard_normal((H, H)) * H ** -0.5).astype(np.float32), (0.1 * rng.standard_normal(H)).astype(np.float32),
                     (1 + 0.1 * rng.standard_normal(H)).astype(np.float32), None,
                     (rng.standard_normal((1, H)) * H ** -0.5).astype(np.float32), np.zeros(1, np.float32), args.pooling)
    tok = IdTokenizer()
    rr = GpuCrossEncoderReranker(eng, tok, rerank_k=50, max_length=2048)

    def question():
        return " ".join(str(int(x)) for x in rng.integers(1000, 50000, 12))

    def results(pair_len):   # documents that pack to exactly pair_len tokens with a 12-token question
        return [SearchResult(id=str(j), score=0.0, metadata={}, text=" ".join(str(int(x)) for x in rng.integers(1000, 50000, pair_len - 15)))
                for j in range(50)]

    def median_ms(fn, iters):
        fn()
        fn()
        ts = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    q1, r512, r2048 = question(), results(512), results(2048)
    qs = [question() for _ in range(args.questions)]
    rs = [results(512) for _ in qs]
    tok.prime([q1] + qs + [r.text for r in r512 + r2048] + [r.text for x in rs for r in x])
    one_512 = median_ms(lambda: rr.rerank(q1, r512), args.iters)
    one_2048 = median_ms(lambda: rr.rerank(q1, r2048), max(3, args.iters // 2))
    batch_ms = median_ms(lambda: rr.rerank_batch(qs, rs), max(3, args.iters // 3))
    eng.set_profiling(True)
    eng.read_profile(reset=True)
    rr.rerank_batch(qs, rs)
    prof = eng.read_profile(reset=True)
    eng.set_profiling(False)
    total = sum(ms for ms, _n in prof.values())
    out = {"tool": "bench_rerank", "shape": "modernbert-base", "operands": "bf16", "pooling": args.pooling,
           "one_q_50x512_ms": round(one_512, 3),
           "questions": args.questions, "batch_pairs_per_s": round(args.questions * 50 / (batch_ms / 1e3), 1),
           "batch_ms": round(batch_ms, 2),
           "one_q_50x2048_ms": round(one_2048, 3),
           "head_ms": round(prof["head"][0], 3), "device_ms": round(total, 3),
           "head_share": round(prof["head"][0] / total, 5) if total else None}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
