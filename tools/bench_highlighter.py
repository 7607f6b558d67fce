"""API-level rate of the v2 highlighter format, host route against device route (`GpuModelSpanExtractor(highlighter_route=...)`), on
one engine of random ModernBERT-base-shaped weights with a 2-label token head (fp16 operands) and a byte-level BPE tokenizer.json
trained here on the synthetic texts (NFC, ByteLevel, runs of 2..24 spaces as added tokens).
  workload     256 questions x 5 chunks of about 400 tokens through `extract_spans_batch`
  host         HF `tokenizers` per (question, chunk) on the caller's thread, window logits read back, softmax + spans in Python
  device warm  contexts already in the chunk cache (they are known at ingest): device question ids, numpy packing, spans read back
  device cold  a fresh chunk cache every call: plus one `encode_batch_offsets` over the call's contexts
  engine only  load -> run -> token head of the same packed batches, nothing read back: the ceiling of both routes
5 timed repeats after 2 warm-ups per row, median and min..max, rows interleaved within one process.  Writes
profiles/highlighter_route_probe.txt."""
from __future__ import annotations

import argparse
import dataclasses
import os
import statistics
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEFAULT_OUT = os.path.join(ROOT, "profiles", "highlighter_route_probe.txt")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=256)
    ap.add_argument("--chunks", type=int, default=5)
    ap.add_argument("--chunk-tokens", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()

    import numpy as np
    import torch
    from tokenizers import Tokenizer

    import verbatim_rag_amd  # noqa: F401
    from bench_tokenize import synth_texts, synth_vocab, write_bpe_tokenizer
    from verbatim_rag_amd.bpe import GpuByteBpeTokenizer
    from verbatim_rag_amd.engine import EncoderEngine, ModernBertShape
    from verbatim_rag_amd.extractors import GpuModelSpanExtractor
    from verbatim_rag_amd.weights import random_init

    pieces = synth_vocab(8000)
    tmp = tempfile.mkdtemp()
    path = write_bpe_tokenizer(os.path.join(tmp, "tokenizer.json"), synth_texts(pieces, 400, 2500), 8000)
    hf_tok, gpu_tok = Tokenizer.from_file(path), GpuByteBpeTokenizer.from_file(path)
    # chunk texts cut to about --chunk-tokens tokens each; every (question, chunk) pair is distinct text
    n_pairs = args.questions * args.chunks
    raw = synth_texts(pieces, n_pairs, 6 * args.chunk_tokens, seed=3)
    chunks = []
    for t, enc in zip(raw, hf_tok.encode_batch(raw, add_special_tokens=False)):
        cut = enc.offsets[min(args.chunk_tokens, len(enc.ids)) - 1][1]
        chunks.append(t[:cut])
    n_ctx_tokens = sum(len(e.ids) for e in hf_tok.encode_batch(chunks, add_special_tokens=False))
    rng = np.random.default_rng(5)
    words = [p for p in pieces[5:] if not p.startswith("##") and len(p) > 2]
    questions = ["where is the " + " ".join(rng.choice(words, int(rng.integers(4, 9))).tolist()) + "?" for _ in range(args.questions)]
    results = [[types.SimpleNamespace(text=c) for c in chunks[q * args.chunks:(q + 1) * args.chunks]] for q in range(args.questions)]

    shape = dataclasses.replace(ModernBertShape.base(), cls_token_id=gpu_tok.cls_token_id, sep_token_id=gpu_tok.sep_token_id)
    weights = random_init(shape, seed=1234)
    eng = EncoderEngine(shape, weights, max_tokens=65536, max_seqs=512, max_seq_len=512, max_ranges=64, operand_dtype="f16")
    H = shape.hidden_size
    eng.set_token_head((rng.standard_normal((H, H)) * 0.02).astype(np.float32), np.ones(H, np.float32),
                       (rng.standard_normal((2, H)) * H ** -0.5).astype(np.float32), np.zeros(2, np.float32))
    kw = dict(model_format="highlighter", threshold=0.5, max_length=512, doc_stride=128)
    host = GpuModelSpanExtractor(engine=eng, tokenizer=hf_tok, **kw)
    dev = GpuModelSpanExtractor(engine=eng, tokenizer=gpu_tok, highlighter_route="device", **kw)

    # the packed batches of the device route, recorded once, for the engine-only row
    batches = []
    real = eng.load_packed
    eng.load_packed = lambda ids, lens, stream=None: batches.append((ids.copy(), lens.copy())) or real(ids, lens, stream)
    out_dev = dev.extract_spans_batch(questions, results)
    eng.load_packed = real
    out_host = host.extract_spans_batch(questions, results)
    n_tokens = int(sum(len(ids) for ids, _l in batches))
    agree = sum(a == b for a, b in zip(out_dev, out_host))

    def engine_only():
        for ids, lens in batches:
            eng.load_packed(ids, lens)
            eng.run()
            eng.run_token_head()
        torch.cuda.synchronize()

    def cold():
        dev._chunk_cache.clear()
        dev.extract_spans_batch(questions, results)

    rows = {"host route": lambda: host.extract_spans_batch(questions, results),
            "device route, warm chunk cache": lambda: dev.extract_spans_batch(questions, results),
            "device route, cold chunk cache": cold,
            "engine only (load + run + token head)": engine_only}
    times = {k: [] for k in rows}
    for rep in range(args.warmup + args.reps):
        for name, fn in rows.items():      # interleaved: drift of the machine hits every row alike
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times[name].append(dt)
    lines = [f"highlighter route probe: {args.questions} questions x {args.chunks} chunks = {n_pairs} pairs, {n_ctx_tokens / n_pairs:.0f} context "
             f"tokens per chunk, {n_tokens} packed tokens in {len(batches)} device batches; ModernBERT-base shape, random weights, fp16 operands",
             f"{args.reps} timed repeats after {args.warmup} warm-ups, rows interleaved; median [min .. max] seconds per call, chunks/s at the median",
             f"queries whose result dictionaries are equal between the routes (random weights, threshold 0.5; not a parity test): {agree} of "
             f"{args.questions}; device tokenizer fallbacks: {gpu_tok.fallback_count}"]
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"  {name:40s} {med:7.3f} [{min(ts):.3f} .. {max(ts):.3f}] s   {n_pairs / med:8.0f} chunks/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
