"""Text -> ids throughput of the BERT WordPiece pipeline, three ways on one machine, plus `GpuDenseProvider.embed_batch` from text
with `tokenizer="host"` and `"gpu"`: 2 000 synthetic ~2.5 KB texts over a synthetic 30 522-piece vocabulary.
  per_text_loop   `TokenizerAdapter.ids` once per text (what the providers did)
  hf_encode_batch HF `tokenizers` encode_batch on 16 threads
  device          `GpuWordPieceTokenizer.encode_batch`: host->device copy of the text, kernels, device->host copy of the ids
Writes profiles/wordpiece_bench.json (median of `--reps` runs after one warm-up).
`--bpe`: the same three baselines for the byte-level BPE pipeline of the ModernBERT checkpoints (`GpuByteBpeTokenizer`) over a
BPE vocabulary trained here on the synthetic texts, NFC + space-run tokens 2..24; writes profiles/bpe_bench.json."""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import string
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "wordpiece_bench.json")


def synth_vocab(n: int, seed: int = 0):
    rng = random.Random(seed)
    pieces = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    seen = set(pieces)
    for ch in string.ascii_lowercase + string.digits + string.punctuation:
        for p in (ch, "##" + ch):
            seen.add(p)
            pieces.append(p)
    while len(pieces) < n:
        w = "".join(rng.choice(string.ascii_lowercase) for _ in range(rng.randint(2, 10)))
        p = w if rng.random() < 0.75 else "##" + w
        if p not in seen:
            seen.add(p)
            pieces.append(p)
    return pieces


def write_tokenizer(path: str, pieces) -> str:
    """A bert-base-uncased style tokenizer.json over `pieces`."""
    vocab = {p: i for i, p in enumerate(pieces)}
    special = lambda t: {"SpecialToken": {"id": t, "type_id": 0}}      # noqa: E731
    spec = {
        "version": "1.0", "truncation": None, "padding": None,
        "added_tokens": [{"id": vocab[t], "content": t, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
                          "special": True} for t in pieces[:5]],
        "normalizer": {"type": "BertNormalizer", "clean_text": True, "handle_chinese_chars": True, "strip_accents": None, "lowercase": True},
        "pre_tokenizer": {"type": "BertPreTokenizer"},
        "post_processor": {"type": "TemplateProcessing", "single": [special("[CLS]"), {"Sequence": {"id": "A", "type_id": 0}}, special("[SEP]")],
                           "pair": [special("[CLS]"), {"Sequence": {"id": "A", "type_id": 0}}, special("[SEP]"),
                                    {"Sequence": {"id": "B", "type_id": 1}}, {"SpecialToken": {"id": "[SEP]", "type_id": 1}}],
                           "special_tokens": {t: {"id": t, "ids": [vocab[t]], "tokens": [t]} for t in ("[CLS]", "[SEP]")}},
        "decoder": {"type": "WordPiece", "prefix": "##", "cleanup": True},
        "model": {"type": "WordPiece", "unk_token": "[UNK]", "continuing_subword_prefix": "##", "max_input_chars_per_word": 100, "vocab": vocab},
    }
    with open(path, "w", encoding="utf-8") as f:
        json.dump(spec, f, ensure_ascii=False)
    return path


def synth_texts(pieces, n: int, n_bytes: int, seed: int = 1):
    rng = random.Random(seed)
    words = [p for p in pieces[5:] if not p.startswith("##") and len(p) > 1]
    tails = [p[2:] for p in pieces if p.startswith("##") and len(p) > 3]
    texts = []
    for _ in range(n):
        out, size = [], 0
        while size < n_bytes:
            w = rng.choice(words)
            r = rng.random()
            if r < 0.3:
                w += rng.choice(tails)
            elif r < 0.35:
                w = w.capitalize()
            elif r < 0.4:
                w += rng.choice(",.;!?")
            out.append(w)
            size += len(w) + 1
        texts.append(" ".join(out))
    return texts


def write_bpe_tokenizer(path: str, texts, vocab_size: int) -> str:
    """A ModernBERT-style tokenizer.json (NFC, ByteLevel, BPE, runs of 2..24 spaces as added tokens) trained on `texts`."""
    from tokenizers import AddedToken, Tokenizer, models, normalizers, pre_tokenizers, processors, trainers

    tok = Tokenizer(models.BPE())
    tok.normalizer = normalizers.NFC()
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    tok.train_from_iterator(texts, trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"],
                                                       initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False))
    tok.add_tokens([AddedToken(" " * n, normalized=True) for n in range(2, 25)])
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                                       special_tokens=[("[CLS]", 2), ("[SEP]", 3)])
    tok.save(path)
    return path


def bench_bpe(args) -> int:
    import numpy as np
    from tokenizers import Tokenizer

    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd.bpe import GpuByteBpeTokenizer
    from verbatim_rag_amd.packing import TokenizerAdapter

    rng = random.Random(2)
    texts = []
    for t in synth_texts(synth_vocab(30522), args.texts, args.bytes):      # contractions, double spaces and newlines as real text has them
        words = t.split(" ")
        texts.append("".join(w + rng.choice(["'s", "'re", "", "", "", ""]) + rng.choice([" "] * 12 + ["  ", "\n", ". "]) for w in words))
    with tempfile.TemporaryDirectory() as tmp:
        path = write_bpe_tokenizer(os.path.join(tmp, "tokenizer.json"), texts[:200], args.vocab)
        hf = Tokenizer.from_file(path)
        gpu = GpuByteBpeTokenizer.from_file(path)
    adapter = TokenizerAdapter(hf, sep_token_id=3, cls_token_id=2)
    want = [adapter.ids(t, add_special_tokens=True, max_length=512) for t in texts]
    ids, lens = gpu.encode_batch(texts)
    assert ids.tolist() == [i for w in want for i in w] and gpu.fallback_count == 0, "device ids differ from HF's"
    res = {"pipeline": "NFC + ByteLevel + BPE", "texts": len(texts), "mean_text_bytes": sum(len(t) for t in texts) / len(texts),
           "vocab": gpu.vocab_size, "max_length": 512, "mean_ids_per_text": float(np.mean(lens)), "reps": args.reps,
           "hf_threads": os.environ["RAYON_NUM_THREADS"], "ms": {}}
    res["ms"]["per_text_loop"] = median_ms(lambda: [adapter.ids(t, add_special_tokens=True, max_length=512) for t in texts], args.reps)
    res["ms"]["hf_encode_batch"] = median_ms(lambda: hf.encode_batch(texts, add_special_tokens=False), args.reps)
    res["ms"]["device"] = median_ms(lambda: gpu.encode_batch(texts), args.reps)
    res["ms"]["device_ids_as_lists"] = median_ms(lambda: gpu.ids_batch(texts, max_length=512, add_special_tokens=True), args.reps)
    res["texts_per_s"] = {k: len(texts) / (v / 1e3) for k, v in res["ms"].items()}
    gpu.close()
    out = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "bpe_bench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


def median_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=2000)
    ap.add_argument("--bytes", type=int, default=2500)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--bpe", action="store_true", help="the byte-level BPE pipeline instead (profiles/bpe_bench.json)")
    args = ap.parse_args()
    os.environ.setdefault("RAYON_NUM_THREADS", "16")
    if args.bpe:
        return bench_bpe(args)
    import numpy as np
    from tokenizers import Tokenizer

    import verbatim_rag_amd  # noqa: F401
    from verbatim_rag_amd.embedding_providers import GpuDenseProvider
    from verbatim_rag_amd.engine import BertEncoderEngine, BertShape
    from verbatim_rag_amd.packing import TokenizerAdapter
    from verbatim_rag_amd.weights import random_init_bert
    from verbatim_rag_amd.wordpiece import GpuWordPieceTokenizer

    pieces = synth_vocab(args.vocab)
    texts = synth_texts(pieces, args.texts, args.bytes)
    with tempfile.TemporaryDirectory() as tmp:
        path = write_tokenizer(os.path.join(tmp, "tokenizer.json"), pieces)
        hf = Tokenizer.from_file(path)
        gpu = GpuWordPieceTokenizer.from_file(path)
    adapter = TokenizerAdapter(hf, sep_token_id=3, cls_token_id=2)
    want = [adapter.ids(t, add_special_tokens=True, max_length=512) for t in texts]
    ids, lens = gpu.encode_batch(texts)
    assert ids.tolist() == [i for w in want for i in w] and gpu.fallback_count == 0, "device ids differ from HF's"
    res = {"texts": len(texts), "mean_text_bytes": sum(len(t) for t in texts) / len(texts), "vocab": len(pieces), "max_length": 512,
           "mean_ids_per_text": float(np.mean(lens)), "reps": args.reps, "hf_threads": os.environ["RAYON_NUM_THREADS"], "ms": {}}
    res["ms"]["per_text_loop"] = median_ms(lambda: [adapter.ids(t, add_special_tokens=True, max_length=512) for t in texts], args.reps)
    res["ms"]["hf_encode_batch"] = median_ms(lambda: hf.encode_batch(texts, add_special_tokens=False), args.reps)
    res["ms"]["device"] = median_ms(lambda: gpu.encode_batch(texts), args.reps)
    res["ms"]["device_ids_as_lists"] = median_ms(lambda: gpu.ids_batch(texts, max_length=512, add_special_tokens=True), args.reps)
    shape = BertShape(vocab_size=len(pieces), hidden_size=384, num_hidden_layers=6, num_attention_heads=12, intermediate_size=1536,
                      max_position_embeddings=512, norm_eps=1e-12, pad_token_id=0, cls_token_id=2, sep_token_id=3, model_type="bert")
    eng = BertEncoderEngine(shape, random_init_bert(shape, mlm=False), max_tokens=65536, max_seqs=512, max_seq_len=512, max_ranges=512)
    rows = {}
    for name, tok in (("host", hf), ("gpu", gpu)):
        prov = GpuDenseProvider(eng, tok, pooling="mean")
        rows[name] = np.asarray(prov.embed_batch(texts[:64]))
        res["ms"][f"embed_batch_tokenizer_{name}"] = median_ms(lambda: prov.embed_batch(texts), max(2, args.reps // 2))
    assert np.array_equal(rows["host"], rows["gpu"])
    res["texts_per_s"] = {k: len(texts) / (v / 1e3) for k, v in res["ms"].items()}
    eng.close()
    gpu.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
