"""Full-text (BM25) timings on one GPU: ingest rows/s (tokenise + index build of one batch), single-query latency and batched
query rate over a corpus of words drawn Zipf-like from a synthetic vocabulary.  Prints one JSON line.
usage: python tools/bench_full_text.py [--rows 1000000] [--words 300] [--reps 50] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import verbatim_rag_amd  # noqa: F401,E402
from verbatim_rag_amd import vector_stores as vs  # noqa: E402


def corpus(n_rows: int, mean_words: int, vocab: int, seed: int):
    """Rows of words drawn Zipf-like (exponent 1.1) from `vocab` synthetic lower-case words; word 0 ("common") is the head.
    Returns (texts, vocabulary)."""
    rng = np.random.default_rng(seed)
    alpha = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    words = {"common"}
    while len(words) < vocab:
        words.add("".join(alpha[rng.integers(0, 26, int(rng.integers(3, 10)))]))
    words = ["common"] + sorted(words - {"common"})
    p = 1.0 / np.arange(1, vocab + 1, dtype=np.float64) ** 1.1
    p /= p.sum()
    lens = rng.integers(max(1, mean_words // 2), mean_words * 3 // 2 + 1, n_rows)
    bounds = np.concatenate([[0], np.cumsum(lens)])
    box = np.array(words, dtype=object)
    texts = []
    for a in range(0, n_rows, 65536):                             # draw the word ids a slab of rows at a time
        b = min(n_rows, a + 65536)
        ids = rng.choice(vocab, size=int(bounds[b] - bounds[a]), p=p)
        for r in range(a, b):
            texts.append(" ".join(box[ids[bounds[r] - bounds[a]:bounds[r + 1] - bounds[a]]]))
    return texts, words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--words", type=int, default=300, help="mean words (tokens) per row")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    texts, words = corpus(a.rows, a.words, vocab=50000, seed=11)
    n_bytes = sum(len(t.encode("utf-8")) for t in texts)
    warm = vs.TextIndex()
    warm.add(texts[:1000], fold=True)
    warm.search(["common"], 5)
    warm.close()
    ix = vs.TextIndex()
    t0 = time.perf_counter()
    ix.add(texts, fold=True)
    ingest_s = time.perf_counter() - t0
    st = ix.stats()
    rng = np.random.default_rng(5)

    def queries(n):
        return [" ".join(words[int(j)] for j in rng.zipf(1.3, size=int(rng.integers(2, 6))) if j < len(words)) or words[1]
                for _ in range(n)]

    res = {"rows": a.rows, "mean_words": a.words, "tokens": st["sum_dl"], "postings": st["postings"], "text_mb": round(n_bytes / 2**20, 1),
           "ingest_s": round(ingest_s, 3), "ingest_rows_per_s": round(a.rows / ingest_s)}
    for nq, k in ((1, 10), (1, 100), (16, 10), (256, 10)):
        qs = [queries(nq) for _ in range(a.reps)]
        ix.search(qs[0], k)
        times = []
        for q in qs:
            t = time.perf_counter()
            ix.search(q, k)
            times.append(time.perf_counter() - t)
        med = float(np.median(times))
        res[f"q{nq}_k{k}_ms"] = round(med * 1e3, 3)
        res[f"q{nq}_k{k}_qps"] = round(nq / med)
    res["q1_common_ms"] = None
    t = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ix.search(["common"], 10)
        t.append(time.perf_counter() - t0)
    res["q1_common_ms"] = round(float(np.median(t)) * 1e3, 3)
    ix.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
