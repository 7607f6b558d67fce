"""The v2 highlighter's device route against its host route on the tiny encoder: same engine, same synthetic byte-level
tokenizer.json -- `tokenizers.Tokenizer` on the host route, `GpuByteBpeTokenizer` on the device route."""
import os
import types

import numpy as np
import pytest

from bpe_cases import VARIANTS, write_tokenizer
from oracle import modernbert_np as O
from test_heads_gpu import TINY

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
KW = dict(model_format="highlighter", max_length=128, doc_stride=16, min_span_chars=5, merge_gap_chars=3)
CTXS = [" ".join([f"The tall iron tower number {i} in paris was built for the world fair."] * (5 + 7 * i)) for i in range(4)]
MIXED = "caf\u00e9 中文 \U0001F600 " * 40
QS = ["Where is the tower?", "Who built it?", "When was the fair?"]


def _docs(texts):
    return [types.SimpleNamespace(text=t) for t in texts]


RS = [_docs(CTXS), _docs([CTXS[2], "", MIXED, " "]), _docs(CTXS[::-1] + [MIXED])]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The tiny engine and token head of tests/test_heads_gpu.py, with the synthetic tokenizer's [CLS] = 2 / [SEP] = 3 in its shape."""
    from tokenizers import Tokenizer

    from verbatim_rag_amd.bpe import GpuByteBpeTokenizer
    from verbatim_rag_amd.engine import EncoderEngine, ModernBertShape

    shape = dict(TINY, cls_token_id=2, sep_token_id=3)
    w = O.random_weights(O.EncoderConfig(**TINY), seed=7)
    z = np.load(os.path.join(G, "encoder_tiny.npz"))
    engines = []
    for max_tokens, max_seq_len in ((8192, 2048), (512, 512)):
        eng = EncoderEngine(ModernBertShape(**shape), w, max_tokens=max_tokens, max_seqs=64, max_seq_len=max_seq_len, max_ranges=256)
        eng.set_token_head(z["tk_head.dense.weight"], z["tk_head.norm.weight"], z["tk_classifier.weight"], z["tk_classifier.bias"])
        engines.append(eng)
    path = write_tokenizer(tmp_path_factory.mktemp("route") / "tokenizer.json", vocab_size=480, **VARIANTS["nfc_runs"])
    gpu_tok = GpuByteBpeTokenizer.from_file(path)
    assert gpu_tok.vocab_size <= TINY["vocab_size"]
    yield engines, Tokenizer.from_file(path), gpu_tok
    gpu_tok.close()
    for eng in engines:
        eng.close()


_THR = []


def _threshold(host):
    """The midpoint of the widest gap of the host route's own P (per context token, window maximum) inside [0.35, 0.65]; no P lies
    within 1e-5 of it -- the fp32 softmax and the fp32 margin comparison differ by a few 1e-7 at most, so both routes see every
    token on the same side.  A condition of the comparison, not a tolerance."""
    from verbatim_rag_amd.extractors import softmax_rows

    if _THR:
        return _THR[0]
    ps = []
    for q, docs in zip(QS, RS):
        for d in docs:
            if not d.text.strip():
                continue
            windows, _offsets, n_ctx = host._encode_windows(q, d.text)
            eng = host.engine
            eng.load_batch([w[0] for w in windows])
            eng.run()
            eng.run_token_head()
            p1 = softmax_rows(eng.read_token_logits())[:, 1]
            P = np.zeros(n_ctx, np.float32)
            o = 0
            for ids, (a, b), q_len in windows:
                P[a:b] = np.maximum(P[a:b], p1[o + q_len:o + q_len + (b - a)])
                o += len(ids)
            ps.append(P)
    P = np.sort(np.concatenate(ps).astype(np.float64))
    inside = P[(P >= 0.35) & (P <= 0.65)]
    edges = np.concatenate([[0.35], inside, [0.65]])
    k = int(np.argmax(np.diff(edges)))
    thr = float((edges[k] + edges[k + 1]) / 2)
    print("threshold", thr, "nearest P", np.abs(P - thr).min(), "P in [0.35, 0.65]:", len(inside), "of", len(P))
    assert np.abs(P - thr).min() > 1e-5, (thr, np.abs(P - thr).min())
    _THR.append(thr)
    return thr


def test_device_route_equals_host_route(setup, caplog):
    from verbatim_rag_amd.extractors import GpuModelSpanExtractor

    (eng, small), hf_tok, gpu_tok = setup
    probe = GpuModelSpanExtractor(engine=eng, tokenizer=hf_tok, threshold=0.5, **KW)
    thr = _threshold(probe)
    host = GpuModelSpanExtractor(engine=eng, tokenizer=hf_tok, threshold=thr, **KW)
    dev = GpuModelSpanExtractor(engine=eng, tokenizer=gpu_tok, threshold=thr, highlighter_route="device", **KW)
    before = gpu_tok.fallback_count
    want = host.extract_spans_batch(QS, RS)
    got = dev.extract_spans_batch(QS, RS)
    assert got == want
    assert [list(d) for d in got] == [list(d) for d in want] and got[1][""] == [] and got[1][" "] == []
    assert any(len(v) > 0 for d in got for v in d.values()) and len(got[1][MIXED]) + len(got[2][MIXED]) > 0
    assert got == [dev.extract_spans(q, r) for q, r in zip(QS, RS)]
    assert gpu_tok.fallback_count == before
    # a second call is served from the chunk cache: no tokenizer work for the contexts
    calls = []
    real = gpu_tok.encode_batch_offsets
    gpu_tok.encode_batch_offsets = lambda *a, **k: calls.append(a) or real(*a, **k)
    try:
        assert dev.extract_spans_batch(QS, RS) == want and calls == []
        fresh = GpuModelSpanExtractor(engine=eng, tokenizer=gpu_tok, threshold=thr, highlighter_route="device", **KW)
        fresh.prepare_chunks(CTXS + [MIXED, ""])      # the ingest hook fills it for this format too
        assert len(calls) == 1 and len(calls[0][0]) == 5
        assert fresh.extract_spans_batch(QS, RS) == want and len(calls) == 1
    finally:
        del gpu_tok.encode_batch_offsets
    assert not [r for r in caplog.records if r.levelname == "ERROR"]


def test_a_job_larger_than_a_device_batch_takes_the_host_code(setup, caplog):
    """max_batch_tokens below the windows of the longest contexts (but above one window): those jobs run window by window through the
    host route's code, the others through the device route; the result is the host route's."""
    from verbatim_rag_amd.extractors import GpuModelSpanExtractor

    (eng, small), hf_tok, gpu_tok = setup
    thr = _threshold(GpuModelSpanExtractor(engine=eng, tokenizer=hf_tok, threshold=0.5, **KW))
    host = GpuModelSpanExtractor(engine=eng, tokenizer=hf_tok, threshold=thr, **KW)
    want = host.extract_spans_batch(QS, RS)
    seen = []
    for kw, engine in ((dict(max_batch_tokens=512), eng), ({}, small)):      # the extractor's own bound, and a small workspace
        dev = GpuModelSpanExtractor(engine=engine, tokenizer=gpu_tok, threshold=thr, highlighter_route="device", **kw, **KW)
        routes = []
        real_host, real_dev = dev._run_highlighter_jobs, dev._run_device_batch
        dev._run_highlighter_jobs = lambda jobs, out: routes.append(("host", len(jobs))) or real_host(jobs, out)
        dev._run_device_batch = lambda jobs, *a: routes.append(("device", len(jobs))) or real_dev(jobs, *a)
        assert dev.extract_spans_batch(QS, RS) == want
        assert {r for r, _n in routes} == {"host", "device"}
        seen.append(routes)
    assert seen[0] == seen[1]
    assert not [r for r in caplog.records if r.levelname == "ERROR"]
