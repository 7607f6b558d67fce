"""The v2 highlighter's device route, the parts that need no GPU: the offsets rule of `vrag_bpe_encode_offsets` against HF
`tokenizers`, the numpy span reference against `token_spans_to_char_spans`, the numpy window plan against `_encode_windows`, and
what the constructor refuses."""
import json
import math
import types

import numpy as np
import pytest

from bpe_cases import VARIANTS, corpus, spec_ids, tokenizer_json
from spans_ref import logits_of, plan_windows, random_job, select, spec_offsets, window_max

# the EDGE texts of tests/test_bpe_gpu.py (that module is all GPU tests; importing it runs none)
from test_bpe_gpu import EDGE


@pytest.mark.parametrize("name", list(VARIANTS))
def test_offsets_rule_equals_hf(name):
    """Byte range -> code points: start = the code point that holds the first byte, end = the one that holds the last byte, + 1."""
    from tokenizers import Tokenizer

    from verbatim_rag_amd.bpe import parse_spec

    spec = json.loads(tokenizer_json(**VARIANTS[name]))
    cfg = parse_spec(spec)
    hf = Tokenizer.from_str(json.dumps(spec))
    four_byte = ["\U0001F600", "a\U0001F600b", "\U0001F600\U0001F601 \U00010348x", "x \U0001F9E0\U0001F9E0 y", "\U00020000\U00020001"]
    texts = EDGE + corpus(7, 400) + four_byte + ["\u00e9" * 32, " " * 30 + "x", "tokenization " * 20]
    n_tokens = split = 0
    for text, enc in zip(texts, hf.encode_batch(texts, add_special_tokens=False)):
        got = spec_offsets(text, cfg)
        if got is None:
            assert spec_ids(text, cfg) is None
            continue
        assert spec_ids(text, cfg) == list(enc.ids), repr(text)
        assert got == [tuple(o) for o in enc.offsets], (repr(text), enc.tokens)
        n_tokens += len(got)
        split += sum(1 for a, b in zip(got, got[1:]) if b[0] < a[1])
    assert n_tokens > 5000 and split > 0      # ids that start inside the previous id's character are among them
    # the 4-byte characters are outside the vocabulary: byte-fallback ids that share one character
    assert spec_offsets("\U0001F600", cfg) == [(0, 1)] * len(spec_ids("\U0001F600", cfg)) and len(spec_ids("\U0001F600", cfg)) > 1


def _host_spans(logits, windows, offsets, thr, min_span, gap):
    """The host route: softmax, window maximum over zero-initialised probabilities, `token_spans_to_char_spans`."""
    from verbatim_rag_amd.extractors import softmax_rows, token_spans_to_char_spans

    p1 = softmax_rows(logits)[:, 1]
    probs = np.zeros(len(offsets), np.float32)
    for a, b, first in windows:
        probs[a:b] = np.maximum(probs[a:b], p1[first:first + b - a])
    context = "".join(chr(0x4E00 + i) for i in range(int(offsets.max()) + 1))      # every substring names its position
    with np.errstate(invalid="ignore"):
        return token_spans_to_char_spans(probs, [tuple(o) for o in offsets.tolist()], context, thr, min_span, gap), context


def test_span_reference_equals_the_host_route():
    rng = np.random.default_rng(2024)
    seen = dict(spans=0, zero_width=0, shared=0, exact=0, nan=0, multi=0)
    for j in range(2000):
        thr = float(rng.choice([0.2, 0.45, 0.5, 0.8]))
        tau = np.float32(math.log(thr / (1 - thr)))
        min_span, gap = int(rng.integers(1, 8)), int(rng.integers(0, 5))
        room = int(rng.integers(3, 40))
        n_ctx = int(rng.integers(1, 4 * room))
        margins, windows, offsets = random_job(rng, n_ctx, room, int(rng.integers(0, room + 3)), tau, min_span, gap,
                                               hot_rate=float(rng.choice([0.1, 0.5, 0.9])), nan_rate=0.02 if j % 4 == 0 else 0.0)
        assert np.all(np.isnan(margins) | (np.abs(margins - tau) > 1e-3 * 0.999))
        got = select(margins, windows, offsets, tau, min_span, gap)
        want, context = _host_spans(logits_of(margins, rng), windows, offsets, thr, min_span, gap)
        assert [context[a:b] for a, b in got] == want, j
        seen["spans"] += len(got)
        seen["zero_width"] += int((offsets[:, 1] == offsets[:, 0]).any())
        seen["shared"] += int((offsets[1:, 0] < offsets[:-1, 1]).any())
        seen["exact"] += sum(1 for a, b in got if b - a == min_span)
        seen["nan"] += int(np.isnan(window_max(margins, windows, n_ctx)).any())
        seen["multi"] += int(len(windows) > 2)
    assert all(v > 50 for v in seen.values()), seen


def test_span_reference_on_the_rule_s_edges():
    """Gaps of -1, 0, gap, gap + 1 between two runs; spans of min_span - 1 and min_span; a zero-width token inside a run."""
    tau, min_span, gap = 0.0, 4, 2

    def spans(offsets, hot):
        margins = np.where(np.asarray(hot, bool), 1.0, -1.0).astype(np.float32)
        return select(margins, [(0, len(hot), 0)], np.asarray(offsets, np.int32), tau, min_span, gap)

    for d, want in [(-1, [(0, 7)]), (0, [(0, 8)]), (gap, [(0, 10)]), (gap + 1, [(0, 4), (7, 11)])]:
        assert spans([(0, 4), (4, 4), (4 + d, 4 + d), (4 + d, 8 + d)], [1, 0, 0, 1]) == [(0, 8 + d)], d      # zero width closes nothing: one run
        assert spans([(0, 4), (1, 2), (4 + d, 8 + d)], [1, 0, 1]) == want, d
    assert spans([(0, 3), (3, 5), (20, 24)], [1, 0, 1]) == [(20, 24)]                # 3 < min_span is dropped, 4 is kept
    assert spans([(0, 2), (2, 2), (2, 4)], [1, 0, 1]) == [(0, 4)]                    # the cold token has no characters: one run
    assert spans([(0, 2), (0, 0), (5, 9)], [0, 1, 0]) == []


@pytest.mark.parametrize("doc_stride", [0, 16, 39, 40, 41, 500])
def test_window_plan_equals_encode_windows(doc_stride):
    """`window_plan` (numpy, the device route) against the loop of `_encode_windows` for context lengths around `room`, and for
    doc_stride >= room, where the step is 1."""
    from verbatim_rag_amd.extractors import GpuModelSpanExtractor, window_plan

    class Tok:
        sep_token_id, cls_token_id = 3, 2

        def ids(self, text, add_special_tokens, max_length):
            return [2, 7, 7, 3]

    ext = GpuModelSpanExtractor.__new__(GpuModelSpanExtractor)
    ext.max_length, ext.doc_stride, ext._tok = 45, doc_stride, Tok()
    room = 45 - 4 - 1
    for n_ctx in (1, room - 1, room, room + 1, 3 * room + 5):
        ext.tokenizer = lambda text, **kw: dict(input_ids=list(range(10, 10 + n_ctx)), offset_mapping=[(i, i + 1) for i in range(n_ctx)])
        windows, _offsets, n = ext._encode_windows("q", "c")
        a, b = window_plan(n_ctx, room, doc_stride)
        assert n == n_ctx and [w[1] for w in windows] == list(zip(a.tolist(), b.tolist())) == plan_windows(n_ctx, room, doc_stride)
        assert all(w[0] == [2, 7, 7, 3] + list(range(10 + x, 10 + y)) + [3] and w[2] == 4 for w, (x, y) in zip(windows, zip(a, b)))
        if doc_stride >= room and n_ctx > room:
            assert len(a) == n_ctx - room + 1      # step 1


class _Engine:
    """Stands in for EncoderEngine: enough for the constructor."""
    max_seqs, max_tokens, max_ranges, qa_labels = 64, 8192, 1024, 0

    def __init__(self, token_labels=2):
        self.token_labels = token_labels
        self.shape = types.SimpleNamespace(sep_token_id=3, cls_token_id=2)


class _OffsetsTokenizer:
    sep_token_id, cls_token_id = 3, 2

    def encode_batch_offsets(self, texts, add_special_tokens=False, max_length=512):
        raise AssertionError("the constructor tokenises nothing")


class _PlainTokenizer:
    sep_token_id, cls_token_id = 3, 2


def test_constructor_validation(tmp_path, monkeypatch):
    from verbatim_rag_amd import packing
    from verbatim_rag_amd.extractors import GpuModelSpanExtractor

    monkeypatch.setattr(packing.TokenizerAdapter, "for_model", classmethod(lambda cls, tok, shape: tok))
    kw = dict(model_format="highlighter", threshold=0.5)
    ext = GpuModelSpanExtractor(engine=_Engine(), tokenizer=_OffsetsTokenizer(), highlighter_route="device", **kw)
    assert ext.highlighter_route == "device"
    assert GpuModelSpanExtractor(engine=_Engine(), tokenizer=_PlainTokenizer(), **kw).highlighter_route == "host"
    with pytest.raises(ValueError, match="highlighter_route must be 'host' or 'device'"):
        GpuModelSpanExtractor(engine=_Engine(), tokenizer=_OffsetsTokenizer(), highlighter_route="gpu", **kw)
    for thr in (0.0, 1.0):
        with pytest.raises(ValueError, match="strictly between 0 and 1"):
            GpuModelSpanExtractor(engine=_Engine(), tokenizer=_OffsetsTokenizer(), highlighter_route="device", model_format="highlighter",
                                  threshold=thr)
        GpuModelSpanExtractor(engine=_Engine(), tokenizer=_PlainTokenizer(), model_format="highlighter", threshold=thr)      # the host route takes it
    with pytest.raises(ValueError, match="2-label token head.*3 labels"):
        GpuModelSpanExtractor(engine=_Engine(3), tokenizer=_OffsetsTokenizer(), highlighter_route="device", **kw)
    with pytest.raises(ValueError, match="encode_batch_offsets"):
        GpuModelSpanExtractor(engine=_Engine(), tokenizer=_PlainTokenizer(), highlighter_route="device", **kw)
    with pytest.raises(ValueError, match="route of the highlighter format"):
        GpuModelSpanExtractor(engine=_Engine(), tokenizer=_OffsetsTokenizer(), highlighter_route="device", model_format="qa_model",
                              threshold=0.5)
    # with model_path the route loads the device tokenizer itself: "host" contradicts it, before any engine is built
    (tmp_path / "config.json").write_text(json.dumps({"auto_map": {"AutoModel": "modeling_verbatim.VerbatimHighlighterModel"}}))
    with pytest.raises(ValueError, match='not "host"'):
        GpuModelSpanExtractor(model_path=str(tmp_path), tokenizer="host", highlighter_route="device", threshold=0.5)
    # ... and the default route keeps its refusal of the device tokenizer
    with pytest.raises(ValueError, match="yields no character offsets"):
        GpuModelSpanExtractor(model_path=str(tmp_path), tokenizer="gpu", threshold=0.5)


def test_new_kernels_keep_everything_in_registers():
    """The offsets kernels of csrc/bpe.hip and the span kernel: no scratch, no spills; the offsets merge kernel holds no LDS, like the
    merge kernel it shares its body with."""
    import os

    from test_kernel_resources import HIPCC, _resources

    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    rows = {r["name"]: r for r in _resources("bpe.hip") if "offsets_" in r["name"] or "pack_gather" in r["name"]}
    rows.update({r["name"]: r for r in _resources("spans.hip")})
    assert len(rows) == 5, list(rows)      # lead count, offsets merge, the gather for ids and for offsets, token spans
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
        if "merge" in name or "token_spans" in name:
            assert int(r["LDS Size [bytes/block]"]) == 0, r
