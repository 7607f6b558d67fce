"""CPU: the ModernBERT sequence-classification reranker -- the numpy head oracle against transformers' logits (golden
fixture), checkpoint loading (head attached from `architectures`, refusals naming the config key), and the host logic of
`GpuCrossEncoderReranker.rerank_batch` / `StaticVerbatimPipeline.query_batch` on fake engines."""
import os
import sys
import types

import numpy as np
import pytest
from tokenizers import Tokenizer
from tokenizers.models import WordLevel
from tokenizers.pre_tokenizers import Whitespace

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd.pipeline import StaticVerbatimPipeline
from verbatim_rag_amd.rerankers import FUSED_ATTENTION_MAX_LEN, GpuCrossEncoderReranker
from verbatim_rag_amd.vector_stores import SearchResult

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seq_head_oracle as SH  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return SH.load_golden()


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_head_oracle_matches_transformers_golden(golden, pooling):
    m = golden["models"][pooling]
    assert m["classifier_bias"] == (pooling == "cls")
    for ids, ref in zip(golden["ids"], m["logits"]):
        got = SH.pair_logits(golden["cfg"], golden["encoder"], ids, m["head"], pooling)
        assert got.shape == ref.shape
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5)


def test_pooling_choice_matters(golden):
    """The two poolings give different logits on the same hidden state (a head that ignored the mode would pass nothing)."""
    m = golden["models"]["mean"]
    hid = SH.O.encoder_forward(golden["cfg"], golden["encoder"], golden["ids"][1])
    assert np.abs(SH.head_logits(hid, m["head"], "cls", 1e-5) - SH.head_logits(hid, m["head"], "mean", 1e-5)).max() > 1e-3


# ------------------------------------------------------------------------------------------------ checkpoint loading
class _Recorder:
    max_seqs, max_tokens, max_ranges, has_mlm = 64, 65536, 1024, False

    def __init__(self, shape, weights, **kw):
        self.shape, self.weights, self.kw = shape, weights, kw
        self.max_seq_len = kw.get("max_seq_len", 512)
        self.pair_labels = 0
        self.seq_head = None

    def set_mlm_head(self, *a, **k):
        self.has_mlm = True

    def set_seq_head(self, dense_w, dense_b, norm_w, norm_b, cls_w, cls_b, pooling="cls"):
        self.seq_head = dict(dense_w=dense_w, dense_b=dense_b, norm_w=norm_w, norm_b=norm_b, cls_w=cls_w, cls_b=cls_b, pooling=pooling)
        self.pair_labels = int(np.asarray(cls_w).shape[0])


@pytest.fixture
def recorder(monkeypatch):
    from verbatim_rag_amd import engine as eng_mod

    monkeypatch.setattr(eng_mod, "EncoderEngine", _Recorder)


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_sequence_classification_directory_attaches_the_head(tmp_path, golden, recorder, pooling):
    SH.write_checkpoint(str(tmp_path), golden, pooling)
    rr = GpuCrossEncoderReranker.from_directory(str(tmp_path), rerank_k=9)
    eng, m = rr.engine, golden["models"][pooling]
    assert rr.rerank_k == 9 and eng.pair_labels == m["head"]["cls_w"].shape[0]
    h = eng.seq_head
    assert h["pooling"] == pooling and h["norm_b"] is None
    for k in ("dense_w", "norm_w", "cls_w", "cls_b"):
        assert np.array_equal(h[k], m["head"][k]), k
    if m["classifier_bias"]:
        assert np.array_equal(h["dense_b"], m["head"]["dense_b"])
    else:
        assert h["dense_b"] is None
    # defaults of a ModernBERT cross-encoder: the checkpoint's context (CrossEncoder's max_length) and bf16 operands
    assert rr.max_length == 8192 and eng.kw["max_seq_len"] == 8192 and eng.kw["operand_dtype"] == "bf16"
    assert GpuCrossEncoderReranker.from_directory(str(tmp_path), max_length=1024, operand_dtype="f16").engine.kw["operand_dtype"] == "f16"


def test_classifier_bias_is_read_from_the_config_not_the_tensors(tmp_path, golden, recorder):
    """`head.dense.bias` present but classifier_bias false in config.json: the config decides (as transformers would build it)."""
    SH.write_checkpoint(str(tmp_path), golden, "cls", classifier_bias=False)
    assert GpuCrossEncoderReranker.from_directory(str(tmp_path)).engine.seq_head["dense_b"] is None


def test_token_classification_directory_has_no_pair_head(tmp_path, golden, recorder):
    SH.write_checkpoint(str(tmp_path), golden, "cls", architectures=["ModernBertForTokenClassification"])
    with pytest.raises(ValueError, match="no pair head"):
        GpuCrossEncoderReranker.from_directory(str(tmp_path))


@pytest.mark.parametrize("key,value", [("norm_bias", True), ("classifier_activation", "silu"), ("classifier_pooling", "max")])
def test_unsupported_head_config_is_refused_naming_the_key(tmp_path, golden, recorder, key, value):
    SH.write_checkpoint(str(tmp_path), golden, "mean", **{key: value})
    with pytest.raises(ValueError, match=key):
        GpuCrossEncoderReranker.from_directory(str(tmp_path))


# ------------------------------------------------------------------------------------------------ rerank_batch host logic
def _tok():
    vocab = {"[PAD]": 0, "[CLS]": 1, "[SEP]": 2, "[UNK]": 3}
    vocab.update({f"w{i}": 4 + i for i in range(200)})
    t = Tokenizer(WordLevel(vocab, unk_token="[UNK]"))
    t.pre_tokenizer = Whitespace()
    return t


class FakeSeqEngine:
    """Duck-typed EncoderEngine: score = number of document tokens equal to the first question token, minus a length
    tie-breaker (scores depend on the pair only, never on its batch mates)."""
    max_seq_len, max_seqs, max_tokens, pair_labels = 1024, 6, 1500, 1
    shape = types.SimpleNamespace(cls_token_id=1, sep_token_id=2)

    def __init__(self):
        self.batches = []

    def pair_logits(self, seqs, type_ids=None):
        self.batches.append([len(s) for s in seqs])
        assert len(seqs) <= self.max_seqs and sum(len(s) for s in seqs) <= self.max_tokens
        out = []
        for s in seqs:
            sep = s.index(2)
            out.append([float(sum(1 for x in s[sep + 1:] if x == s[1])) - 1e-3 * len(s)])
        return np.asarray(out, dtype=np.float32)


def _results(rng, n, long_every=0):
    out = []
    for j in range(n):
        m = 700 if long_every and j % long_every == 0 else int(rng.integers(1, 60))
        out.append(SearchResult(id=str(j), score=1.0 / (j + 1), metadata={},
                                text=" ".join(f"w{int(i)}" for i in rng.integers(0, 12, m))))
    return out


def _questions(rng, n):
    return [" ".join(f"w{int(i)}" for i in rng.integers(0, 12, int(rng.integers(1, 6)))) for _ in range(n)]


@pytest.mark.parametrize("rerank_k", [50, 5])
def test_rerank_batch_equals_per_question_rerank(rerank_k):
    rng = np.random.default_rng(rerank_k)
    qs = _questions(rng, 7)
    res = [_results(rng, int(n), long_every=4) for n in rng.integers(0, 14, len(qs))]
    res[2] = []
    one = GpuCrossEncoderReranker(FakeSeqEngine(), _tok(), rerank_k=rerank_k, max_length=1024)
    batched = GpuCrossEncoderReranker(FakeSeqEngine(), _tok(), rerank_k=rerank_k, max_length=1024)
    want = [one.rerank(q, r) for q, r in zip(qs, res)]
    got = batched.rerank_batch(qs, res)
    assert [[r.id for r in x] for x in got] == [[r.id for r in x] for x in want]
    n_pairs = sum(min(len(r), rerank_k) for r in res)
    assert sum(len(b) for b in batched.engine.batches) == n_pairs
    # shared device batches: the short pairs of all questions fill whole batches (their tokens never reach max_tokens)
    n_short = sum(1 for b in one.engine.batches for n in b if n <= FUSED_ATTENTION_MAX_LEN)
    short_batches = [b for b in batched.engine.batches if b[0] <= FUSED_ATTENTION_MAX_LEN]
    assert len(short_batches) == -(-n_short // FakeSeqEngine.max_seqs)


def test_rerank_batch_keeps_long_pairs_off_short_batches():
    rng = np.random.default_rng(3)
    qs = _questions(rng, 5)
    res = [_results(rng, 10, long_every=3) for _ in qs]
    rr = GpuCrossEncoderReranker(FakeSeqEngine(), _tok(), rerank_k=50, max_length=1024)
    rr.rerank_batch(qs, res)
    lens = [n for b in rr.engine.batches for n in b]
    assert any(n > FUSED_ATTENTION_MAX_LEN for n in lens) and any(n <= FUSED_ATTENTION_MAX_LEN for n in lens)
    for b in rr.engine.batches:
        assert all(n > FUSED_ATTENTION_MAX_LEN for n in b) or all(n <= FUSED_ATTENTION_MAX_LEN for n in b), b
        assert b == sorted(b)                       # ordered by packed length
    assert all(len(b) <= FakeSeqEngine.max_seqs for b in rr.engine.batches)


def test_rerank_batch_on_the_text_field():
    rng = np.random.default_rng(5)
    qs = _questions(rng, 3)
    res = [_results(rng, 6) for _ in qs]
    for rs in res:
        for r in rs[::2]:
            r.enhanced_text = "w1 w1 w1 " + r.text
    one = GpuCrossEncoderReranker(FakeSeqEngine(), _tok(), text_field="enhanced_text", max_length=1024)
    got = GpuCrossEncoderReranker(FakeSeqEngine(), _tok(), text_field="enhanced_text", max_length=1024).rerank_batch(qs, res)
    assert [[r.id for r in x] for x in got] == [[r.id for r in one.rerank(q, r)] for q, r in zip(qs, res)]


def test_rerank_batch_rejects_mismatched_lengths():
    rr = GpuCrossEncoderReranker(FakeSeqEngine(), _tok(), max_length=1024)
    with pytest.raises(ValueError, match="2 questions but 1 result"):
        rr.rerank_batch(["a", "b"], [[]])


# ------------------------------------------------------------------------------------------------ pipeline
class _Index:
    def query(self, text, k=5, **kw):
        return [SearchResult(id=f"{text}-{j}", score=1.0, metadata={}, text=f"{text} doc {j}.") for j in range(k)]


class _Extractor:
    def extract_spans(self, question, results):
        return {r.text: [r.text] for r in results[:2]}


def test_query_batch_uses_rerank_batch_and_falls_back_per_question():
    calls = []

    class Batched:
        def rerank_batch(self, qs, rs):
            calls.append(("batch", len(qs)))
            return [list(reversed(r)) for r in rs]

        def rerank(self, q, rs):
            calls.append(("one", q))
            return list(reversed(rs))

    qs = ["alpha", "beta", "gamma"]
    pipe = StaticVerbatimPipeline(_Index(), _Extractor(), k=3, reranker=Batched())
    got = [r.model_dump() for r in pipe.query_batch(qs)]
    assert calls == [("batch", 3)]
    assert got == [pipe.query(q).model_dump() for q in qs]

    def one_by_one(q, rs):
        if q == "beta":
            raise RuntimeError("this question fails")
        return list(reversed(rs))

    class Failing:
        def rerank_batch(self, qs, rs):
            raise RuntimeError("device batch failed")

        rerank = staticmethod(one_by_one)

    got = [r.model_dump() for r in StaticVerbatimPipeline(_Index(), _Extractor(), k=3, reranker=Failing()).query_batch(qs)]
    per_q = StaticVerbatimPipeline(_Index(), _Extractor(), k=3, reranker=types.SimpleNamespace(rerank=one_by_one))
    assert got == [per_q.query(q).model_dump() for q in qs]
    plain = StaticVerbatimPipeline(_Index(), _Extractor(), k=3)
    assert got[1] == plain.query("beta").model_dump()          # the failing question keeps its retrieval order
    assert got[0] != plain.query("alpha").model_dump()         # the others are reranked
