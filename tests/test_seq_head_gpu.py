"""GPU: the ModernBERT sequence-classification head (`vrag_encoder_run_seq_head`, csrc/norm_heads.hip seq_pool_kernel +
seq_head_kernel) and the ModernBERT cross-encoder reranker built on it -- the head alone against the numpy head on the
engine's own final hidden states, pair logits against transformers' (golden fixture), lengths on both attention paths,
`rerank_batch` against per-question `rerank`, the batched pipeline, and `from_directory` end to end."""
import os
import sys

import numpy as np
import pytest

from oracle import modernbert_np as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seq_head_oracle as SH  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-3   # ModernBERT pooled / sentence logits against the fp32 reference (tests/test_extractor_gpu.py)


@pytest.fixture(scope="module")
def golden():
    return SH.load_golden()


def _shape(cfg):
    from verbatim_rag_amd.engine import ModernBertShape

    return ModernBertShape(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                           num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                           pad_token_id=cfg.pad_token_id, cls_token_id=cfg.cls_token_id, sep_token_id=cfg.sep_token_id)


def _set(eng, m):
    h = m["head"]
    eng.set_seq_head(h["dense_w"], h["dense_b"], h["norm_w"], h["norm_b"], h["cls_w"], h["cls_b"], pooling=m["pooling"])


@pytest.fixture(scope="module")
def tiny(golden):
    """The fixture's encoder on a handle that takes every path: fused attention (<= 512 tokens, throughput-sized batches),
    the separate attention kernel (longer sequences) and a 2 048-token max_seq_len."""
    from verbatim_rag_amd.engine import EncoderEngine

    eng = EncoderEngine(_shape(golden["cfg"]), golden["encoder"], max_tokens=16384, max_seqs=64, max_seq_len=2048, max_ranges=64)
    yield eng
    eng.close()


def _split(hidden, lens):
    out, o = [], 0
    for n in lens:
        out.append(hidden[o:o + n])
        o += n
    return out


def _random_head(rng, H, labels, dense_bias, norm_bias):
    return {"dense_w": (rng.standard_normal((H, H)) * H ** -0.5).astype(np.float32),
            "dense_b": (0.1 * rng.standard_normal(H)).astype(np.float32) if dense_bias else None,
            "norm_w": (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32),
            "norm_b": (0.1 * rng.standard_normal(H)).astype(np.float32) if norm_bias else None,
            "cls_w": (rng.standard_normal((labels, H)) * H ** -0.5).astype(np.float32),
            "cls_b": (0.1 * rng.standard_normal(labels)).astype(np.float32)}


@pytest.mark.parametrize("hidden_size", [128, 768])
@pytest.mark.parametrize("pooling", ["cls", "mean"])
@pytest.mark.parametrize("biases", [False, True])
def test_head_alone_against_numpy_on_the_engines_hidden_states(golden, hidden_size, pooling, biases):
    """The kernel apart from encoder rounding: numpy head on `read_hidden(final_norm=True)` of the same batch, 1e-5 of the
    logit scale.  21 sequences = two full row blocks of 8 and a partial one; H = 768 gives each thread three columns."""
    from verbatim_rag_amd.engine import EncoderEngine, ModernBertShape

    H = hidden_size
    shape = ModernBertShape(vocab_size=512, hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64,
                            intermediate_size=H * 3 // 2, pad_token_id=0, cls_token_id=1, sep_token_id=2)
    cfg = O.EncoderConfig(vocab_size=512, hidden_size=H, num_hidden_layers=1, num_attention_heads=H // 64,
                          intermediate_size=H * 3 // 2, pad_token_id=0, cls_token_id=1, sep_token_id=2)
    rng = np.random.default_rng(H + 2 * biases + (pooling == "mean"))
    eng = EncoderEngine(shape, O.random_weights(cfg, seed=3), max_tokens=8192, max_seqs=32, max_seq_len=1024, max_ranges=64)
    try:
        labels = 3 if biases else 1
        head = _random_head(rng, H, labels, biases, biases)
        eng.set_seq_head(head["dense_w"], head["dense_b"], head["norm_w"], head["norm_b"], head["cls_w"], head["cls_b"], pooling)
        lens = [int(n) for n in rng.integers(1, 300, 21)] + [700]
        seqs = [rng.integers(3, 512, n).astype(np.int32) for n in lens]
        eng.load_batch(seqs)
        eng.run()
        eng.run_seq_head()
        got = eng.read_seq_logits()
        hid = eng.read_hidden(final_norm=True)
        ref = np.stack([SH.head_logits(h, head, pooling, shape.norm_eps) for h in _split(hid, lens)])
        assert got.shape == (len(lens), labels)
        scale = max(1.0, float(np.abs(ref).max()))
        assert float(np.abs(got - ref).max()) <= 1e-5 * scale, np.abs(got - ref).max()
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_pair_logits_against_transformers_golden(golden, pooling, dtype):
    from verbatim_rag_amd.engine import EncoderEngine

    eng = EncoderEngine(_shape(golden["cfg"]), golden["encoder"], max_tokens=4096, max_seqs=16, max_seq_len=512, max_ranges=16,
                        operand_dtype=dtype)
    try:
        m = golden["models"][pooling]
        _set(eng, m)
        got = eng.pair_logits(golden["ids"])
        assert got.shape == m["logits"].shape
        err = float(np.abs(got - m["logits"]).max())
        assert err <= TOL, err
    finally:
        eng.close()


def test_seq_head_refusals(golden, tiny):
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.engine import BertEncoderEngine, BertShape
    from verbatim_rag_amd.weights import random_init_bert

    m = golden["models"]["cls"]
    with pytest.raises(ValueError, match="pooling"):
        tiny.set_seq_head(m["head"]["dense_w"], None, m["head"]["norm_w"], None, m["head"]["cls_w"], m["head"]["cls_b"], "max")
    sh = BertShape(vocab_size=300, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                   max_position_embeddings=64)
    bert = BertEncoderEngine(sh, random_init_bert(sh, mlm=False), max_tokens=512, max_seqs=4, max_seq_len=64, max_ranges=4)
    try:
        with pytest.raises(_lib.VragError, match="set_pair_head"):
            bert.set_seq_head(m["head"]["dense_w"], None, m["head"]["norm_w"], None, m["head"]["cls_w"], m["head"]["cls_b"], "cls")
    finally:
        bert.close()


def _oracle(golden, m, seqs):
    return np.stack([SH.pair_logits(golden["cfg"], golden["encoder"], s, m["head"], m["pooling"]) for s in seqs])


def _pair_ids(rng, n, V):
    return np.concatenate([[1], rng.integers(5, V, 7), [2], rng.integers(5, V, n - 10), [2]]).astype(np.int32)


@pytest.mark.parametrize("case", ["fused", "long", "max_seq_len"])
def test_lengths_on_both_attention_paths(golden, tiny, case):
    """<= 512 tokens in a throughput-sized batch (fused QKV + attention kernel), 513 - 2 048 tokens (separate attention
    kernel), and one pair at the handle's max_seq_len -- against the numpy oracle."""
    rng = np.random.default_rng({"fused": 1, "long": 2, "max_seq_len": 3}[case])
    V = golden["cfg"].vocab_size
    lens = {"fused": [int(n) for n in rng.integers(380, 513, 24)], "long": [513, 777, 1500, 2048 - 64],
            "max_seq_len": [tiny.max_seq_len]}[case]
    if case == "fused":
        assert sum(lens) > 8192   # above the launch-bound threshold: the fused kernel's regime
    seqs = [_pair_ids(rng, n, V) for n in lens]
    for pooling in ("cls", "mean"):
        m = golden["models"][pooling]
        _set(tiny, m)
        got = tiny.pair_logits(seqs)
        err = float(np.abs(got - _oracle(golden, m, seqs)).max())
        assert err <= TOL, (pooling, err)


# ------------------------------------------------------------------------------------------------ reranker
WORDS = ("the quick brown fox jumps over lazy dog tower paris iron built year tall meters visitors river city bridge stone "
         "engineer opened museum garden light night climb stairs lift wind steel design world fair").split()


def _text(rng, n):
    return " ".join(WORDS[int(i)] for i in rng.integers(0, len(WORDS), n))


def _tokenizer():
    from tokenizers import Tokenizer

    return Tokenizer.from_file(os.path.join(os.path.dirname(__file__), "golden", "tokenizer.json"))


def _results(rng, n, lo, hi):
    from verbatim_rag_amd.vector_stores import SearchResult

    return [SearchResult(id=f"d{j}", score=1.0 / (j + 1), metadata={}, text=_text(rng, int(rng.integers(lo, hi))))
            for j in range(n)]


def _oracle_scores(golden, rr, m, question, texts):
    from verbatim_rag_amd.rerankers import pack_pair

    q = rr._ids(question)
    seqs = [pack_pair(q, rr._ids(t), 1, 2, rr.max_length)[0] for t in texts]
    return _oracle(golden, m, seqs)[:, 0]


def _orders_agree_where_separated(order, ref_scores, texts_ids, tol):
    """Every pair of results whose oracle scores differ by more than 2 tol is in the oracle's relative order."""
    pos = {rid: i for i, rid in enumerate(order)}
    ids = list(texts_ids)
    for i in range(len(ids)):
        for j in range(len(ids)):
            if ref_scores[i] - ref_scores[j] > 2 * tol:
                assert pos[ids[i]] < pos[ids[j]], (ids[i], ids[j], ref_scores[i], ref_scores[j])


@pytest.fixture(scope="module")
def reranker(golden):
    from verbatim_rag_amd.engine import EncoderEngine
    from verbatim_rag_amd.rerankers import GpuCrossEncoderReranker

    eng = EncoderEngine(_shape(golden["cfg"]), golden["encoder"], max_tokens=32768, max_seqs=256, max_seq_len=1024, max_ranges=64)
    _set(eng, golden["models"]["mean"])   # label 0 of the mean-pooled head: the wider spread of scores
    rr = GpuCrossEncoderReranker(eng, _tokenizer(), rerank_k=50, max_length=1024)
    yield rr
    eng.close()


def test_rerank_batch_bit_identical_when_launch_bound(reranker):
    """Both calls launch-bound (<= 8 192 packed rows): the batched scores are the per-question scores, bit for bit."""
    rng = np.random.default_rng(11)
    qs = [_text(rng, int(rng.integers(2, 8))) for _ in range(4)]
    res = [_results(rng, 12, 5, 60) for _ in qs]
    texts = [[r.text for r in rs] for rs in res]
    batched = reranker.score_batch(qs, texts)
    assert sum(len(reranker._ids(t)) + 10 for ts in texts for t in ts) <= 8192
    for q, ts, b in zip(qs, texts, batched):
        assert b == reranker.score(q, ts)
    got = reranker.rerank_batch(qs, res)
    assert [[r.id for r in x] for x in got] == [[r.id for r in reranker.rerank(q, r)] for q, r in zip(qs, res)]


def test_rerank_batch_orders_in_throughput_batches(golden, reranker):
    """16 questions x 50 pairs (up to 256 pairs of ~100 tokens per device batch: throughput-sized; per question: launch-bound)
    plus a few pairs past 512 tokens: the same order wherever the oracle's scores are separated by more than the tolerance."""
    rng = np.random.default_rng(12)
    qs = [_text(rng, int(rng.integers(2, 8))) for _ in range(16)]
    res = [_results(rng, 50, 60, 140) for _ in qs]
    for rs in res[:3]:
        rs[0].text = _text(rng, 700)
    batched = reranker.rerank_batch(qs, res)
    m = golden["models"]["mean"]
    for q, rs, b in zip(qs, res, batched):
        ref = _oracle_scores(golden, reranker, m, q, [r.text for r in rs])
        one = reranker.rerank(q, rs)
        for order in ([r.id for r in b], [r.id for r in one]):
            _orders_agree_where_separated(order, ref, [r.id for r in rs], TOL)


def test_query_batch_with_the_modernbert_reranker_equals_per_question_query(reranker):
    from verbatim_rag_amd.pipeline import StaticVerbatimPipeline

    rng = np.random.default_rng(13)
    corpus = {}

    class Index:
        def query(self, text, k=5, **kw):
            if text not in corpus:
                corpus[text] = _results(rng, k, 5, 80)
            return list(corpus[text])

    class Extractor:
        def extract_spans(self, question, results):
            return {r.text: [r.text.split(" ")[0]] for r in results[:3]}

    qs = [_text(rng, int(rng.integers(2, 8))) for _ in range(5)]
    pipe = StaticVerbatimPipeline(Index(), Extractor(), k=10, reranker=reranker)
    got = [r.model_dump() for r in pipe.query_batch(qs)]
    assert got == [pipe.query(q).model_dump() for q in qs]
    plain = StaticVerbatimPipeline(Index(), Extractor(), k=10)
    assert got != [plain.query(q).model_dump() for q in qs]   # the reranker did reorder


def test_from_directory_end_to_end(tmp_path, golden):
    """A checkpoint written with safetensors.numpy (no transformers): defaults of a ModernBERT cross-encoder, and `rerank`
    in the oracle's order."""
    from verbatim_rag_amd.rerankers import GpuCrossEncoderReranker

    SH.write_checkpoint(str(tmp_path), golden, "mean")
    rr = GpuCrossEncoderReranker.from_directory(str(tmp_path), rerank_k=6)
    try:
        assert rr.max_length == 8192 and rr.engine.operand_dtype == "bf16" and rr.engine.pair_labels == 2
        rng = np.random.default_rng(19)   # oracle scores at least 8e-3 apart: far outside the tolerance
        q = _text(rng, 5)
        res = _results(rng, 9, 10, 120)
        got = rr.rerank(q, res)
        assert [r.id for r in got[6:]] == [r.id for r in res[6:]]       # the tail past rerank_k keeps its place
        ref = _oracle_scores(golden, rr, golden["models"]["mean"], q, [r.text for r in res[:6]])
        assert np.diff(np.sort(ref)).min() > 4 * TOL
        assert [r.id for r in got[:6]] == [res[i].id for i in np.argsort(-ref, kind="stable")]
    finally:
        rr.engine.close()


# x3000 on three GeGLU channel pairs of layer 1, as tests/test_heads_gpu.py::_hot_weights.  Measured on this encoder (MI355X, the
# six golden pairs): x300 does not clamp, x1000 does (fp16 logits 6.7e-2 from the bf16 engine's), x3000 clamps with 1.2e-1 --
# three times past the first scale that leaves fp16's range; bf16 logits stay finite up to x30000.
HOT_SCALE = 3000.0


def _hot_fixture(golden, scale=HOT_SCALE):
    """The golden checkpoint with outlier channels: rows c (gelu input) and I + c (gate) of layer 1's Wi scaled, so
    gelu(x1) * x2 leaves fp16's range.  -> (encoder weights, fixture for SH.write_checkpoint)."""
    I = golden["cfg"].intermediate_size
    enc = {k: v.copy() for k, v in golden["encoder"].items()}
    wi = enc["layers.1.mlp.Wi.weight"]                         # [2I, H]
    assert wi.shape[0] == 2 * I
    for c in (3, 77, 120):
        wi[c] *= scale
        wi[I + c] *= scale
    m = dict(golden["models"]["mean"])
    m["state_dict"] = {**m["state_dict"], "model.layers.1.mlp.Wi.weight": wi}
    return enc, {**golden, "encoder": enc, "models": {"mean": m}}


def test_fp16_reranker_rebuilds_with_bf16_operands_or_raises(tmp_path, golden, caplog):
    """A cross-encoder with fp16 operands on a checkpoint whose activations leave fp16's range must not return clamped
    scores: built `from_directory` it switches itself to bf16 operands and scores like a reranker built with bf16; handed
    its engine it raises.  First the premise on a bare engine -- the clamp is reported and the logits are wrong."""
    import logging

    from verbatim_rag_amd.engine import EncoderEngine
    from verbatim_rag_amd.rerankers import GpuCrossEncoderReranker

    enc, hot = _hot_fixture(golden)
    m = hot["models"]["mean"]

    def bare(dtype):
        eng = EncoderEngine(_shape(golden["cfg"]), enc, max_tokens=16384, max_seqs=64, max_seq_len=1024, max_ranges=64,
                            operand_dtype=dtype)
        _set(eng, m)
        return eng

    e16, ebf = bare("f16"), bare("bf16")
    try:
        lg16, lgbf = e16.pair_logits(golden["ids"]), ebf.pair_logits(golden["ids"])
        flag16, flagbf = e16.f16_saturated(reset=True), ebf.f16_saturated(reset=True)
        print("hot checkpoint x%g: f16 clamp %s, bf16 clamp %s, max |f16 - bf16| = %.3e, bf16 finite %s"
              % (HOT_SCALE, flag16, flagbf, float(np.abs(lg16 - lgbf).max()), bool(np.isfinite(lgbf).all())))
        assert flag16 and not flagbf and np.isfinite(lgbf).all()
        assert np.abs(lg16 - lgbf).max() > 1e-2                # the clamped run really was wrong, not just flagged
    finally:
        ebf.close()

    rng = np.random.default_rng(23)
    qs = [_text(rng, int(rng.integers(2, 8))) for _ in range(3)]
    res = [_results(rng, 8, 10, 120) for _ in qs]
    texts = [r.text for r in res[0]]
    try:                                                       # handed its engine: nothing to rebuild from
        with pytest.raises(RuntimeError, match="saturated"):
            GpuCrossEncoderReranker(e16, _tokenizer(), max_length=1024).score(qs[0], texts)
    finally:
        e16.close()

    d = str(tmp_path)
    SH.write_checkpoint(d, hot, "mean")
    made = []
    try:
        rr_bf = GpuCrossEncoderReranker.from_directory(d, operand_dtype="bf16")
        made.append(rr_bf)
        for call in ("score", "rerank_batch"):                 # a fresh fp16 reranker each: the first clamp swaps for good
            rr = GpuCrossEncoderReranker.from_directory(d, operand_dtype="f16")
            made.append(rr)
            assert rr.engine.operand_dtype == "f16"
            caplog.clear()
            with caplog.at_level(logging.WARNING):
                if call == "score":
                    assert rr.score(qs[0], texts) == rr_bf.score(qs[0], texts)
                else:
                    got, want = rr.rerank_batch(qs, res), rr_bf.rerank_batch(qs, res)
                    assert [[r.id for r in x] for x in got] == [[r.id for r in x] for x in want]
                    assert rr.score_batch(qs, [[r.text for r in rs] for rs in res]) == \
                        rr_bf.score_batch(qs, [[r.text for r in rs] for rs in res])
            assert rr.engine.operand_dtype == "bf16" and any("saturated" in r.getMessage() for r in caplog.records)
            assert rr._checked.locks == [rr.engine.lock]
    finally:
        for rr in made:
            rr.engine.close()
