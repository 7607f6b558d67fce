"""GPU parity of the BERT-family encoder path (vrag_bert_encoder_create) through the C ABI: golden vectors
captured from `transformers` (tiny BERT / DistilBERT), the numpy oracle at BERT-base width, and the embedding
providers on top.  Same precision recipe as the ModernBERT path (bf16 MFMA operands, fp32 elsewhere)."""
import os

import numpy as np
import pytest

from oracle import bert_np as B
from oracle import modernbert_np as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _shape(cfg, kind):
    from verbatim_rag_amd.engine import BertShape

    return BertShape(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                     num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                     max_position_embeddings=cfg.max_position_embeddings, norm_eps=cfg.layer_norm_eps,
                     pad_token_id=0, cls_token_id=1, sep_token_id=2, model_type=kind)


@pytest.mark.parametrize("fold", ["0", "1"])
@pytest.mark.parametrize("name", ["bert_tiny", "distilbert_tiny"])
def test_tiny_models_vs_transformers_golden(name, fold, monkeypatch):
    """fold = 1: the opt-in schedule without LayerNorm kernels (lazy LayerNorm folded into the GEMM epilogues)."""
    monkeypatch.setenv("VRAG_BERT_LN_FOLD", fold)
    from verbatim_rag_amd.engine import BertEncoderEngine
    from verbatim_rag_amd.weights import bert_canonical

    z = np.load(os.path.join(GOLD, f"{name}.npz"))
    V, H, L, NH, I, P = (int(x) for x in z["cfg"])
    cfg = B.BertConfig(vocab_size=V, hidden_size=H, num_hidden_layers=L, num_attention_heads=NH, intermediate_size=I,
                       max_position_embeddings=P)
    W = bert_canonical({k[3:]: z[k] for k in z.files if k.startswith("sd:")})
    eng = BertEncoderEngine(_shape(cfg, "bert" if name == "bert_tiny" else "distilbert"), W, max_tokens=1024,
                            max_seqs=8, max_seq_len=64, max_ranges=16)
    try:
        seqs = [z["ids0"], z["ids1"]]
        eng.load_batch(seqs)
        eng.run()
        got = eng.read_hidden(final_norm=True)   # no final LayerNorm in this family: flag is ignored
        assert np.array_equal(got, eng.read_hidden(final_norm=False))
        o = 0
        for i, s in enumerate(seqs):
            err = np.abs(got[o:o + len(s)] - z[f"hidden{i}"]).max()
            assert err < 3e-2, (name, i, err)
            o += len(s)
        eng.run_splade()
        rows = eng.read_splade()
        for i in range(2):
            ref = O.splade_pool(z[f"mlm{i}"])
            assert np.abs(rows[i] - ref).max() < 3e-2, np.abs(rows[i] - ref).max()
        # per-layer prefix (post-LN stream after the embedding LayerNorm and after layer 1)
        Wo = B.canonical_from_hf({k[3:]: z[k] for k in z.files if k.startswith("sd:")})
        for nl in (0, 1):
            eng.run(n_layers=nl)
            g = eng.read_hidden(final_norm=False)[: len(seqs[0])]
            ref = B.encoder_forward(cfg, Wo, seqs[0], n_layers=nl)
            assert np.abs(g - ref).max() < (1e-5 if nl == 0 else 2e-2), (nl, fold, np.abs(g - ref).max())
    finally:
        eng.close()


@pytest.fixture(scope="module")
def base_width():
    """BERT-base width (H=768, 12 heads, I=3072: the 256x256 GEMM tiles), 2 layers, small vocabulary."""
    from verbatim_rag_amd.engine import BertEncoderEngine

    cfg = B.BertConfig(vocab_size=2048, hidden_size=768, num_hidden_layers=2, num_attention_heads=12,
                       intermediate_size=3072, max_position_embeddings=512)
    W = B.random_weights(cfg, seed=5, kind="bert", std=0.03)
    eng = BertEncoderEngine(_shape(cfg, "bert"), W, max_tokens=8192, max_seqs=32, max_seq_len=512, max_ranges=64,
                            micro_batch_tokens=2048)
    yield cfg, W, eng
    eng.close()


def test_base_width_hidden_pool_and_splade_vs_oracle(base_width):
    cfg, W, eng = base_width
    rng = np.random.default_rng(2)
    lens = [512, 7, 130, 64, 257, 300, 1, 511, 33]
    seqs = [rng.integers(3, cfg.vocab_size, size=n).astype(np.int32) for n in lens]
    eng.load_batch(seqs)
    n = len(seqs)
    eng.load_ranges(list(range(n)), [0] * n, [len(s) - 1 for s in seqs])
    eng.run()
    got = eng.read_hidden(final_norm=False)
    eng.run_pool(True)
    pooled = eng.read_pool()
    eng.run_splade()
    rows = eng.read_splade()
    o = 0
    for i, s in enumerate(seqs):
        ref = B.encoder_forward(cfg, W, s)
        err = np.abs(got[o:o + len(s)] - ref).max()
        assert err < 4e-2, (len(s), err)
        pr = O.dense_pool(ref, "mean", True)
        assert abs(float(np.linalg.norm(pooled[i])) - 1.0) < 1e-5
        assert np.abs(pooled[i] - pr).max() < 2e-3
        sr = O.splade_pool(B.mlm_logits(cfg, W, ref))
        assert np.abs(rows[i] - sr).max() < 4e-2
        o += len(s)
    # micro-batching (2048-token micro-batches on two streams) must not change a sequence's rows, bit for bit: the lone 512-token
    # sequence takes the launch-bound residual GEMMs with K split over four waves, the batch's micro-batches the one-wave tiles --
    # which since round 6 visit the K-steps chain by chain and add the chain sums in the K-split's order (csrc/gemm_bf16.hip, KCH):
    # one fp32 summation order for every launch-bound configuration.  (Round 5 accepted 1e-2 here: observed 7.6e-3.)
    eng.load_batch([seqs[0]])
    eng.run()
    alone = eng.read_hidden(final_norm=False)
    assert np.array_equal(alone, got[:512]), float(np.abs(alone - got[:512]).max())


def test_providers_on_bert_engine(base_width):
    from tokenizers import Tokenizer

    from verbatim_rag_amd.embedding_providers import GpuDenseProvider, GpuSpladeProvider

    cfg, W, eng = base_width
    tok = Tokenizer.from_file(os.path.join(GOLD, "tokenizer.json"))
    texts = ["The Eiffel Tower is in Paris.", "It was built in 1889. Millions visit it.", "tower"]
    sp = GpuSpladeProvider(eng, tok)
    one = sp.embed_text(texts[0])
    many = sp.embed_batch(texts)
    assert sp.get_dimension() == cfg.vocab_size and len(many) == 3
    assert all(isinstance(k, int) and isinstance(v, float) and v > 0 for k, v in one.items())
    assert all(abs(many[0][k] - v) < 1e-6 for k, v in one.items())
    dn = GpuDenseProvider(eng, tok, pooling="cls")
    v = dn.embed_text(texts[1])
    assert len(v) == cfg.hidden_size == dn.get_dimension() and abs(np.linalg.norm(v) - 1) < 1e-5
    # CLS pooling == the first token's hidden state, L2-normalised
    ids = sp._encode([texts[1]])[0]
    ref = O.dense_pool(B.encoder_forward(cfg, W, [min(i, cfg.vocab_size - 1) for i in ids]), "cls", True)
    if max(ids) < cfg.vocab_size:
        assert np.abs(np.asarray(v) - ref).max() < 2e-3
    # the query side of a cross-query batch: rows do not depend on their batch mates, bit for bit
    assert sp.embed_queries(texts) == [sp.embed_text(t) for t in texts]
    assert dn.embed_queries(texts) == [dn.embed_text(t) for t in texts]


def test_head_dim_32_minilm_geometry_vs_oracle():
    """all-MiniLM-L6-v2 geometry (H=384, 12 heads x 32): heads are zero-padded to 64 inside the library."""
    from verbatim_rag_amd.engine import BertEncoderEngine

    cfg = B.BertConfig(vocab_size=1024, hidden_size=384, num_hidden_layers=3, num_attention_heads=12,
                       intermediate_size=1536, max_position_embeddings=256)
    W = B.random_weights(cfg, seed=9, kind="bert", mlm=False, std=0.04)
    eng = BertEncoderEngine(_shape(cfg, "bert"), W, max_tokens=2048, max_seqs=8, max_seq_len=256, max_ranges=8)
    try:
        rng = np.random.default_rng(4)
        seqs = [rng.integers(3, cfg.vocab_size, size=n).astype(np.int32) for n in (256, 9, 130, 64)]
        eng.load_batch(seqs)
        eng.load_ranges(list(range(4)), [0] * 4, [len(s) - 1 for s in seqs])
        eng.run()
        got = eng.read_hidden(final_norm=False)
        eng.run_pool(True)
        pooled = eng.read_pool()
        o = 0
        for i, s in enumerate(seqs):
            ref = B.encoder_forward(cfg, W, s)
            assert np.abs(got[o:o + len(s)] - ref).max() < 3e-2, np.abs(got[o:o + len(s)] - ref).max()
            assert np.abs(pooled[i] - O.dense_pool(ref, "mean", True)).max() < 2e-3
            o += len(s)
    finally:
        eng.close()


def test_rejects_unsupported_shapes():
    from verbatim_rag_amd._lib import VragError
    from verbatim_rag_amd.engine import BertEncoderEngine, BertShape
    from verbatim_rag_amd.weights import random_init_bert

    shp = BertShape(vocab_size=128, hidden_size=128, num_hidden_layers=1, num_attention_heads=8, intermediate_size=256,
                    max_position_embeddings=64)   # head_dim 16
    with pytest.raises(VragError, match="head_dim must be 32 or 64"):
        BertEncoderEngine(shp, random_init_bert(shp, mlm=False), max_tokens=256, max_seqs=2, max_seq_len=64, max_ranges=4)


def test_cross_encoder_pairs_vs_transformers_golden():
    """BertForSequenceClassification (4 heads x 32: zero-padded heads; token types 0 / 1; pooler + classifier):
    hidden states and the pair logit against the golden vectors, batched and alone."""
    from verbatim_rag_amd.engine import BertEncoderEngine
    from verbatim_rag_amd.weights import bert_canonical

    z = np.load(os.path.join(GOLD, "bert_pair_tiny.npz"))
    V, H, L, NH, I, P = (int(x) for x in z["cfg"])
    cfg = B.BertConfig(vocab_size=V, hidden_size=H, num_hidden_layers=L, num_attention_heads=NH, intermediate_size=I,
                       max_position_embeddings=P)
    W = bert_canonical({k[3:]: z[k] for k in z.files if k.startswith("sd:")})
    eng = BertEncoderEngine(_shape(cfg, "bert"), W, max_tokens=1024, max_seqs=8, max_seq_len=64, max_ranges=8)
    try:
        assert eng.pair_labels == 1
        seqs = [z[f"ids{i}"] for i in range(3)]
        types = [z[f"types{i}"] for i in range(3)]
        logits = eng.pair_logits(seqs, types)
        hid = eng.read_hidden(final_norm=False)
        o = 0
        for i, s in enumerate(seqs):
            assert np.abs(hid[o:o + len(s)] - z[f"hidden{i}"]).max() < 3e-2
            assert np.abs(logits[i] - z[f"logits{i}"]).max() < 5e-3, (logits[i], z[f"logits{i}"])
            o += len(s)
        alone = eng.pair_logits([seqs[1]], [types[1]])
        assert np.array_equal(alone[0], logits[1]), float(np.abs(alone[0] - logits[1]).max())   # one summation order across the launch-bound configurations
        # without segment ids every token gets type 0: a different (and wrong for pairs) result, not a crash
        eng.load_batch([seqs[1]])
        eng.run()
        h0 = eng.read_hidden(final_norm=False)
        assert np.abs(h0 - z["hidden1"]).max() > 1e-3
    finally:
        eng.close()


def test_one_summation_order_across_the_launch_bound_residual_configurations():
    """a sequence's bits must not depend on the batch it rides in.  At BERT-base width (N = 768) the residual
    GEMMs of a launch-bound batch take, by row count, 64 x 64 tiles with K split over four waves (<= 1 365 rows), one-wave
    64 x 64 tiles (<= 2 730 rows) or 128 x 128 tiles (above) -- csrc/gemm_bf16.hip launch_t; the two forms without a K-split visit
    the K-steps chain by chain and add the chain sums in the K-split's order (KCH), so all three give the same hidden states for
    the same 512-token sequence.  K = 768 (12 K-steps: three per chain) and K = 3 072 (48) are both in this model."""
    from verbatim_rag_amd.engine import BertEncoderEngine

    cfg = B.BertConfig(vocab_size=2048, hidden_size=768, num_hidden_layers=2, num_attention_heads=12,
                       intermediate_size=3072, max_position_embeddings=512)
    W = B.random_weights(cfg, seed=15, kind="bert", std=0.03)
    eng = BertEncoderEngine(_shape(cfg, "bert"), W, max_tokens=8192, max_seqs=32, max_seq_len=512, max_ranges=64)
    try:
        rng = np.random.default_rng(12)
        first = rng.integers(3, cfg.vocab_size, size=512).astype(np.int32)
        others = [rng.integers(3, cfg.vocab_size, size=512).astype(np.int32) for _ in range(11)]
        out = {}
        for n_rows, batch in (("k_split_512_rows", [first]), ("one_wave_2048_rows", [first] + others[:3]),
                              ("tiles_128_6144_rows", [first] + others)):
            eng.load_batch(batch)
            eng.run()
            out[n_rows] = eng.read_hidden(final_norm=False)[:512].copy()
        ref = B.encoder_forward(cfg, W, first)
        assert np.abs(out["k_split_512_rows"] - ref).max() < 3e-2
        assert np.array_equal(out["k_split_512_rows"], out["one_wave_2048_rows"]), float(np.abs(out["k_split_512_rows"] - out["one_wave_2048_rows"]).max())
        assert np.array_equal(out["k_split_512_rows"], out["tiles_128_6144_rows"]), float(np.abs(out["k_split_512_rows"] - out["tiles_128_6144_rows"]).max())
    finally:
        eng.close()


def test_mlm_head_set_again_without_biases_drops_the_old_biases():
    """vrag_encoder_set_mlm_head after a head with biases (vrag_encoder_set_mlm_head_ex): the new head has none, so the SPLADE rows
    equal those of an engine that never had them."""
    from verbatim_rag_amd.engine import BertEncoderEngine

    cfg = B.BertConfig(vocab_size=1024, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                       max_position_embeddings=128)
    W = B.random_weights(cfg, seed=21, kind="bert", std=0.05)
    Wm = {k: v for k, v in W.items() if not k.startswith("mlm.")}
    seqs = [np.random.default_rng(4).integers(3, cfg.vocab_size, size=n).astype(np.int32) for n in (37, 90)]
    a = BertEncoderEngine(_shape(cfg, "bert"), W, max_tokens=512, max_seqs=4, max_seq_len=128, max_ranges=4)
    b = BertEncoderEngine(_shape(cfg, "bert"), Wm, max_tokens=512, max_seqs=4, max_seq_len=128, max_ranges=4)
    try:
        rows = {}
        for name, eng in (("a_biased", a), ("a", a), ("b", b)):
            if name != "a_biased":
                eng.set_mlm_head(W["mlm.dense.w"], W["mlm.ln.w"], W["mlm.dec.b"])
            eng.load_batch(seqs)
            eng.run()
            eng.run_splade()
            rows[name] = eng.read_splade()
        assert not np.array_equal(rows["a_biased"], rows["b"])   # the biases show in the rows: the check below can fail
        assert np.array_equal(rows["a"], rows["b"]), float(np.abs(rows["a"] - rows["b"]).max())
    finally:
        a.close()
        b.close()


def test_token_type_table_set_again_after_graph_capture():
    """A captured layer schedule holds the token-type table's address: setting the table again must not leave a replay reading
    the old one.  Hidden states after the re-set equal those of an engine built with the new table."""
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.engine import BertEncoderEngine, _fp
    from verbatim_rag_amd.weights import bert_canonical

    z = np.load(os.path.join(GOLD, "bert_pair_tiny.npz"))
    V, H, L, NH, I, P = (int(x) for x in z["cfg"])
    cfg = B.BertConfig(vocab_size=V, hidden_size=H, num_hidden_layers=L, num_attention_heads=NH, intermediate_size=I,
                       max_position_embeddings=P)
    W = bert_canonical({k[3:]: z[k] for k in z.files if k.startswith("sd:")})
    new_types = np.ascontiguousarray(np.random.default_rng(5).normal(0.0, 0.05, W["emb.types"].shape).astype(np.float32))
    seqs, types = [z["ids0"], z["ids1"]], [z["types0"], z["types1"]]

    def hidden(eng):
        eng.load_batch(seqs)
        eng.load_token_types(types)
        eng.run()
        return eng.read_hidden(final_norm=False)

    eng = BertEncoderEngine(_shape(cfg, "bert"), W, max_tokens=1024, max_seqs=8, max_seq_len=64, max_ranges=8)
    fresh = BertEncoderEngine(_shape(cfg, "bert"), dict(W, **{"emb.types": new_types}), max_tokens=1024, max_seqs=8,
                              max_seq_len=64, max_ranges=8)
    try:
        for _ in range(4):   # eager twice, then captured and replayed
            old = hidden(eng)
            if eng.graph_stats()[0] > 0:
                break
        assert eng.graph_stats()[0] > 0, "the geometry was never replayed from a graph"
        _lib.check("vrag_encoder_set_token_types",
                   eng._lib.vrag_encoder_set_token_types(eng._h, _fp(new_types), new_types.shape[0]))
        got, want = hidden(eng), hidden(fresh)
        assert not np.array_equal(old, want)   # the new table changes the result: the check below can fail
        assert np.array_equal(got, want), float(np.abs(got - want).max())
    finally:
        eng.close()
        fresh.close()
