"""Device byte-level BPE tokenizer (csrc/bpe.hip) against HF `tokenizers` built from the same seeded tokenizer.json: every
comparison is array_equal on ids and lengths, and `fallback_count` deltas are asserted exactly.

The code-point sweep's first set is every code point of the required blocks that the table's generator covers (assigned in its
`unicodedata`, not left to the host by name) and that has NFC_Quick_Check = Yes; for those no fallback is allowed.  Every other
code point of the blocks is swept separately and must take the host path (with the `normalizer: null` variant only the
uncovered ones do)."""
import json
import os

import numpy as np
import pytest

from bpe_cases import VARIANTS, table, write_tokenizer

pytestmark = pytest.mark.gpu
BLOCKS = [(0x0000, 0x024F), (0x0370, 0x03FF), (0x0400, 0x04FF), (0x0590, 0x05FF), (0x0600, 0x06FF), (0x0900, 0x097F), (0x2000, 0x206F),
          (0x3000, 0x30FF), (0x1F300, 0x1FAFF)]
SAMPLED = [(0x4E00, 0x9FFF), (0xAC00, 0xD7A3)]      # every 16th
CLS, SEP = 2, 3


@pytest.fixture(scope="module", params=list(VARIANTS))
def pair(request, tmp_path_factory):
    """(device tokenizer, HF tokenizer, variant name) over one vocabulary of about 1 200 ids."""
    from tokenizers import Tokenizer

    from verbatim_rag_amd.bpe import GpuByteBpeTokenizer

    path = write_tokenizer(tmp_path_factory.mktemp(request.param) / "tokenizer.json", **VARIANTS[request.param])
    gpu = GpuByteBpeTokenizer.from_file(path)
    assert 1200 <= gpu.vocab_size <= 1230 and (gpu.cls_token_id, gpu.sep_token_id) == (CLS, SEP)
    yield gpu, Tokenizer.from_file(path), request.param
    gpu.close()


def _hf(hf, texts, add_special_tokens, max_length):
    out = []
    for e in hf.encode_batch(list(texts), add_special_tokens=False):
        body = list(e.ids)
        out.append([CLS] + body[:max_length - 2] + [SEP] if add_special_tokens else body[:max_length])
    return out


def _check(pair, texts, add_special_tokens=True, max_length=512, fallbacks=0):
    gpu, hf, _name = pair
    before = gpu.fallback_count
    ids, lens = gpu.encode_batch(texts, add_special_tokens=add_special_tokens, max_length=max_length)
    want = _hf(hf, texts, add_special_tokens, max_length)
    assert ids.dtype == np.int32 and lens.dtype == np.int32
    assert np.array_equal(lens, [len(w) for w in want])
    flat = [i for w in want for i in w]
    if not np.array_equal(ids, flat):
        o = 0
        for t, w in zip(texts, want):
            assert ids[o:o + len(w)].tolist() == w, repr(t[:80])
            o += len(w)
    assert gpu.fallback_count - before == fallbacks
    return want


def test_hf_template_is_what_the_oracle_assumes(pair):
    _gpu, hf, _name = pair
    assert hf.encode("hello world").ids == [CLS] + hf.encode("hello world", add_special_tokens=False).ids + [SEP]


EDGE = ["", " ", "a", "a's", "a 's", "!'s", "a\n's", "A'S", "a'll", "a'l", "''s", "a's's", "a'sb", "we're they've I'm he'd don't", "abc123",
        "!!!...???", "--(([[", "a,b;c", "x \n", "x\t\ty", "\ta", " \t\r\n ", "a\u00a0b", "a\u3000b", "a\u0085b", "\u00a0 x", "caf\u00e9 na\u00efve",
        "\u043f\u0440\u0438\u0432\u0435\u0442 \u043c\u0438\u0440", "\u4e2d\u6587 \u6771\u4eac", "\U0001F468\u200d\U0001F469\u200d\U0001F467 family",
        "the quick brown fox tokenizer tokenization", "Hello World", "a  's", "x  ", "  x", "a   b", " '", "' s", "1's 2'll", "\n's", "a\n\n b", "a \n b",
        " 's", "a\u2028\u2028b", "a \u00a0b", "a\u00a0 b"]


def test_edge_texts(pair):
    _check(pair, EDGE)
    _check(pair, EDGE, add_special_tokens=False)
    for t in EDGE[:16]:      # and one text at a time, through ids()
        assert pair[0].ids(t, add_special_tokens=True, max_length=512) == _hf(pair[1], [t], True, 512)[0]


def test_space_runs(pair):
    texts = []
    for r in range(1, 51):
        s = " " * r
        texts += [s + "ab", "ab" + s + "cd", "ab" + s + "'s", "ab\n" + s + "cd", "ab" + s, s, "a" + s + "\n", "a" + s + "1" + s + "."]
    _check(pair, texts)
    _check(pair, texts, add_special_tokens=False, max_length=8)


def test_tile_boundaries(pair):
    """A pre-token, a space run, a 4-byte character and a contraction (behind a letter, and behind a double space) each placed so
    that they start at every byte offset boundary-8 .. boundary+8 of the first two tile boundaries; then one run of 5 000 spaces."""
    from verbatim_rag_amd.bpe import TILE_BYTES

    probes = ["tokenization", " " * 11 + "x", "\U0001F600", "'ll", "  're"]
    texts = []
    for boundary in (TILE_BYTES, 2 * TILE_BYTES):
        for at in range(boundary - 8, boundary + 9):
            pad = ("ab " * (at // 3 + 1))[:at - 1] + "a"
            assert len(pad.encode("utf-8")) == at
            texts += [pad + p + " tail" for p in probes]
    _check(pair, texts)
    # without space-run tokens the run is ONE pre-token of white space, far beyond the 64-byte cap: those four texts go to the host
    long_runs = ["a" + " " * 5000 + "b", " " * 5000, "a" + " " * 4095, "a" + " " * 4096 + "'s"]
    _check(pair, texts[::7] + long_runs, fallbacks=0 if VARIANTS[pair[2]]["runs"] else len(long_runs))
    # a contraction across the boundary behind more spaces than the byte-by-byte look-back in front of a tile counts (256): given up
    far = "a" + " " * 300
    text = ("ab " * TILE_BYTES)[:TILE_BYTES - 1 - len(far)] + far + "'re x"
    assert text.encode("utf-8")[TILE_BYTES - 1:TILE_BYTES + 2] == b"'re"
    _check(pair, [text, "plain"], fallbacks=1)


def test_pre_token_length(pair):
    from verbatim_rag_amd.bpe import MAX_WORD_BYTES

    assert MAX_WORD_BYTES == 64
    _check(pair, ["x\n" + "a" * n + "\ny" for n in (63, 64)] + ["\u00e9" * 32, "x " + "a" * 63 + " y", "=" * 64], fallbacks=0)      # 64 = the cap
    _check(pair, ["x\n" + "a" * 65 + "\ny", "ok"], fallbacks=1)
    _check(pair, ["=" * 1000, "x " + "a" * 64 + " y", "\u00e9" * 32 + "a"], fallbacks=3)      # the space in front joins: 65 bytes


@pytest.mark.parametrize("max_length", [8, 512])
def test_truncation(pair, max_length):
    texts = [" ".join(["a"] * n) for n in range(max_length - 3, max_length + 2)]
    texts += ["q" * n for n in range(max_length - 3, max_length + 2) if n <= 64]
    texts += [" ".join(["ab"] * (max_length // 2 - 1)) + " tokenization" * k for k in range(3)]
    for special in (True, False):
        want = _check(pair, texts, add_special_tokens=special, max_length=max_length)
        assert max(len(w) for w in want) == max_length and min(len(w) for w in want) < max_length


def test_batch_geometry(pair):
    import random

    rng = random.Random(5)
    _check(pair, [])
    _check(pair, ["hello world"])
    tiny = [rng.choice(["", "", "a", "ab", " a ", "'s", "\u00e9", "  ", "1 2", "\u4e2d"]) for _ in range(1000)]
    assert all(len(t.encode("utf-8")) <= 3 for t in tiny) and tiny.count("") > 100
    _check(pair, tiny)
    words = ["hello", "world", "it's", "tokenization", "caf\u00e9", "\u4e2d\u6587", "  ", "Hello,", "na\u00efve!", "\u043c\u0438\u0440", "a1b2", "...", "\n", "   "]
    long_text = " ".join(rng.choice(words) for _ in range(60000))[:200000]
    assert len(long_text.encode("utf-8")) >= 200000
    _check(pair, ["x", long_text, "", "y"], max_length=2 ** 20)


def test_nfc(pair):
    on_device = pair[2] == "raw_runs48"      # normalizer: null -- nothing to prove
    _check(pair, ["caf\u00e9"], fallbacks=0)
    _check(pair, ["cafe\u0301", "plain"], fallbacks=0 if on_device else 1)
    _check(pair, ["a\u0301\u0327 x", "plain"], fallbacks=0 if on_device else 1)      # combining classes 230 then 202
    _check(pair, ["a\u0327\u0301 x"], fallbacks=0 if on_device else 1)               # in order, but both marks are NFC_QC = Maybe
    assert table.nfc_qc_yes(0x05B0) and table.nfc_qc_yes(0x05B1)      # Hebrew points, combining classes 10 and 11: only their order matters
    _check(pair, ["\u05d0\u05b0\u05b1 x"], fallbacks=0)
    _check(pair, ["\u05d0\u05b1\u05b0 x", "plain"], fallbacks=0 if on_device else 1)


def _sweep_text(c):
    ch = chr(c)
    return "a" + ch + "b " + ch + ch + " 1" + ch


def test_code_point_sweep(pair):
    nfc = pair[2] != "raw_runs48"
    cps = [c for a, b in BLOCKS for c in range(a, b + 1)] + [c for a, b in SAMPLED for c in range(a, b + 1, 16)]
    cps = [c for c in cps if not 0xD800 <= c <= 0xDFFF]
    first = [c for c in cps if table.covered(c) and table.nfc_qc_yes(c)]
    rest = [c for c in cps if c not in set(first)]
    assert len(first) > 5000 and 0 < len(rest) < 1500
    assert len([c for c in cps if table.assigned(c) and table.nfc_qc_yes(c)]) - len(first) <= 16
    _check(pair, [_sweep_text(c) for c in first], fallbacks=0)
    expected = len(rest) if nfc else len([c for c in rest if not table.covered(c)])
    _check(pair, [_sweep_text(c) for c in rest], fallbacks=expected)


def test_private_use_and_added_tokens_take_the_host_path(pair):
    texts = ["hello \ue000 world", "hello [SEP] world", "a [MASK] b", "hello world"]
    want = _check(pair, texts, fallbacks=3)
    assert SEP in want[1][1:-1] and 4 in want[2]      # HF matched the added tokens


def test_capacity_status_through_the_c_abi(pair):
    import ctypes as C

    from verbatim_rag_amd import _lib

    gpu, hf, _name = pair
    blob = b"hello world"
    n_want = len(hf.encode("hello world", add_special_tokens=False).ids) + 2
    off = np.array([0, len(blob)], np.int64)
    lens, needs, n_ids = np.zeros(1, np.int32), np.zeros(1, np.uint8), C.c_int64(0)
    ids = np.zeros(1, np.int32)
    rc = _lib.load().vrag_bpe_encode(gpu._h, C.cast(C.c_char_p(blob), C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), 1, 1, 512,
                                     1, ids.ctypes.data_as(C.POINTER(C.c_int32)), lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                     needs.ctypes.data_as(C.c_void_p), C.byref(n_ids))
    assert rc == -3 and n_ids.value == lens[0] == n_want and needs[0] == 0


# ------------------------------------------------------------------------------------------ wiring
QUESTION = "what's the  tallest tower?"
CHUNKS = ["The tower is 300 m tall. It's made of iron.  Gustave's firm built it.", "Nothing here.  We're done! caf\u00e9 \u4e2d\u6587.",
          "One sentence only", "a  b. c's d? " * 12]


def _modernbert_dir(path, kind, seed=5):
    """A tiny random ModernBERT checkpoint directory with a synthetic byte-level BPE tokenizer.json ([CLS] = 2, [SEP] = 3).
    Built here, as tests/test_checkpoint_loading.py builds its directories, rather than from the `encoder_tiny` /
    `modernbert_seqcls_tiny` goldens: `tokenizer="gpu"` is an argument of the constructors that take a checkpoint DIRECTORY
    (config.json + safetensors + tokenizer.json), which the .npz goldens are not, and their [CLS] / [SEP] ids (1, 2) are not the
    synthetic tokenizer's."""
    import torch
    import transformers
    from safetensors.numpy import save_file

    os.makedirs(path, exist_ok=True)
    torch.manual_seed(seed)
    hc = transformers.ModernBertConfig(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=192,
                                       max_position_embeddings=8192, pad_token_id=0, cls_token_id=CLS, sep_token_id=SEP, bos_token_id=CLS,
                                       eos_token_id=SEP, num_labels=1)
    if kind == "qa":
        m = transformers.ModernBertModel(hc).eval()
        rng = np.random.default_rng(seed)
        sd = {"bert." + k: v.numpy() for k, v in m.state_dict().items()}
        sd["classifier.weight"], sd["classifier.bias"] = rng.standard_normal((2, 128)).astype(np.float32), rng.standard_normal(2).astype(np.float32)
        save_file(sd, os.path.join(path, "model.safetensors"))
        hc.save_pretrained(path)
    else:
        cls = {"mlm": transformers.ModernBertForMaskedLM, "seqcls": transformers.ModernBertForSequenceClassification,
               "dense": transformers.ModernBertModel}[kind]
        cls(hc).eval().save_pretrained(path, safe_serialization=True)
    write_tokenizer(os.path.join(path, "tokenizer.json"), vocab_size=480, **VARIANTS["nfc_runs"])
    return str(path)


def test_load_model_tokenizer_dispatches_on_the_file(tmp_path):
    from verbatim_rag_amd.bpe import GpuByteBpeTokenizer
    from verbatim_rag_amd.embedding_providers import load_model_tokenizer

    write_tokenizer(tmp_path / "tokenizer.json", **VARIANTS["nfc_plain"])
    tok = load_model_tokenizer(str(tmp_path), "gpu")
    try:
        assert isinstance(tok, GpuByteBpeTokenizer) and tok.ids("it's", True, 16)[0] == CLS
    finally:
        tok.close()
    spec = json.load(open(tmp_path / "tokenizer.json", encoding="utf-8"))
    spec["pre_tokenizer"]["add_prefix_space"] = True
    json.dump(spec, open(tmp_path / "tokenizer.json", "w", encoding="utf-8"))
    with pytest.raises(ValueError, match="add_prefix_space"):
        load_model_tokenizer(str(tmp_path), "gpu")


def test_extractor_with_the_device_tokenizer_equals_the_host_tokenizer(tmp_path):
    from verbatim_rag_amd.bpe import GpuByteBpeTokenizer
    from verbatim_rag_amd.extractors import GpuModelSpanExtractor

    d = _modernbert_dir(tmp_path / "qa", "qa")
    kw = dict(threshold=0.5, min_span_chars=1, qa_max_length=128, max_batch_tokens=4096, max_batch_seqs=32)
    host = GpuModelSpanExtractor(d, tokenizer="host", **kw)
    dev = GpuModelSpanExtractor(d, tokenizer="gpu", **kw)
    assert isinstance(dev.tokenizer, GpuByteBpeTokenizer) and dev._tok is dev.tokenizer

    class Doc:
        def __init__(self, text):
            self.text = text

    docs = [Doc(t) for t in CHUNKS]
    a, b = host.extract_spans(QUESTION, docs), dev.extract_spans(QUESTION, docs)
    assert a == b and len(a) == len(CHUNKS)
    packed = [[(s.input_ids, s.sentence_boundaries) for s in e.pack_qa(QUESTION, CHUNKS)[1]] for e in (host, dev)]      # and the ids behind them
    assert packed[0] == packed[1] and min(len(ids) for ids, _b in packed[0]) > 8
    assert dev.tokenizer.fallback_count == 0
    cfg = json.load(open(os.path.join(d, "config.json")))
    cfg["auto_map"] = {"AutoModel": "modeling.ZeroEntropyHighlighter"}
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    with pytest.raises(ValueError, match="character offsets"):
        GpuModelSpanExtractor(d, tokenizer="gpu", **kw)
    with pytest.raises(ValueError, match="'host', 'gpu'"):
        GpuModelSpanExtractor(d, tokenizer="device", **kw)


def test_reranker_and_providers_with_the_device_tokenizer_equal_the_host_tokenizer(tmp_path):
    from verbatim_rag_amd.bpe import GpuByteBpeTokenizer
    from verbatim_rag_amd.embedding_providers import GpuDenseProvider, GpuSpladeProvider
    from verbatim_rag_amd.rerankers import GpuCrossEncoderReranker

    texts = CHUNKS + ["", QUESTION]
    host = GpuCrossEncoderReranker.from_directory(_modernbert_dir(tmp_path / "ce", "seqcls"), max_length=128)
    dev = GpuCrossEncoderReranker.from_directory(str(tmp_path / "ce"), max_length=128, tokenizer="gpu")
    assert isinstance(dev.tokenizer, GpuByteBpeTokenizer)
    a, b = host.score(QUESTION, CHUNKS), dev.score(QUESTION, CHUNKS)
    assert a == b and len(set(a)) > 1
    host = GpuSpladeProvider.from_directory(_modernbert_dir(tmp_path / "mlm", "mlm"), max_length=128)
    dev = GpuSpladeProvider.from_directory(str(tmp_path / "mlm"), max_length=128, tokenizer="gpu")
    a, b = host.embed_batch(texts), dev.embed_batch(texts)
    assert a == b and any(a)
    host = GpuDenseProvider.from_directory(_modernbert_dir(tmp_path / "dense", "dense"), max_length=128)
    dev = GpuDenseProvider.from_directory(str(tmp_path / "dense"), max_length=128, tokenizer="gpu")
    assert isinstance(dev.tokenizer, GpuByteBpeTokenizer)
    assert np.array_equal(np.asarray(host.embed_batch(texts)), np.asarray(dev.embed_batch(texts)))
