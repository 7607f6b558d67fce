"""The host frame of the device tokenizers (csrc/token_frame.h) through its three entries -- vrag_wordpiece_encode, vrag_bpe_encode,
vrag_bpe_encode_offsets -- against HF `tokenizers`: one handle across batches that make every workspace array grow, batches without
a byte of text, and truncation down to the two special tokens.  array_equal on ids, lengths and offsets; nothing may take the host path."""
import random

import numpy as np
import pytest

import bpe_cases
import wordpiece_cases

pytestmark = pytest.mark.gpu
CLS, SEP = 2, 3
ENTRIES = ["vrag_wordpiece_encode", "vrag_bpe_encode", "vrag_bpe_encode_offsets"]
WORDS = ["the", "quick", "brown", "fox", "hello", "world", "it's", "we're", "tokenization", "café", "x=1", "2024", "a,b", "  ", "\n"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("frame")
    return {"wordpiece": wordpiece_cases.write_tokenizer(d / "wp.json", wordpiece_cases.make_vocab(seed=1, n_words=400)),
            "bpe": bpe_cases.write_tokenizer(d / "bpe.json", **bpe_cases.VARIANTS["nfc_runs"])}


@pytest.fixture(params=ENTRIES)
def check(request, files):
    """check(texts, add_special_tokens, max_length) on ONE fresh handle of the entry: the device's result equals HF's; returns it."""
    from tokenizers import Tokenizer

    from verbatim_rag_amd.bpe import GpuByteBpeTokenizer
    from verbatim_rag_amd.wordpiece import GpuWordPieceTokenizer

    kind = "wordpiece" if request.param == "vrag_wordpiece_encode" else "bpe"
    gpu = (GpuWordPieceTokenizer if kind == "wordpiece" else GpuByteBpeTokenizer).from_file(files[kind])
    hf = Tokenizer.from_file(files[kind])
    assert (gpu.cls_token_id, gpu.sep_token_id) == (CLS, SEP)
    with_offsets = request.param == "vrag_bpe_encode_offsets"

    def run(texts, add_special_tokens, max_length=512):
        keep = max_length - 2 if add_special_tokens else max_length
        want_ids, want_off = [], []
        for e in hf.encode_batch(list(texts), add_special_tokens=False):
            i, o = list(e.ids)[:keep], [tuple(x) for x in e.offsets][:keep]
            want_ids.append([CLS] + i + [SEP] if add_special_tokens else i)
            want_off.append([(0, 0)] + o + [(0, 0)] if add_special_tokens else o)
        if with_offsets:
            ids, offsets, lens = gpu.encode_batch_offsets(texts, add_special_tokens=add_special_tokens, max_length=max_length)
            assert offsets.dtype == np.int32 and offsets.shape == (len(ids), 2)
            assert np.array_equal(offsets, np.asarray([o for w in want_off for o in w], np.int32).reshape(-1, 2))
        else:
            ids, lens = gpu.encode_batch(texts, add_special_tokens=add_special_tokens, max_length=max_length)
        assert ids.dtype == np.int32 and lens.dtype == np.int32
        assert np.array_equal(lens, [len(w) for w in want_ids])
        assert np.array_equal(ids, np.asarray([i for w in want_ids for i in w], np.int32))
        assert gpu.fallback_count == 0
        return want_ids, want_off

    yield run
    gpu.close()


def test_one_handle_across_growing_and_shrinking_batches(check):
    rng = random.Random(11)
    middle = []
    while len(middle) < 300:
        t = " ".join(rng.choice(WORDS) for _ in range(8))
        if 32 <= len(t.encode("utf-8")) <= 48:
            middle.append(t)
    assert sum(len(t.encode("utf-8")) for t in middle) > 2 * 4096       # three tiles: both tile boundaries lie inside the batch
    for special in (True, False):
        check(["hello world", "it's", "café 2024"], special)
        want, _ = check(middle, special)
        assert min(len(w) for w in want) > (2 if special else 0)
        check(["the quick brown fox"], special)


def test_batches_without_a_byte_of_text(check):
    want, want_off = check(["", "", "", ""], True)
    assert want == [[CLS, SEP]] * 4 and want_off == [[(0, 0), (0, 0)]] * 4
    want, _ = check(["", "", "", ""], False)
    assert want == [[]] * 4
    check([""], True)


def test_max_length_two_keeps_only_the_special_tokens(check):
    texts = ["hello world " * 400, "x", "", "tokenization it's " * 500]
    assert len(texts[0]) > 4096 and len(texts[3]) > 2 * 4096
    want, want_off = check(texts, True, max_length=2)
    assert want == [[CLS, SEP]] * 4 and want_off == [[(0, 0), (0, 0)]] * 4
    want, _ = check(texts, True, max_length=3)
    assert [len(w) for w in want] == [3, 3, 2, 3]
