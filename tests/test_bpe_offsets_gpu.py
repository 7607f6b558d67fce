"""`GpuByteBpeTokenizer.encode_batch_offsets` (csrc/bpe.hip, `vrag_bpe_encode_offsets`) against HF `tokenizers` built from the same
seeded tokenizer.json: array_equal on ids, offsets and lengths, `fallback_count` deltas asserted exactly."""
import numpy as np
import pytest

from bpe_cases import VARIANTS, write_tokenizer
from test_bpe_gpu import EDGE

pytestmark = pytest.mark.gpu
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
    ids, offsets = [], []
    for e in hf.encode_batch(list(texts), add_special_tokens=False):
        keep = max_length - 2 if add_special_tokens else max_length
        i, o = list(e.ids)[:keep], [tuple(x) for x in e.offsets][:keep]
        ids.append([CLS] + i + [SEP] if add_special_tokens else i)
        offsets.append([(0, 0)] + o + [(0, 0)] if add_special_tokens else o)
    return ids, offsets


def _check(pair, texts, add_special_tokens=False, max_length=2 ** 20, fallbacks=0):
    gpu, hf, _name = pair
    before = gpu.fallback_count
    ids, offsets, lens = gpu.encode_batch_offsets(texts, add_special_tokens=add_special_tokens, max_length=max_length)
    want_ids, want_off = _hf(hf, texts, add_special_tokens, max_length)
    assert ids.dtype == np.int32 and offsets.dtype == np.int32 and lens.dtype == np.int32 and offsets.shape == (len(ids), 2)
    assert np.array_equal(lens, [len(w) for w in want_ids])
    assert np.array_equal(ids, [i for w in want_ids for i in w])
    flat = np.asarray([o for w in want_off for o in w], np.int32).reshape(-1, 2)
    if not np.array_equal(offsets, flat):
        o = 0
        for t, w in zip(texts, want_off):
            assert [tuple(x) for x in offsets[o:o + len(w)].tolist()] == w, repr(t[:80])
            o += len(w)
    assert gpu.fallback_count - before == fallbacks
    # and the ids route is what it was
    assert np.array_equal(gpu.encode_batch(texts, add_special_tokens=add_special_tokens, max_length=max_length)[0], ids)
    gpu.fallback_count = before + fallbacks
    return want_off


def test_edge_texts(pair):
    _check(pair, EDGE)
    _check(pair, EDGE, add_special_tokens=True)
    _check(pair, [])


def test_space_runs_and_truncation(pair):
    texts = []
    for r in range(1, 51):
        s = " " * r
        texts += [s + "ab", "ab" + s + "cd", "ab" + s + "'s", "ab\n" + s + "cd", "ab" + s, s, "a" + s + "\n", "a" + s + "1" + s + "."]
    _check(pair, texts)
    for special in (True, False):
        want = _check(pair, texts, add_special_tokens=special, max_length=8)
        assert max(len(w) for w in want) == 8 and min(len(w) for w in want) < 8


def test_pre_token_of_64_bytes_and_multi_byte_characters(pair):
    want = _check(pair, ["x\n" + "a" * 64 + "\ny", "\U0001F600", "\u00e9" * 32, "=" * 64, "a\U0001F600\U0001F601b"])
    assert set(want[1]) == {(0, 1)} and len(want[1]) > 1      # byte-fallback ids share their character
    _check(pair, ["x\n" + "a" * 65 + "\ny", "ok"], fallbacks=1)      # beyond the cap: ids and offsets from the host


def test_tile_boundaries(pair):
    """The probes of tests/test_bpe_gpu.py::test_tile_boundaries, each starting at every byte offset boundary-8 .. boundary+8 of
    the first two tile boundaries: the lead-byte count crosses lanes and tiles; the 4-byte character straddles the boundary at
    offsets boundary-3 .. boundary-1.  Multi-byte padding in front makes byte and character indices differ by thousands."""
    from verbatim_rag_amd.bpe import TILE_BYTES

    probes = ["tokenization", " " * 11 + "x", "\U0001F600", "'ll", "  're"]
    texts = []
    for boundary in (TILE_BYTES, 2 * TILE_BYTES):
        for at in range(boundary - 8, boundary + 9):
            pad = ("ab " * (at // 3 + 1))[:at - 1] + "a"
            wide = ("\u00e9b " * (at // 4 + 1))[:(at - 1) // 4 * 3]
            wide += "a" * (at - len(wide.encode("utf-8")))
            assert len(pad.encode("utf-8")) == at == len(wide.encode("utf-8"))
            texts += [pad + p + " tail" for p in probes] + [wide + p + " tail" for p in probes[:3]]
    _check(pair, texts)


def test_per_text_base_behind_multi_byte_text(pair):
    """The second and later texts start mid-tile behind multi-byte text: offsets count from their own first character."""
    want = _check(pair, ["\u00e9" * 3000, "", "日本 x", "a"], fallbacks=1)      # 6000 bytes in one pre-token: the host's
    assert want[2][0][0] == 0 and want[3] == [(0, 1)]
    want = _check(pair, ["\u00e9 " * 3000, "", "日本 x", "a", "\U0001F600 " * 1100, "caf\u00e9"])
    assert want[2][0][0] == 0 and want[3] == [(0, 1)] and want[5][0][0] == 0


def test_one_200_kb_text(pair):
    import random

    rng = random.Random(5)
    words = ["hello", "world", "it's", "tokenization", "caf\u00e9", "中文", "  ", "Hello,", "na\u00efve!", "мир", "a1b2", "...", "\n", "   "]
    long_text = " ".join(rng.choice(words) for _ in range(60000))[:200000]
    assert len(long_text.encode("utf-8")) >= 200000
    _check(pair, ["x", long_text, "", "y"])


def test_flagged_texts_take_offsets_from_the_host(pair):
    """A text the device cannot prove NFC, and a private-use character: ids AND offsets are HF's (which refer to the text as given)."""
    on_device = pair[2] == "raw_runs48"      # normalizer: null -- nothing to prove
    _check(pair, ["cafe\u0301", "plain caf\u00e9"], fallbacks=0 if on_device else 1)
    _check(pair, ["hello \ue000 world", "plain"], fallbacks=1)
    _check(pair, ["hello \ue000 world", "cafe\u0301 x", "ok"], add_special_tokens=True, max_length=6, fallbacks=1 if on_device else 2)
