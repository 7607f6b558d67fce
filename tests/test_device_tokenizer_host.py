"""`DeviceTokenizer` (verbatim_rag_amd/device_tokenizer.py) without a GPU: the routing of texts around the device call, the sizing
of that call and the splice of host-tokenised texts into the packed device batch, with the device call replaced by a stub that
returns prepared ids, offsets, lengths and flags."""
import re
from types import SimpleNamespace

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd.device_tokenizer import DeviceTokenizer

CLS, SEP = 1, 2


class FakeHF:
    """Stands in for `tokenizers.Tokenizer`: one id per whitespace-separated word (its length), offsets = the word's characters."""
    copies = 0

    def to_str(self):
        return "fake"

    @classmethod
    def from_str(cls, s):
        assert s == "fake"
        cls.copies += 1
        return cls()

    def no_truncation(self):
        self.truncation = None

    def no_padding(self):
        self.padding = None

    def encode(self, text, add_special_tokens=False):
        assert not add_special_tokens
        words = list(re.finditer(r"\S+", text))
        return SimpleNamespace(ids=[len(m.group()) for m in words], offsets=[m.span() for m in words])


class StubTokenizer(DeviceTokenizer):
    """The device call answers with `reply` = (ids, offsets, seq_lens, needs_host) and records what it was asked."""
    _destroy_entry = "stub_destroy"

    def __init__(self, reply=None):
        super().__init__(FakeHF(), CLS, SEP, 100)
        self.destroyed, self.calls, self.reply = [], [], reply
        self._lib = SimpleNamespace(stub_destroy=self.destroyed.append)
        self._h = "handle"

    def _goes_to_host(self, texts):
        return {d for d, t in enumerate(texts) if "[MASK]" in t}

    def encode_batch_offsets(self, texts, add_special_tokens=False, max_length=512):
        return self._encode(texts, add_special_tokens, max_length, True)

    def _device_encode(self, blob, off, add_special_tokens, max_length, cap, with_offsets):
        self.calls.append(SimpleNamespace(blob=blob, off=off.copy(), special=add_special_tokens, max_length=max_length, cap=cap,
                                          with_offsets=with_offsets))
        ids, offsets, seq_lens, needs = self.reply
        assert len(seq_lens) == len(needs) == len(off) - 1 and len(ids) == sum(seq_lens) <= max(cap, 0)
        return (np.asarray(ids, np.int32), np.asarray(offsets, np.int32).reshape(-1, 2) if with_offsets else None,
                np.asarray(seq_lens, np.int32), np.asarray(needs, np.uint8))


class OffByOneStarts(StubTokenizer):
    """Negative control: the device's texts are cut one id too far to the right."""

    def _splice(self, texts, host, ids, offsets, seq_lens, add_special_tokens, max_length):
        shifted = np.concatenate([ids[1:], ids[:1]])
        return super()._splice(texts, host, shifted, offsets, seq_lens, add_special_tokens, max_length)


class StaleSeqLens(StubTokenizer):
    """Negative control: the lengths of the host-tokenised texts stay the device's."""

    def _splice(self, texts, host, ids, offsets, seq_lens, add_special_tokens, max_length):
        return super()._splice(texts, host, ids, offsets, seq_lens.copy(), add_special_tokens, max_length)[:2] + (seq_lens,)


# Five texts with specials, max_length 16.  0 and 4 hold an added token (never shown to the device), 2 is flagged by the device.
TEXTS5 = ["[MASK] aa", "bbb c", "dd zz", "e", "ffff [MASK] g"]
DEV5 = dict(ids=[CLS, SEP, CLS, 50, 51, SEP, CLS, 60, SEP, CLS, 70, SEP, CLS, SEP],
            offsets=[(0, 0), (0, 0), (0, 0), (0, 3), (4, 5), (0, 0), (0, 0), (0, 5), (0, 0), (0, 0), (0, 1), (0, 0), (0, 0), (0, 0)],
            seq_lens=[2, 4, 3, 3, 2], needs=[0, 0, 1, 0, 0])
WANT5 = dict(ids=[CLS, 6, 2, SEP, CLS, 50, 51, SEP, CLS, 2, 2, SEP, CLS, 70, SEP, CLS, 4, 6, 1, SEP],
             offsets=[(0, 0), (0, 6), (7, 9), (0, 0), (0, 0), (0, 3), (4, 5), (0, 0), (0, 0), (0, 2), (3, 5), (0, 0), (0, 0), (0, 1), (0, 0),
                      (0, 0), (0, 4), (5, 11), (12, 13), (0, 0)],
             seq_lens=[4, 4, 4, 3, 5])


def check_splice5(cls, with_offsets):
    tok = cls((DEV5["ids"], DEV5["offsets"], DEV5["seq_lens"], DEV5["needs"]))
    if with_offsets:
        ids, offsets, lens = tok.encode_batch_offsets(TEXTS5, add_special_tokens=True, max_length=16)
        assert offsets.dtype == np.int32 and offsets.tolist() == [list(p) for p in WANT5["offsets"]]
    else:
        ids, lens = tok.encode_batch(TEXTS5, add_special_tokens=True, max_length=16)
    assert ids.dtype == np.int32 and lens.dtype == np.int32
    assert lens.tolist() == WANT5["seq_lens"]
    assert ids.tolist() == WANT5["ids"]
    assert tok.fallback_count == 3 and len(tok.calls) == 1
    return tok


@pytest.mark.parametrize("with_offsets", [False, True], ids=["ids", "offsets"])
def test_flagged_texts_at_the_first_a_middle_and_the_last_position(with_offsets):
    before = FakeHF.copies
    tok = check_splice5(StubTokenizer, with_offsets)
    assert FakeHF.copies == before + 1 and tok._hf.truncation is None and tok._hf.padding is None      # its own copy of the HF tokenizer
    assert tok.calls[0].with_offsets == with_offsets and tok.calls[0].special is True


@pytest.mark.parametrize("with_offsets", [False, True], ids=["ids", "offsets"])
@pytest.mark.parametrize("broken", [OffByOneStarts, StaleSeqLens])
def test_a_wrong_splice_does_not_pass_the_check_above(broken, with_offsets):
    with pytest.raises(AssertionError):
        check_splice5(broken, with_offsets)


def test_splice_when_the_device_or_the_host_length_is_zero():
    # text 0: nothing on the device (routed), two ids on the host; text 1: three ids on the device (flagged), none on the host
    tok = StubTokenizer(([7, 8, 9, 30], [(0, 1), (1, 2), (2, 3), (0, 1)], [0, 3, 1], [0, 1, 0]))
    ids, offsets, lens = tok.encode_batch_offsets(["[MASK] q", "   ", "r"], add_special_tokens=False, max_length=8)
    assert ids.tolist() == [6, 1, 30] and lens.tolist() == [2, 0, 1] and offsets.tolist() == [[0, 6], [7, 8], [0, 1]]
    assert tok.fallback_count == 2
    tok.reply = ([7, 8, 9], None, [0, 3], [0, 1])       # every text goes to the host, and the last one has no ids there
    ids, lens = tok.encode_batch(["[MASK]", "   "], add_special_tokens=False, max_length=4)
    assert ids.tolist() == [6] and lens.tolist() == [1, 0] and ids.dtype == np.int32


def test_unencodable_and_added_token_texts_never_reach_the_device():
    texts = ["plain é", "lone \ud800 surrogate", "has [MASK] inside", "tail"]
    tok = StubTokenizer(([40, 41, 42], None, [2, 0, 0, 1], [0, 0, 0, 0]))
    ids, lens = tok.encode_batch(texts, add_special_tokens=False, max_length=8)
    call = tok.calls[0]
    seen = [call.blob[call.off[d]:call.off[d + 1]] for d in range(4)]
    assert seen == ["plain é".encode("utf-8"), b"", b"", b"tail"] and call.off.dtype == np.int64 and call.off[0] == 0
    assert lens.tolist() == [2, 3, 3, 1] and ids.tolist() == [40, 41, 4, 1, 9, 3, 6, 6, 42] and tok.fallback_count == 2


def test_argument_checks_empty_batch_and_closed_tokenizer():
    tok = StubTokenizer()
    with pytest.raises(ValueError, match="max_length 1 leaves no room for the special tokens"):
        tok.encode_batch(["a"], add_special_tokens=True, max_length=1)
    with pytest.raises(ValueError, match="max_length -1 leaves no room"):
        tok.encode_batch(["a"], add_special_tokens=False, max_length=-1)
    ids, lens = tok.encode_batch([])
    assert (ids.dtype, ids.shape, lens.dtype, lens.shape) == (np.int32, (0,), np.int32, (0,))
    ids, offsets, lens = tok.encode_batch_offsets([])
    assert (ids.shape, offsets.dtype, offsets.shape, lens.shape) == ((0,), np.int32, (0, 2), (0,))
    assert tok.ids_batch([], max_length=8) == [] and tok.calls == []
    tok.close()
    tok.close()
    assert tok.destroyed == ["handle"]
    with pytest.raises(RuntimeError, match="StubTokenizer is closed"):
        tok.encode_batch(["a"])
    assert tok.encode_batch([])[0].shape == (0,) and tok.calls == []      # as before: an empty batch needs no handle


@pytest.mark.parametrize("texts,special,max_length,cap", [
    (["abcd", "é", ""], True, 512, 6 + 2 * 3),            # bytes + 2 per text
    (["abcd", "é", ""], False, 512, 6 + 2 * 3),           # the same rule without specials: an upper bound only
    (["x" * 100, "y" * 50], True, 8, 8 * 2),              # max_length per text
    (["x" * 100, "[MASK]" * 9], True, 60, 100 + 2 * 2),   # a routed text counts no bytes
    ([""], False, 0, 0),
])
def test_cap_is_the_smaller_of_bytes_plus_specials_and_max_length_per_text(texts, special, max_length, cap):
    n = len(texts)
    tok = StubTokenizer(([], None, [0] * n, [0] * n))
    tok.encode_batch(texts, add_special_tokens=special, max_length=max_length)
    assert tok.calls[0].cap == cap and isinstance(tok.calls[0].cap, int) and tok.calls[0].max_length == max_length


def test_ids_batch_splits_on_the_lengths():
    tok = StubTokenizer(([5, 6, 7, 8], None, [0, 3, 0, 1, 0], [0] * 5))
    assert tok.ids_batch(["", "a b c", "", "d", ""], max_length=8) == [[], [5, 6, 7], [], [8], []]
    assert tok.calls[0].special is False and tok.calls[0].max_length == 8
    tok.reply = ([CLS, 5, SEP], None, [3], [0])
    assert tok.ids("a", True, 8) == [CLS, 5, SEP]
