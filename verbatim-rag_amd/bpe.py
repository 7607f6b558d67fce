"""Byte-level BPE tokenisation on the GPU (csrc/bpe.hip behind `vrag_bpe_*`): the ids HF `tokenizers` returns for the
ModernBERT pipeline [NFC] -> ByteLevel(add_prefix_space=False, use_regex=True) -> BPE -> `[CLS] $A [SEP]`, for a whole batch
of texts in one call.

The device never guesses: a text it cannot vouch for -- a code point the committed table does not cover, a text it cannot
prove to be NFC already, a pre-token of more than `MAX_WORD_BYTES` bytes -- comes back flagged and is tokenised here with the
HF tokenizer the object was built from, as is -- before the device call -- any text that holds the literal content of an added
token other than the runs of spaces the device cuts itself (`[SEP]`, `[MASK]`, `|||IP_ADDRESS|||`, ...) or that is not
encodable as UTF-8.  `fallback_count` counts the texts that went that way."""
from __future__ import annotations

import ctypes as C
import re
import unicodedata
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np

from .device_tokenizer import DeviceTokenizer, _template_ids

TILE_BYTES = 4096        # VRAG_BPE_TILE_BYTES: text bytes per workgroup of the boundary passes
MAX_WORD_BYTES = 64      # VRAG_BPE_MAX_WORD_BYTES: a longer pre-token sends its text to the host
MAX_SPACE_RUN = 64       # VRAG_BPE_MAX_SPACE_RUN
_NFC, _IGNORE_MERGES = 1, 2


def byte_alphabet() -> List[str]:
    """Character of every byte in the byte-level alphabet (GPT-2's `bytes_to_unicode`, as `ByteLevel.alphabet()`)."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    out, extra = [""] * 256, 0
    for b in range(256):
        if b in keep:
            out[b] = chr(b)
        else:
            out[b] = chr(256 + extra)
            extra += 1
    return out


def parse_spec(spec: dict, path: str = "tokenizer.json") -> dict:
    """Everything the device tokenizer needs from a parsed `tokenizer.json`, or ValueError naming the component that is not
    [NFC] / ByteLevel(add_prefix_space=False, use_regex=True) / BPE / `<cls> $A <sep>` TemplateProcessing.  Needs no device."""
    model = spec.get("model") or {}
    if model.get("type") != "BPE":
        raise ValueError(f"{path}: model must be BPE, got {model.get('type')!r}")
    norm = spec.get("normalizer")
    if norm is not None and (not isinstance(norm, dict) or norm.get("type") != "NFC"):
        raise ValueError(f"{path}: normalizer must be null or NFC, got {norm.get('type') if isinstance(norm, dict) else norm!r}")
    pre = spec.get("pre_tokenizer") or {}
    if pre.get("type") != "ByteLevel":
        raise ValueError(f"{path}: pre_tokenizer must be ByteLevel, got {pre.get('type')!r}")
    if pre.get("add_prefix_space", True):
        raise ValueError(f"{path}: pre_tokenizer add_prefix_space must be false")
    if not pre.get("use_regex", True):
        raise ValueError(f"{path}: pre_tokenizer use_regex must be true")
    if model.get("dropout"):
        raise ValueError(f"{path}: model dropout must be null or 0, got {model['dropout']!r}")
    if model.get("byte_fallback"):
        raise ValueError(f"{path}: model byte_fallback must be false")
    for key in ("continuing_subword_prefix", "end_of_word_suffix"):
        if model.get(key):
            raise ValueError(f"{path}: model {key} must be empty, got {model[key]!r}")
    cls_tok, sep_tok = _template_ids(spec.get("post_processor"), path)
    vocab: Dict[str, int] = dict(model["vocab"])
    alphabet = byte_alphabet()
    for b, ch in enumerate(alphabet):
        if ch not in vocab:
            raise ValueError(f"{path}: model vocabulary lacks the byte-level character of byte 0x{b:02X}")
    every = dict(vocab)
    added = spec.get("added_tokens") or []
    for tok in added:
        if every.setdefault(tok["content"], tok["id"]) != tok["id"]:
            raise ValueError(f"{path}: added_tokens entry {tok['content']!r} has id {tok['id']}, the model vocabulary another")
    if sorted(every.values()) != list(range(len(every))):
        raise ValueError(f"{path}: ids of the model vocabulary and the added tokens must be 0 .. n-1 without gaps")
    for name in (cls_tok, sep_tok):
        if name not in every:
            raise ValueError(f"{path}: post_processor special token {name!r} is neither in the model vocabulary nor an added token")
    post_ids = spec["post_processor"]["special_tokens"]
    if post_ids[cls_tok]["ids"][0] != every[cls_tok] or post_ids[sep_tok]["ids"][0] != every[sep_tok]:
        raise ValueError(f"{path}: post_processor special token ids differ from the vocabulary's")
    space_ids = [-1] * (MAX_SPACE_RUN + 1)
    routed = []
    for tok in added:
        content = tok.get("content") or ""
        if not content:
            continue
        plain = not (tok.get("lstrip") or tok.get("rstrip") or tok.get("single_word"))
        if tok.get("normalized") and not tok.get("special"):
            if not plain:
                raise ValueError(f"{path}: added_tokens entry {content!r} is normalized with lstrip / rstrip / single_word set")
            if unicodedata.normalize("NFC", content) != content:
                raise ValueError(f"{path}: added_tokens entry {content!r} is normalized and changes under NFC")
            if 2 <= len(content) <= MAX_SPACE_RUN and content == " " * len(content):
                space_ids[len(content)] = int(tok["id"])      # cut on the device
                continue
        elif not plain and not tok.get("special"):
            raise ValueError(f"{path}: added_tokens entry {content!r} has lstrip / rstrip / single_word set without being special")
        routed.append(content)
    left, right, merged = [], [], []
    for r, m in enumerate(model.get("merges") or []):
        a, b = m.split(" ") if isinstance(m, str) else m
        if a not in vocab or b not in vocab or a + b not in vocab:
            raise ValueError(f"{path}: model merge {r} ({a!r}, {b!r}) names a token the vocabulary lacks")
        left.append(vocab[a])
        right.append(vocab[b])
        merged.append(vocab[a + b])
    ignore = bool(model.get("ignore_merges"))
    whole: List[Tuple[bytes, int]] = []
    if ignore:
        byte_of = {ch: b for b, ch in enumerate(alphabet)}
        for tok, i in vocab.items():
            if tok and len(tok) <= MAX_WORD_BYTES and all(ch in byte_of for ch in tok):
                whole.append((bytes(byte_of[ch] for ch in tok), i))
    return dict(n_vocab=len(every), cls_id=int(every[cls_tok]), sep_id=int(every[sep_tok]), nfc=norm is not None, ignore_merges=ignore,
                byte_ids=[int(vocab[ch]) for ch in alphabet], space_ids=space_ids, merges=(left, right, merged), whole=whole, routed=routed)


def _i32(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(values, np.int32).reshape(-1))


class GpuByteBpeTokenizer(DeviceTokenizer):
    """`encode_batch(texts)` -> packed int32 ids + lengths, equal to HF's; `encode_batch_offsets(texts)` adds HF's character
    offsets per id; `ids(text, ...)` as `TokenizerAdapter` offers it."""

    parse_spec = staticmethod(parse_spec)
    _destroy_entry, _encode_entry, _offsets_entry = "vrag_bpe_destroy", "vrag_bpe_encode", "vrag_bpe_encode_offsets"

    def __init__(self, spec: dict, hf_tokenizer: Any, device: int = 0, path: str = "tokenizer.json"):
        cfg = parse_spec(spec, path)
        super().__init__(hf_tokenizer, cfg["cls_id"], cfg["sep_id"], cfg["n_vocab"], device)
        self._routed = re.compile("|".join(re.escape(c) for c in cfg["routed"])) if cfg["routed"] else None
        left, right, merged = (_i32(x) for x in cfg["merges"])
        raw = [b for b, _i in cfg["whole"]]
        woff = np.zeros(len(raw) + 1, np.int64)
        np.cumsum([len(b) for b in raw], out=woff[1:])
        wblob = b"".join(raw)
        wid = _i32([i for _b, i in cfg["whole"]])
        ip = C.POINTER(C.c_int32)
        self._create("vrag_bpe_create", self.vocab_size, left.ctypes.data_as(ip), right.ctypes.data_as(ip), merged.ctypes.data_as(ip),
                     len(left), _i32(cfg["byte_ids"]).ctypes.data_as(ip), _i32(cfg["space_ids"]).ctypes.data_as(ip),
                     C.cast(C.c_char_p(wblob), C.c_void_p), woff.ctypes.data_as(C.POINTER(C.c_int64)), wid.ctypes.data_as(ip), len(raw),
                     self.cls_token_id, self.sep_token_id, (_NFC if cfg["nfc"] else 0) | (_IGNORE_MERGES if cfg["ignore_merges"] else 0))

    def _goes_to_host(self, texts) -> set:
        return {d for d, t in enumerate(texts) if self._routed.search(t)} if self._routed is not None else set()

    def encode_batch_offsets(self, texts: Sequence[str], add_special_tokens: bool = False,
                             max_length: int = 512) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids int32 [n], offsets int32 [n, 2], seq_lens int32 [n_docs]): `encode_batch` plus, per id, the half-open range of
        characters of its own text that HF reports as `Encoding.offsets` (include/vrag_amd.h states the rule; `(0, 0)` for
        [CLS] / [SEP]).  A flagged text takes ids AND offsets from the HF tokenizer."""
        return self._encode(texts, add_special_tokens, max_length, True)
