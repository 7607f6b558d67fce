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
import json
import os
import re
import unicodedata
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np

from . import _lib
from .wordpiece import _template_ids

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


class GpuByteBpeTokenizer:
    """`encode_batch(texts)` -> packed int32 ids + lengths, equal to HF's; `encode_batch_offsets(texts)` adds HF's character
    offsets per id; `ids(text, ...)` as `TokenizerAdapter` offers it."""

    def __init__(self, spec: dict, hf_tokenizer: Any, device: int = 0, path: str = "tokenizer.json"):
        cfg = parse_spec(spec, path)
        self._hf = type(hf_tokenizer).from_str(hf_tokenizer.to_str())      # a copy: the caller's keeps its truncation / padding
        self._hf.no_truncation()
        self._hf.no_padding()
        self._routed = re.compile("|".join(re.escape(c) for c in cfg["routed"])) if cfg["routed"] else None
        self.cls_token_id, self.sep_token_id = cfg["cls_id"], cfg["sep_id"]
        self.vocab_size = cfg["n_vocab"]
        self.device = int(device)
        self.fallback_count = 0
        left, right, merged = (_i32(x) for x in cfg["merges"])
        raw = [b for b, _i in cfg["whole"]]
        woff = np.zeros(len(raw) + 1, np.int64)
        np.cumsum([len(b) for b in raw], out=woff[1:])
        wblob = b"".join(raw)
        wid = _i32([i for _b, i in cfg["whole"]])
        ip = C.POINTER(C.c_int32)
        self._lib = _lib.load()
        _lib.require_gpu()
        handle = C.c_void_p()
        _lib.check("vrag_bpe_create", self._lib.vrag_bpe_create(
            self.vocab_size, left.ctypes.data_as(ip), right.ctypes.data_as(ip), merged.ctypes.data_as(ip), len(left),
            _i32(cfg["byte_ids"]).ctypes.data_as(ip), _i32(cfg["space_ids"]).ctypes.data_as(ip),
            C.cast(C.c_char_p(wblob), C.c_void_p), woff.ctypes.data_as(C.POINTER(C.c_int64)), wid.ctypes.data_as(ip), len(raw),
            self.cls_token_id, self.sep_token_id, (_NFC if cfg["nfc"] else 0) | (_IGNORE_MERGES if cfg["ignore_merges"] else 0),
            self.device, C.byref(handle)))
        self._h = handle

    @classmethod
    def from_file(cls, path_or_dir: str, device: int = 0) -> "GpuByteBpeTokenizer":
        """From a `tokenizer.json` (or the checkpoint directory that holds it).  ValueError naming the component unless the
        file is the byte-level BPE pipeline `parse_spec` accepts."""
        from tokenizers import Tokenizer

        path = os.path.join(path_or_dir, "tokenizer.json") if os.path.isdir(path_or_dir) else path_or_dir
        with open(path, encoding="utf-8") as f:
            spec = json.load(f)
        parse_spec(spec, path)      # refuse a wrong file before anything touches the device
        return cls(spec, Tokenizer.from_file(path), device=device, path=path)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vrag_bpe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode_batch(self, texts: Sequence[str], add_special_tokens: bool = True, max_length: int = 512) -> Tuple[np.ndarray, np.ndarray]:
        """(ids int32 [sum of lengths], seq_lens int32 [n]): the texts' ids back to back, as `vrag_encoder_load_batch` takes them."""
        ids, _offsets, seq_lens = self._encode(texts, add_special_tokens, max_length, False)
        return ids, seq_lens

    def encode_batch_offsets(self, texts: Sequence[str], add_special_tokens: bool = False,
                             max_length: int = 512) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(ids int32 [n], offsets int32 [n, 2], seq_lens int32 [n_docs]): `encode_batch` plus, per id, the half-open range of
        characters of its own text that HF reports as `Encoding.offsets` (include/vrag_amd.h states the rule; `(0, 0)` for
        [CLS] / [SEP]).  A flagged text takes ids AND offsets from the HF tokenizer."""
        return self._encode(texts, add_special_tokens, max_length, True)

    def _host_encode(self, text: str, add_special_tokens: bool, max_length: int) -> Tuple[List[int], List[Tuple[int, int]]]:
        enc = self._hf.encode(text, add_special_tokens=False)
        keep = max_length - 2 if add_special_tokens else max_length
        ids, offsets = list(enc.ids)[:keep], list(enc.offsets)[:keep]
        if add_special_tokens:
            return [self.cls_token_id] + ids + [self.sep_token_id], [(0, 0)] + offsets + [(0, 0)]
        return ids, offsets

    def _encode(self, texts: Sequence[str], add_special_tokens: bool, max_length: int, with_offsets: bool):
        texts = list(texts)
        max_length = int(max_length)
        if max_length < (2 if add_special_tokens else 0):
            raise ValueError(f"max_length {max_length} leaves no room for the special tokens")
        n = len(texts)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
        if not self._h:
            raise RuntimeError("GpuByteBpeTokenizer is closed")
        raw: List[bytes] = []
        host = set()
        for d, t in enumerate(texts):
            try:
                b = t.encode("utf-8")
            except UnicodeEncodeError:          # lone surrogates
                b = None
            if b is None or (self._routed is not None and self._routed.search(t)):
                host.add(d)
                b = b""
            raw.append(b)
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(b) for b in raw], out=off[1:])
        blob = b"".join(raw)
        seq_lens = np.empty(n, np.int32)
        needs = np.empty(n, np.uint8)
        n_ids = C.c_int64(0)
        cap = int(min(len(blob) + 2 * n, max_length * n))   # no text has more ids than bytes (+ 2 specials) or than max_length
        ids = np.empty(max(cap, 1), np.int32)
        ip = C.POINTER(C.c_int32)
        head = (self._h, C.cast(C.c_char_p(blob), C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), n, 1 if add_special_tokens else 0,
                max_length, cap, ids.ctypes.data_as(ip))
        tail = (seq_lens.ctypes.data_as(ip), needs.ctypes.data_as(C.c_void_p), C.byref(n_ids))
        if with_offsets:
            offsets = np.empty((max(cap, 1), 2), np.int32)
            _lib.check("vrag_bpe_encode_offsets", self._lib.vrag_bpe_encode_offsets(*head, offsets.ctypes.data_as(ip), *tail))
            offsets = offsets[:n_ids.value]
        else:
            offsets = None
            _lib.check("vrag_bpe_encode", self._lib.vrag_bpe_encode(*head, *tail))
        ids = ids[:n_ids.value]
        host.update(np.nonzero(needs)[0].tolist())
        if not host:
            return ids, offsets, seq_lens
        self.fallback_count += len(host)
        starts = np.zeros(n + 1, np.int64)
        np.cumsum(seq_lens, out=starts[1:])
        parts, oparts = [], []
        for d in range(n):
            if d in host:
                h_ids, h_off = self._host_encode(texts[d], add_special_tokens, max_length)
                part = np.asarray(h_ids, np.int32)
                seq_lens[d] = len(part)
                if with_offsets:
                    oparts.append(np.asarray(h_off, np.int32).reshape(-1, 2))
            else:
                part = ids[starts[d]:starts[d + 1]]
                if with_offsets:
                    oparts.append(offsets[starts[d]:starts[d + 1]])
            parts.append(part)
        return (np.concatenate(parts).astype(np.int32, copy=False),
                np.concatenate(oparts).astype(np.int32, copy=False) if with_offsets else None, seq_lens)

    def ids_batch(self, texts: Sequence[str], max_length: int, add_special_tokens: bool = False) -> List[List[int]]:
        """As `TokenizerAdapter.ids_batch`: one list of ids per text, from one device batch."""
        ids, lens = self.encode_batch(texts, add_special_tokens=add_special_tokens, max_length=max_length)
        cuts = np.cumsum(lens)[:-1]
        return [part.tolist() for part in np.split(ids, cuts)] if len(lens) else []

    def ids(self, text: str, add_special_tokens: bool, max_length: int) -> List[int]:
        return self.encode_batch([text], add_special_tokens=add_special_tokens, max_length=max_length)[0].tolist()
