"""WordPiece tokenisation on the GPU (csrc/wordpiece.hip behind `vrag_wordpiece_*`): the ids HF `tokenizers` returns for the
BERT pipeline BertNormalizer -> BertPreTokenizer -> WordPiece -> `[CLS] $A [SEP]`, for a whole batch of texts in one call.

The device never guesses: a text with a code point the committed table does not cover comes back flagged and is tokenised
here with the HF tokenizer the object was built from, as is -- before the device call -- any text that holds the literal
content of an added token (`[SEP]`, `[MASK]`, ...: HF matches those ahead of the normaliser) or that is not encodable as UTF-8.
`fallback_count` counts the texts that went that way."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Any, List, Sequence, Tuple

import numpy as np

from . import _lib

TILE_BYTES = 4096   # VRAG_WORDPIECE_TILE_BYTES: text bytes per workgroup of the word-boundary passes
MAX_CHARS_PER_WORD = 128   # VRAG_WP_MAX_CHARS_PER_WORD
_LOWERCASE, _STRIP_ACCENTS, _CLEAN_TEXT, _CHINESE_CHARS = 1, 2, 4, 8


def _template_ids(post: Any, path: str) -> Tuple[str, str]:
    """([CLS] token, [SEP] token) of a `[CLS] $A [SEP]` TemplateProcessing; ValueError otherwise."""
    if not isinstance(post, dict) or post.get("type") != "TemplateProcessing":
        raise ValueError(f"{path}: post_processor must be TemplateProcessing, got {post.get('type') if isinstance(post, dict) else post!r}")
    single = post.get("single") or []
    kinds = [next(iter(x)) for x in single]
    if kinds != ["SpecialToken", "Sequence", "SpecialToken"] or single[1]["Sequence"].get("id") != "A":
        raise ValueError(f"{path}: post_processor template must be `<cls> $A <sep>`, got {single!r}")
    names = (single[0]["SpecialToken"]["id"], single[2]["SpecialToken"]["id"])
    for name in names:
        ids = (post.get("special_tokens") or {}).get(name, {}).get("ids")
        if not isinstance(ids, list) or len(ids) != 1:
            raise ValueError(f"{path}: post_processor special token {name!r} must stand for exactly one id")
    return names


def parse_spec(spec: dict, path: str = "tokenizer.json") -> dict:
    """Everything the device tokenizer needs from a parsed `tokenizer.json`, or ValueError naming the component that is not
    WordPiece / BertNormalizer / BertPreTokenizer / `[CLS] $A [SEP]` TemplateProcessing.  Needs no device."""
    model = spec.get("model") or {}
    if model.get("type") != "WordPiece":
        raise ValueError(f"{path}: model must be WordPiece, got {model.get('type')!r}")
    norm = spec.get("normalizer") or {}
    if norm.get("type") != "BertNormalizer":
        raise ValueError(f"{path}: normalizer must be BertNormalizer, got {norm.get('type')!r}")
    pre = spec.get("pre_tokenizer") or {}
    if pre.get("type") != "BertPreTokenizer":
        raise ValueError(f"{path}: pre_tokenizer must be BertPreTokenizer, got {pre.get('type')!r}")
    cls_tok, sep_tok = _template_ids(spec.get("post_processor"), path)
    vocab = model["vocab"]
    pieces = sorted(vocab, key=vocab.get)
    if [vocab[p] for p in pieces] != list(range(len(pieces))):
        raise ValueError(f"{path}: model vocabulary ids must be 0 .. n-1 without gaps")
    unk = model.get("unk_token", "[UNK]")
    for name in (unk, cls_tok, sep_tok):
        if name not in vocab:
            raise ValueError(f"{path}: model vocabulary lacks {name!r}")
    post_ids = spec["post_processor"]["special_tokens"]
    if post_ids[cls_tok]["ids"][0] != vocab[cls_tok] or post_ids[sep_tok]["ids"][0] != vocab[sep_tok]:
        raise ValueError(f"{path}: post_processor special token ids differ from the model vocabulary's")
    max_chars = int(model.get("max_input_chars_per_word", 100))
    if not 1 <= max_chars <= MAX_CHARS_PER_WORD:
        raise ValueError(f"{path}: model max_input_chars_per_word {max_chars} is outside 1..{MAX_CHARS_PER_WORD}")
    prefix = model.get("continuing_subword_prefix", "##")
    if len(prefix.encode("utf-8")) > 16:
        raise ValueError(f"{path}: model continuing_subword_prefix {prefix!r} is longer than 16 bytes")
    lowercase = bool(norm.get("lowercase", True))
    strip = norm.get("strip_accents")
    strip = lowercase if strip is None else bool(strip)      # HF: strip_accents = null follows lowercase
    flags = (_LOWERCASE if lowercase else 0) | (_STRIP_ACCENTS if strip else 0)
    flags |= _CLEAN_TEXT if norm.get("clean_text", True) else 0
    flags |= _CHINESE_CHARS if norm.get("handle_chinese_chars", True) else 0
    for tok in spec.get("added_tokens") or []:
        # HF matches a normalized=true added token against the NORMALISED text ("Foo" hits an added "foo"): routing texts by
        # their raw content would miss that, so such a file is refused rather than risk a wrong id
        if tok.get("normalized"):
            raise ValueError(f"{path}: added_tokens entry {tok.get('content')!r} has normalized=true (only normalized=false is supported)")
    return dict(pieces=pieces, unk_id=int(vocab[unk]), cls_id=int(vocab[cls_tok]), sep_id=int(vocab[sep_tok]), prefix=prefix,
                max_chars=max_chars, flags=flags, added=[t["content"] for t in spec.get("added_tokens") or [] if t.get("content")])


class GpuWordPieceTokenizer:
    """`encode_batch(texts)` -> packed int32 ids + lengths, equal to HF's; `ids(text, ...)` as `TokenizerAdapter` offers it."""

    def __init__(self, spec: dict, hf_tokenizer: Any, device: int = 0, path: str = "tokenizer.json"):
        cfg = parse_spec(spec, path)
        self._hf = type(hf_tokenizer).from_str(hf_tokenizer.to_str())      # a copy: the caller's keeps its truncation / padding
        self._hf.no_truncation()
        self._hf.no_padding()
        self._added = cfg["added"]
        self.cls_token_id, self.sep_token_id, self.unk_token_id = cfg["cls_id"], cfg["sep_id"], cfg["unk_id"]
        pieces = cfg["pieces"]
        self.vocab_size = len(pieces)
        self.device = int(device)
        self.fallback_count = 0
        raw = [p.encode("utf-8") for p in pieces]
        off = np.zeros(len(raw) + 1, np.int64)
        np.cumsum([len(b) for b in raw], out=off[1:])
        blob = b"".join(raw)
        self._lib = _lib.load()
        _lib.require_gpu()
        handle = C.c_void_p()
        _lib.check("vrag_wordpiece_create", self._lib.vrag_wordpiece_create(
            C.cast(C.c_char_p(blob), C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), len(raw), self.unk_token_id,
            self.cls_token_id, self.sep_token_id, cfg["prefix"].encode("utf-8"), cfg["max_chars"], cfg["flags"],
            self.device, C.byref(handle)))
        self._h = handle

    @classmethod
    def from_file(cls, path_or_dir: str, device: int = 0) -> "GpuWordPieceTokenizer":
        """From a `tokenizer.json` (or the checkpoint directory that holds it).  ValueError naming the component unless the
        file is exactly WordPiece / BertNormalizer / BertPreTokenizer / `[CLS] $A [SEP]` TemplateProcessing."""
        from tokenizers import Tokenizer

        path = os.path.join(path_or_dir, "tokenizer.json") if os.path.isdir(path_or_dir) else path_or_dir
        with open(path, encoding="utf-8") as f:
            spec = json.load(f)
        parse_spec(spec, path)      # refuse a wrong file before anything touches the device
        return cls(spec, Tokenizer.from_file(path), device=device, path=path)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vrag_wordpiece_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _host_ids(self, text: str, add_special_tokens: bool, max_length: int) -> List[int]:
        body = list(self._hf.encode(text, add_special_tokens=False).ids)
        if not add_special_tokens:
            return body[:max_length]
        return [self.cls_token_id] + body[:max_length - 2] + [self.sep_token_id]

    def encode_batch(self, texts: Sequence[str], add_special_tokens: bool = True, max_length: int = 512) -> Tuple[np.ndarray, np.ndarray]:
        """(ids int32 [sum of lengths], seq_lens int32 [n]): the texts' ids back to back, as `vrag_encoder_load_batch` takes them."""
        texts = list(texts)
        max_length = int(max_length)
        if max_length < (2 if add_special_tokens else 0):
            raise ValueError(f"max_length {max_length} leaves no room for the special tokens")
        n = len(texts)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        if not self._h:
            raise RuntimeError("GpuWordPieceTokenizer is closed")
        raw: List[bytes] = []
        host = set()
        for d, t in enumerate(texts):
            try:
                b = t.encode("utf-8")
            except UnicodeEncodeError:          # lone surrogates
                b = None
            if b is None or any(a in t for a in self._added):
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
        _lib.check("vrag_wordpiece_encode", self._lib.vrag_wordpiece_encode(
            self._h, C.cast(C.c_char_p(blob), C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), n, 1 if add_special_tokens else 0,
            max_length, cap, ids.ctypes.data_as(C.POINTER(C.c_int32)), seq_lens.ctypes.data_as(C.POINTER(C.c_int32)),
            needs.ctypes.data_as(C.c_void_p), C.byref(n_ids)))
        ids = ids[:n_ids.value]
        host.update(np.nonzero(needs)[0].tolist())
        if not host:
            return ids, seq_lens
        self.fallback_count += len(host)
        starts = np.zeros(n + 1, np.int64)
        np.cumsum(seq_lens, out=starts[1:])
        parts = []
        for d in range(n):
            if d in host:
                part = np.asarray(self._host_ids(texts[d], add_special_tokens, max_length), np.int32)
                seq_lens[d] = len(part)
            else:
                part = ids[starts[d]:starts[d + 1]]
            parts.append(part)
        return np.concatenate(parts).astype(np.int32, copy=False), seq_lens

    def ids_batch(self, texts: Sequence[str], max_length: int, add_special_tokens: bool = False) -> List[List[int]]:
        """As `TokenizerAdapter.ids_batch`: one list of ids per text, from one device batch."""
        ids, lens = self.encode_batch(texts, add_special_tokens=add_special_tokens, max_length=max_length)
        cuts = np.cumsum(lens)[:-1]
        return [part.tolist() for part in np.split(ids, cuts)] if len(lens) else []

    def ids(self, text: str, add_special_tokens: bool, max_length: int) -> List[int]:
        return self.encode_batch([text], add_special_tokens=add_special_tokens, max_length=max_length)[0].tolist()
