"""WordPiece tokenisation on the GPU (csrc/wordpiece.hip behind `vrag_wordpiece_*`): the ids HF `tokenizers` returns for the
BERT pipeline BertNormalizer -> BertPreTokenizer -> WordPiece -> `[CLS] $A [SEP]`, for a whole batch of texts in one call.

The device never guesses: a text with a code point the committed table does not cover comes back flagged and is tokenised
here with the HF tokenizer the object was built from, as is -- before the device call -- any text that holds the literal
content of an added token (`[SEP]`, `[MASK]`, ...: HF matches those ahead of the normaliser) or that is not encodable as UTF-8.
`fallback_count` counts the texts that went that way."""
from __future__ import annotations

import ctypes as C
from typing import Any

import numpy as np

from .device_tokenizer import DeviceTokenizer, _template_ids

TILE_BYTES = 4096   # VRAG_WORDPIECE_TILE_BYTES: text bytes per workgroup of the word-boundary passes
MAX_CHARS_PER_WORD = 128   # VRAG_WP_MAX_CHARS_PER_WORD
_LOWERCASE, _STRIP_ACCENTS, _CLEAN_TEXT, _CHINESE_CHARS = 1, 2, 4, 8


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


class GpuWordPieceTokenizer(DeviceTokenizer):
    """`encode_batch(texts)` -> packed int32 ids + lengths, equal to HF's; `ids(text, ...)` as `TokenizerAdapter` offers it."""

    parse_spec = staticmethod(parse_spec)
    _destroy_entry, _encode_entry = "vrag_wordpiece_destroy", "vrag_wordpiece_encode"

    def __init__(self, spec: dict, hf_tokenizer: Any, device: int = 0, path: str = "tokenizer.json"):
        cfg = parse_spec(spec, path)
        pieces = cfg["pieces"]
        super().__init__(hf_tokenizer, cfg["cls_id"], cfg["sep_id"], len(pieces), device)
        self._added = cfg["added"]
        self.unk_token_id = cfg["unk_id"]
        raw = [p.encode("utf-8") for p in pieces]
        off = np.zeros(len(raw) + 1, np.int64)
        np.cumsum([len(b) for b in raw], out=off[1:])
        blob = b"".join(raw)
        self._create("vrag_wordpiece_create", C.cast(C.c_char_p(blob), C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), len(raw),
                     self.unk_token_id, self.cls_token_id, self.sep_token_id, cfg["prefix"].encode("utf-8"), cfg["max_chars"], cfg["flags"])

    def _goes_to_host(self, texts) -> set:
        return {d for d, t in enumerate(texts) if any(a in t for a in self._added)}
