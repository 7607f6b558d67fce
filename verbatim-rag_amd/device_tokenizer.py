"""What the device tokenizers (wordpiece.py, bpe.py) share: loading from a `tokenizer.json`, the batch call -- texts the device
must not see go to the HF tokenizer before it runs, texts it flags go there afterwards, and either kind is spliced back between
the device's -- and the `ids` / `ids_batch` surface of `TokenizerAdapter`.  The device call itself is one method
(`_device_encode`), so everything around it runs without a GPU."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib


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


def read_spec(path_or_dir: str) -> Tuple[str, dict]:
    """(path, parsed json) of a `tokenizer.json`, or of the one in a checkpoint directory."""
    path = os.path.join(path_or_dir, "tokenizer.json") if os.path.isdir(path_or_dir) else path_or_dir
    with open(path, encoding="utf-8") as f:
        return path, json.load(f)


class DeviceTokenizer:
    """Base of `GpuWordPieceTokenizer` and `GpuByteBpeTokenizer`.  A subclass sets `parse_spec` (a staticmethod), the names of its
    C entries, uploads its tables in `__init__` (`_create`) and says which texts must not reach the device (`_goes_to_host`)."""

    parse_spec = None               # staticmethod (spec, path) -> dict, ValueError naming the component it refuses
    _destroy_entry = ""
    _encode_entry = ""
    _offsets_entry: Optional[str] = None

    def __init__(self, hf_tokenizer: Any, cls_id: int, sep_id: int, vocab_size: int, device: int = 0):
        self._hf = type(hf_tokenizer).from_str(hf_tokenizer.to_str())      # a copy: the caller's keeps its truncation / padding
        self._hf.no_truncation()
        self._hf.no_padding()
        self.cls_token_id, self.sep_token_id, self.vocab_size = cls_id, sep_id, vocab_size
        self.device = int(device)
        self.fallback_count = 0
        self._h = None

    def _create(self, entry: str, *args) -> None:
        """Calls the C create entry with `args`, the device and the handle slot."""
        self._lib = _lib.load()
        _lib.require_gpu()
        handle = C.c_void_p()
        _lib.check(entry, getattr(self._lib, entry)(*args, self.device, C.byref(handle)))
        self._h = handle

    @classmethod
    def from_file(cls, path_or_dir: str, device: int = 0):
        """From a `tokenizer.json` (or the checkpoint directory that holds it).  ValueError naming the component unless the
        file is exactly the pipeline the class's `parse_spec` accepts."""
        from tokenizers import Tokenizer

        path, spec = read_spec(path_or_dir)
        cls.parse_spec(spec, path)      # refuse a wrong file before anything touches the device
        return cls(spec, Tokenizer.from_file(path), device=device, path=path)

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy_entry)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _goes_to_host(self, texts: List[str]) -> set:
        """Positions of the texts HF must tokenise without the device seeing them: they hold an added token HF matches first.
        Over the batch rather than per text: one Python call per text is measurable against a device call of a few ms."""
        raise NotImplementedError

    def _host_encode(self, text: str, add_special_tokens: bool, max_length: int) -> Tuple[List[int], List[Tuple[int, int]]]:
        enc = self._hf.encode(text, add_special_tokens=False)
        keep = max_length - 2 if add_special_tokens else max_length
        ids, offsets = list(enc.ids)[:keep], list(enc.offsets)[:keep]
        if add_special_tokens:
            return [self.cls_token_id] + ids + [self.sep_token_id], [(0, 0)] + offsets + [(0, 0)]
        return ids, offsets

    def _device_encode(self, blob: bytes, off: np.ndarray, add_special_tokens: bool, max_length: int, cap: int, with_offsets: bool):
        """One C encode call over the texts `blob[off[d]:off[d + 1]]`, room for `cap` ids: (ids int32 [total], offsets int32
        [total, 2] or None, seq_lens int32 [n], needs_host uint8 [n])."""
        n = len(off) - 1
        seq_lens = np.empty(n, np.int32)
        needs = np.empty(n, np.uint8)
        n_ids = C.c_int64(0)
        ids = np.empty(max(cap, 1), np.int32)
        offsets = np.empty((max(cap, 1), 2), np.int32) if with_offsets else None
        ip = C.POINTER(C.c_int32)
        entry = self._offsets_entry if with_offsets else self._encode_entry
        _lib.check(entry, getattr(self._lib, entry)(
            self._h, C.cast(C.c_char_p(blob), C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), n, 1 if add_special_tokens else 0,
            max_length, cap, ids.ctypes.data_as(ip), *([offsets.ctypes.data_as(ip)] if with_offsets else []),
            seq_lens.ctypes.data_as(ip), needs.ctypes.data_as(C.c_void_p), C.byref(n_ids)))
        return ids[:n_ids.value], offsets[:n_ids.value] if with_offsets else None, seq_lens, needs

    def _encode(self, texts: Sequence[str], add_special_tokens: bool, max_length: int, with_offsets: bool):
        """(ids, offsets or None, seq_lens); an empty batch has offsets of shape (0, 2) on either route."""
        texts = list(texts)
        max_length = int(max_length)
        if max_length < (2 if add_special_tokens else 0):
            raise ValueError(f"max_length {max_length} leaves no room for the special tokens")
        n = len(texts)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
        if not self._h:
            raise RuntimeError(f"{type(self).__name__} is closed")
        raw: List[bytes] = []
        host = self._goes_to_host(texts)
        for d, t in enumerate(texts):
            b = b""
            if d not in host:
                try:
                    b = t.encode("utf-8")
                except UnicodeEncodeError:          # lone surrogates
                    host.add(d)
            raw.append(b)
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(b) for b in raw], out=off[1:])
        blob = b"".join(raw)
        cap = int(min(len(blob) + 2 * n, max_length * n))   # no text has more ids than bytes (+ 2 specials) or than max_length
        ids, offsets, seq_lens, needs = self._device_encode(blob, off, add_special_tokens, max_length, cap, with_offsets)
        host.update(np.nonzero(needs)[0].tolist())
        if not host:
            return ids, offsets, seq_lens
        self.fallback_count += len(host)
        return self._splice(texts, host, ids, offsets, seq_lens, add_special_tokens, max_length)

    def _splice(self, texts: List[str], host: set, ids: np.ndarray, offsets: Optional[np.ndarray], seq_lens: np.ndarray,
                add_special_tokens: bool, max_length: int):
        """The packed device batch with the texts of `host` replaced by what HF gives for them (`seq_lens` is updated in place)."""
        with_offsets = offsets is not None
        starts = np.zeros(len(texts) + 1, np.int64)
        np.cumsum(seq_lens, out=starts[1:])
        parts, oparts = [], []
        for d in range(len(texts)):
            if d in host:
                part, opart = self._host_encode(texts[d], add_special_tokens, max_length)
                seq_lens[d] = len(part)
            else:
                part, opart = ids[starts[d]:starts[d + 1]], offsets[starts[d]:starts[d + 1]] if with_offsets else None
            parts.append(np.asarray(part, np.int32))
            if with_offsets:
                oparts.append(np.asarray(opart, np.int32).reshape(-1, 2))
        return (np.concatenate(parts).astype(np.int32, copy=False),
                np.concatenate(oparts).astype(np.int32, copy=False) if with_offsets else None, seq_lens)

    def encode_batch(self, texts: Sequence[str], add_special_tokens: bool = True, max_length: int = 512) -> Tuple[np.ndarray, np.ndarray]:
        """(ids int32 [sum of lengths], seq_lens int32 [n]): the texts' ids back to back, as `vrag_encoder_load_batch` takes them."""
        ids, _offsets, seq_lens = self._encode(texts, add_special_tokens, max_length, False)
        return ids, seq_lens

    def ids_batch(self, texts: Sequence[str], max_length: int, add_special_tokens: bool = False) -> List[List[int]]:
        """As `TokenizerAdapter.ids_batch`: one list of ids per text, from one device batch."""
        ids, lens = self.encode_batch(texts, add_special_tokens=add_special_tokens, max_length=max_length)
        cuts = np.cumsum(lens)[:-1]
        return [part.tolist() for part in np.split(ids, cuts)] if len(lens) else []

    def ids(self, text: str, add_special_tokens: bool, max_length: int) -> List[int]:
        return self.encode_batch([text], add_special_tokens=add_special_tokens, max_length=max_length)[0].tolist()
