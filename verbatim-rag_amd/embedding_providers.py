"""GPU embedding providers behind the reference's provider interfaces.

Kept: `DenseEmbeddingProvider` / `SparseEmbeddingProvider` ABCs and the exact return shapes
(verbatim_rag/embedding_providers.py:14-49): sparse `embed_text -> Dict[int,float]` keeping
|w| > 1e-6 (:138-146), `embed_batch -> List[Dict]` keeping exact non-zeros (:148-166), dense
`List[float]` rows (:73-77).  Replaced: sentence-transformers `SparseEncoder.encode` /
`SentenceTransformer.encode` (third-party, absent here) by the HIP encoder + fused SPLADE head
`max_s log1p(relu(mlm_logits))` / CLS-or-mean pooling + L2 normalise.  `engine` is an
`EncoderEngine` (ModernBERT backbone) or a `BertEncoderEngine` (BERT / DistilBERT: the checkpoints the
reference names -- `naver/splade-v3`, `opensearch-neural-sparse-encoding-doc-v2-distill`, bge-base;
embedding_providers.py:55,120; head_dim 64, or 32 as in the default dense model all-MiniLM-L6-v2).
"""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ._lib import VragError
from .checked_engine import CheckedEngines, greedy_batches
from .packing import TokenizerAdapter, load_tokenizer


class DenseEmbeddingProvider(ABC):
    @abstractmethod
    def embed_text(self, text: str) -> List[float]:
        pass

    @abstractmethod
    def embed_batch(self, texts: List[str]) -> List[List[float]]:
        pass

    @abstractmethod
    def get_dimension(self) -> int:
        pass


class SparseEmbeddingProvider(ABC):
    @abstractmethod
    def embed_text(self, text: str) -> Dict[int, float]:
        pass

    @abstractmethod
    def embed_batch(self, texts: List[str]) -> List[Dict[int, float]]:
        pass

    @abstractmethod
    def get_dimension(self) -> int:
        pass


class _EncoderProvider:
    """`from_directory` builds the engine with **fp16 MFMA operands** (11 significant bits at the bf16 rate): embeddings feed an
    index whose top-k is held to bit-exactness, and nothing averages operand rounding away under SPLADE's max-pool -- measured end
    to end against the fp32 oracle, BERT-base width: SPLADE weights 1.6e-3 (fp16) vs 1.3e-2 (bf16), dense rows 6e-5 (fp16)
    (tests/test_splade_real_vocab_gpu.py, tests/test_e2e_text_in_gpu.py).  fp16 saturates at 65504 instead of overflowing: the
    library reports every clamp, and on the first report the provider rebuilds its engine with bf16 operands (fp32's exponent
    range) and runs the batch again -- `operand_dtype="bf16"` skips the probe; a provider that was HANDED its engine raises
    (the rule lives in checked_engine.py: every device batch goes through `self._checked.run`)."""

    def __init__(self, engine: Any, tokenizer: Any, max_length: int = 512):
        self.tokenizer = tokenizer
        self._max_length = max_length
        self._checked = CheckedEngines([engine], on_swap=self._bind)    # from_directory adds the bf16 rebuild
        self._bind()

    def _bind(self) -> None:
        """What the provider keeps of its engine; derived again when the engine is replaced."""
        self.engine = self._checked.engines[0]
        self.max_length = min(self._max_length, self.engine.max_seq_len)
        self._tok = TokenizerAdapter.for_model(self.tokenizer, self.engine.shape)

    def _encode(self, texts: Sequence[str]) -> List[List[int]]:
        return self._tok.ids_batch(list(texts), max_length=self.max_length, add_special_tokens=True)

    def _batches(self, seqs: List[List[int]]):
        eng = self.engine
        for a, b in greedy_batches([len(s) for s in seqs], eng.max_seqs, eng.max_tokens, eng.max_ranges):
            if a == b:
                raise ValueError("a single text exceeds the engine workspace")
            yield a, b


def load_model_tokenizer(model_path: str, tokenizer: str = "host", device: int = 0) -> Any:
    """The tokenizer of a checkpoint directory: "host" = `load_tokenizer` (HF, on the caller's thread), "gpu" = a device
    tokenizer over the directory's tokenizer.json: `GpuByteBpeTokenizer` for a BPE model behind a ByteLevel pre-tokenizer
    (ModernBERT checkpoints), `GpuWordPieceTokenizer` for every other file (ValueError naming the component for anything but
    the BERT WordPiece pipeline).  The dispatch only looks at `model.type` and `pre_tokenizer.type`; the class it picks reads and
    validates the file itself, so a missing or malformed tokenizer.json is reported from here."""
    if tokenizer == "host":
        return load_tokenizer(model_path)
    if tokenizer != "gpu":
        raise ValueError(f"tokenizer must be 'host' or 'gpu', got {tokenizer!r}")
    from .device_tokenizer import read_spec

    path, spec = read_spec(model_path)
    if (spec.get("model") or {}).get("type") == "BPE" and (spec.get("pre_tokenizer") or {}).get("type") == "ByteLevel":
        from .bpe import GpuByteBpeTokenizer as cls
    else:
        from .wordpiece import GpuWordPieceTokenizer as cls
    return cls.from_file(path, device=device)


def load_encoder_directory(model_path: str, device: int = 0, max_tokens: int = 65536, max_seqs: int = 512,
                           max_seq_len: int = 512, splade_split_operands: bool = True, operand_dtype: str = "f16",
                           tokenizer: str = "host", **engine_kw):
    """(engine, tokenizer, raw config) from a local HF checkpoint directory -- the local-files counterpart of the model
    names the reference hands to sentence-transformers (`SpladeProvider(model_name)`, embedding_providers.py:117-133;
    `SentenceTransformersProvider(model_name)`, :52-71).  BERT / DistilBERT checkpoints get a `BertEncoderEngine` (MLM
    and pair heads attached when the tensors are there), ModernBERT checkpoints an `EncoderEngine` (+ MLM head, or the sequence-classification
    head when `architectures` names ModernBertForSequenceClassification).
    `tokenizer`: "host" or "gpu" (`load_model_tokenizer`; a wrong request is refused before the weights are read).
    `splade_split_operands=False`: the MLM / SPLADE head with plain 16-bit operands (a third of the decoder work, weights within
    ~1e-2 of the fp32 head instead of 2e-5; include/vrag_amd.h vrag_encoder_set_head_precision)."""
    import json
    import os

    from . import engine as engine_mod
    from .weights import load_bert_safetensors_dir, load_safetensors_dir

    tok = load_model_tokenizer(model_path, tokenizer, device)
    try:
        with open(os.path.join(model_path, "config.json")) as f:
            raw_cfg = json.load(f)
        model_type = raw_cfg.get("model_type")
        kw = dict(max_tokens=max_tokens, max_seqs=max_seqs, max_seq_len=max_seq_len, max_ranges=max(max_seqs, 64), device=device,
                  operand_dtype=operand_dtype, **engine_kw)
        if model_type in ("bert", "distilbert"):
            shape, weights, cfg = load_bert_safetensors_dir(model_path)
            eng = engine_mod.BertEncoderEngine(shape, weights, mlm_split_operands=splade_split_operands, **kw)
        elif model_type == "modernbert":
            seq_head = _modernbert_seq_head(model_path, raw_cfg)
            shape, tensors, cfg = load_safetensors_dir(model_path)
            eng = engine_mod.EncoderEngine(shape, tensors, **kw)
            if "head.dense.weight" in tensors and "decoder.bias" in tensors:        # ModernBertForMaskedLM: tied decoder
                eng.set_mlm_head(tensors["head.dense.weight"], tensors["head.norm.weight"], tensors["decoder.bias"],
                                 tensors.get("decoder.weight"), split_operands=splade_split_operands)
            if seq_head is not None:
                eng.set_seq_head(tensors["head.dense.weight"], tensors["head.dense.bias"] if seq_head["dense_bias"] else None,
                                 tensors["head.norm.weight"], None, tensors["classifier.weight"], tensors["classifier.bias"],
                                 pooling=seq_head["pooling"])
        else:
            raise ValueError(f"{model_path}: model_type {model_type!r} is not bert / distilbert / modernbert")
    except BaseException:
        if hasattr(tok, "close"):      # the device tokenizer holds a GPU handle
            tok.close()
        raise
    return eng, tok, cfg


def load_checked_directory(model_path: str, **load_kw):
    """(engine, tokenizer, rebuild) for a wrapper's `from_directory`: `load_encoder_directory` plus the `rebuild` that
    `CheckedEngines` takes -- the same checkpoint with bf16 operands, or None when the engine has no fp16 operands to clamp."""
    engine, tokenizer, _cfg = load_encoder_directory(model_path, **load_kw)
    if getattr(engine, "operand_dtype", "bf16") != "f16":
        return engine, tokenizer, None
    return engine, tokenizer, lambda: load_encoder_directory(model_path, **{**load_kw, "operand_dtype": "bf16", "tokenizer": "host"})[0]


def _modernbert_seq_head(model_path: str, cfg: dict) -> Optional[dict]:
    """The sequence-classification head a ModernBERT checkpoint carries, decided by `architectures` (never by tensor names:
    ModernBertForTokenClassification uses the same `head.*` / `classifier.*` names) -> {"pooling", "dense_bias"} or None.
    What the engine cannot compute is refused here, naming the config key (transformers ModernBertConfig)."""
    if "ModernBertForSequenceClassification" not in (cfg.get("architectures") or []):
        return None
    if cfg.get("norm_bias", False):
        raise ValueError(f"{model_path}: config.json norm_bias: true is not supported (the encoder's LayerNorms take no bias)")
    act = cfg.get("classifier_activation", "gelu")
    if act != "gelu":
        raise ValueError(f"{model_path}: config.json classifier_activation {act!r} is not supported (only 'gelu')")
    pooling = cfg.get("classifier_pooling", "cls")
    if pooling not in ("cls", "mean"):
        raise ValueError(f"{model_path}: config.json classifier_pooling {pooling!r} is not supported (only 'cls' / 'mean')")
    return {"pooling": pooling, "dense_bias": bool(cfg.get("classifier_bias", False))}


def _st_pooling_mode(model_path: str, default: str = "cls") -> str:
    """sentence-transformers checkpoints say how they pool in `1_Pooling/config.json` (bge: CLS, MiniLM: mean)."""
    import json
    import os

    try:
        with open(os.path.join(model_path, "1_Pooling", "config.json")) as f:
            pc = json.load(f)
    except OSError:
        return default
    if pc.get("pooling_mode_mean_tokens"):
        return "mean"
    if pc.get("pooling_mode_cls_token"):
        return "cls"
    raise ValueError(f"{model_path}: only CLS and mean pooling are implemented (1_Pooling/config.json: {pc})")


class GpuSpladeProvider(_EncoderProvider, SparseEmbeddingProvider):
    """SpladeProvider (embedding_providers.py:117-169) on the HIP encoder + fused SPLADE head."""

    def __init__(self, engine: Any, tokenizer: Any, max_length: int = 512, sparse_cap: int = 1024):
        super().__init__(engine, tokenizer, max_length)
        self.sparse_cap = int(sparse_cap)
        if not engine.has_mlm:
            raise ValueError("engine has no MLM head (EncoderEngine.set_mlm_head)")

    @classmethod
    def from_directory(cls, model_path: str, device: int = 0, max_length: int = 512, operand_dtype: str = "f16",
                       tokenizer: str = "host", **kw) -> "GpuSpladeProvider":
        """`SpladeProvider(model_name, device)` (embedding_providers.py:120-133) for a checkpoint on disk.  `tokenizer="gpu"`:
        WordPiece (wordpiece.py) or, for a ModernBERT checkpoint, byte-level BPE (bpe.py) on the device, same ids."""
        engine, tokenizer, rebuild = load_checked_directory(model_path, device=device, max_seq_len=max_length, operand_dtype=operand_dtype,
                                                            tokenizer=tokenizer)
        self = cls(engine, tokenizer, max_length=max_length, **kw)
        self._checked.rebuild = rebuild
        return self

    def _rows(self, texts: Sequence[str]) -> np.ndarray:
        seqs = self._encode(texts)
        out = np.empty((len(seqs), self.engine.shape.vocab_size), np.float32)

        def rows(engine, a, b):
            engine.load_batch(seqs[a:b])
            engine.run()
            engine.run_splade()
            return engine.read_splade()

        for a, b in self._batches(seqs):
            out[a:b] = self._checked.run(lambda engine: rows(engine, a, b))
        return out

    def _dicts(self, texts: Sequence[str], threshold: float) -> List[Dict[int, float]]:
        """Rows compacted on the GPU (vocabulary order = np.nonzero order); a row with more than `sparse_cap`
        entries (e.g. an untrained model) falls back to the dense read for that batch."""
        seqs = self._encode(texts)
        out: List[Dict[int, float]] = []

        def dicts(engine, a, b):
            engine.load_batch(seqs[a:b])
            engine.run()
            engine.run_splade()
            part: List[Dict[int, float]] = []
            try:
                counts, idx, val = engine.read_splade_sparse(threshold, self.sparse_cap)
                for i in range(b - a):
                    n = int(counts[i])
                    part.append(dict(zip(idx[i, :n].tolist(), val[i, :n].tolist())))
            except VragError as exc:
                if exc.status != -3:   # VRAG_ERR_CAPACITY
                    raise
                rows = engine.read_splade()
                for row in rows:
                    nz = np.nonzero(row > threshold)[0]
                    part.append({int(i): float(row[i]) for i in nz})
            return part

        for a, b in self._batches(seqs):
            out.extend(self._checked.run(lambda engine: dicts(engine, a, b)))
        return out

    def embed_text(self, text: str) -> Dict[int, float]:
        return self._dicts([text], 1e-6)[0]                # |w| > 1e-6, embedding_providers.py:141-145 (w >= 0)

    def embed_batch(self, texts: List[str]) -> List[Dict[int, float]]:
        return self._dicts(texts, 0.0)                     # every non-zero, embedding_providers.py:161-163

    def embed_queries(self, texts: List[str]) -> List[Dict[int, float]]:
        """`[embed_text(t) for t in texts]` (the |w| > 1e-6 rule) as shared device batches -- the query side of a
        cross-query batch; `embed_batch` is the ingest side and keeps every non-zero."""
        return self._dicts(texts, 1e-6)

    def get_dimension(self) -> int:
        return int(self.engine.shape.vocab_size)


class GpuDenseProvider(_EncoderProvider, DenseEmbeddingProvider):
    """SentenceTransformersProvider (embedding_providers.py:52-80): pooling `cls` | `mean`, L2 normalise."""

    def __init__(self, engine: Any, tokenizer: Any, pooling: str = "cls", normalize: bool = True, max_length: int = 512):
        super().__init__(engine, tokenizer, max_length)
        if pooling not in ("cls", "mean"):
            raise ValueError("pooling must be 'cls' or 'mean'")
        self.pooling, self.normalize = pooling, normalize

    @classmethod
    def from_directory(cls, model_path: str, device: int = 0, max_length: int = 512, pooling: Optional[str] = None,
                       normalize: bool = True, operand_dtype: str = "f16", tokenizer: str = "host") -> "GpuDenseProvider":
        """`SentenceTransformersProvider(model_name, device)` (embedding_providers.py:55-71) for a checkpoint on disk;
        the pooling mode comes from the checkpoint's `1_Pooling/config.json` unless given.  `tokenizer="gpu"`: WordPiece or
        byte-level BPE on the device (wordpiece.py, bpe.py), same ids."""
        engine, tokenizer, rebuild = load_checked_directory(model_path, device=device, max_seq_len=max_length, operand_dtype=operand_dtype,
                                                            tokenizer=tokenizer)
        self = cls(engine, tokenizer, pooling=pooling or _st_pooling_mode(model_path), normalize=normalize, max_length=max_length)
        self._checked.rebuild = rebuild
        return self

    def _rows(self, texts: Sequence[str]) -> np.ndarray:
        seqs = self._encode(texts)
        out = np.empty((len(seqs), self.engine.shape.hidden_size), np.float32)

        def rows(engine, a, b):
            engine.load_batch(seqs[a:b])
            n = b - a
            ends = [0] * n if self.pooling == "cls" else [len(s) - 1 for s in seqs[a:b]]
            engine.load_ranges(list(range(n)), [0] * n, ends)
            engine.run()
            engine.run_pool(self.normalize)
            return engine.read_pool()

        for a, b in self._batches(seqs):
            out[a:b] = self._checked.run(lambda engine: rows(engine, a, b))
        return out

    def embed_text(self, text: str) -> List[float]:
        return self._rows([text])[0].tolist()

    def embed_batch(self, texts: List[str]) -> List[List[float]]:
        return self._rows(texts).tolist()

    def embed_queries(self, texts: List[str]) -> List[List[float]]:
        """`[embed_text(t) for t in texts]` as shared device batches (rows do not depend on their batch mates)."""
        return self._rows(texts).tolist()

    def get_dimension(self) -> int:
        return int(self.engine.shape.hidden_size)
