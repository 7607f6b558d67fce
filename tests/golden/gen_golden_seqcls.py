#!/usr/bin/env python3
"""Generates tests/golden/modernbert_seqcls_tiny.npz: a tiny random-init `ModernBertForSequenceClassification`
(transformers, fp32, eager attention; head_dim 64, the golden tokenizer's vocabulary) with two heads on ONE encoder --
classifier_pooling "cls" with classifier_bias, 1 label (the cross-encoder form), and "mean" without it, 2 labels -- plus
packed `[CLS] q [SEP] d [SEP]` pair ids and the model's fp32 logits for both.  Run where torch + transformers are installed;
the fixture is data only (weights, ids, outputs).  Every weight is rounded to a bf16-representable fp32 value BEFORE the
forward and stored as its bf16 bit pattern: lossless, and half the bytes (the file stays well under 1 MB)."""
import os
import sys

import numpy as np
import torch
from tokenizers import Tokenizer
from transformers import ModernBertConfig, ModernBertForSequenceClassification

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from verbatim_rag_amd.rerankers import pack_pair  # noqa: E402

WORDS = ("the quick brown fox jumps over lazy dog tower paris iron built year tall meters visitors river city bridge stone "
         "engineer opened museum garden light night climb stairs lift wind steel design world fair").split()


def bf16_round_(model, seed):
    """Random weights, LayerNorm gains jittered around 1 and non-zero biases (a dropped one shows), rounded to bf16 values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif p.dim() == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:   # initializer_range (ModernBertConfig default 0.02)
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            p.copy_(p.to(torch.bfloat16).to(torch.float32))
    return model


def bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).copy()


def main():
    tok = Tokenizer.from_file(os.path.join(HERE, "tokenizer.json"))
    V = tok.get_vocab_size()
    H, L, NH, I, P = 128, 3, 2, 128, 8192
    pad, cls_id, sep_id = tok.token_to_id("[PAD]"), tok.token_to_id("[CLS]"), tok.token_to_id("[SEP]")
    base = dict(vocab_size=V, hidden_size=H, num_hidden_layers=L, num_attention_heads=NH, intermediate_size=I,
                max_position_embeddings=P, pad_token_id=pad, cls_token_id=cls_id, sep_token_id=sep_id, bos_token_id=cls_id,
                eos_token_id=sep_id, attention_dropout=0.0, embedding_dropout=0.0, mlp_dropout=0.0, classifier_dropout=0.0,
                attn_implementation="eager")
    rng = np.random.default_rng(17)

    def text(n):
        return " ".join(WORDS[int(i)] for i in rng.integers(0, len(WORDS), size=n))

    pairs = []
    for nq, nd, max_len in [(4, 12, 128), (7, 40, 128), (3, 90, 128), (10, 25, 128), (6, 200, 160), (2, 3, 128)]:
        q = tok.encode(text(nq), add_special_tokens=False).ids
        d = tok.encode(text(nd), add_special_tokens=False).ids
        pairs.append(pack_pair(q, d, cls_id, sep_id, max_len)[0])

    out = {"cfg": np.asarray([V, H, L, NH, I, P], np.int32), "special_ids": np.asarray([pad, cls_id, sep_id], np.int32),
           "n_pairs": np.asarray(len(pairs), np.int32)}
    for i, ids in enumerate(pairs):
        out[f"ids{i}"] = np.asarray(ids, np.int32)
    enc_sd = None
    for name, bias, labels, seed in (("cls", True, 1, 21), ("mean", False, 2, 22)):
        torch.manual_seed(seed)
        m = ModernBertForSequenceClassification(ModernBertConfig(classifier_pooling=name, classifier_bias=bias, num_labels=labels,
                                                                 **base))
        bf16_round_(m, 5 if enc_sd is None else seed)
        if enc_sd is None:
            enc_sd = {k: v.clone() for k, v in m.model.state_dict().items()}
        else:   # both heads sit on the same encoder
            m.model.load_state_dict(enc_sd)
        m.eval()
        with torch.no_grad():
            logits = [m(input_ids=torch.tensor([ids])).logits[0].numpy() for ids in pairs]
        out[f"logits:{name}"] = np.stack(logits).astype(np.float32)
        for k, v in m.state_dict().items():
            if not k.startswith("model."):
                out[f"head:{name}:{k}"] = bits(v)
    for k, v in enc_sd.items():
        out[f"enc:{k}"] = bits(v)
    path = os.path.join(HERE, "modernbert_seqcls_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
