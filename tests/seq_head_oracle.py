"""numpy restatement of the ModernBertForSequenceClassification head (transformers models/modernbert/modeling_modernbert.py:
ModernBertPredictionHead + classifier) on top of `oracle/modernbert_np`, and the loader of the tiny golden fixture
`tests/golden/modernbert_seqcls_tiny.npz` (tests/golden/gen_golden_seqcls.py).

    p      = h[0]                      classifier_pooling "cls"
           = mean of h over the tokens "mean" (every real token of the pair, [CLS] and [SEP]s included)
    y      = LayerNorm(gelu_erf(Wd . p + bd); wn, bn)
    logits = Wc . y + bc
where h is the final-normed hidden state of one unpadded sequence."""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

import numpy as np

from oracle import modernbert_np as O

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modernbert_seqcls_tiny.npz")


def pool(hidden: np.ndarray, pooling: str) -> np.ndarray:
    if pooling == "cls":
        return hidden[0].astype(F32)
    if pooling == "mean":
        return hidden.astype(F32).mean(axis=0, dtype=F32)
    raise ValueError(pooling)


def head_logits(hidden: np.ndarray, head: Dict[str, Optional[np.ndarray]], pooling: str, eps: float) -> np.ndarray:
    """[labels] logits of one sequence from its final-normed hidden state [S, H]."""
    p = pool(hidden, pooling)
    x = p @ head["dense_w"].astype(F32).T
    if head.get("dense_b") is not None:
        x = x + head["dense_b"].astype(F32)
    y = O.layer_norm(O.gelu_erf(x.astype(F32)), head["norm_w"], eps)
    if head.get("norm_b") is not None:
        y = y + head["norm_b"].astype(F32)
    return (y @ head["cls_w"].astype(F32).T + head["cls_b"].astype(F32)).astype(F32)


def pair_logits(cfg: "O.EncoderConfig", w: Dict[str, np.ndarray], ids: Sequence[int], head, pooling: str) -> np.ndarray:
    return head_logits(O.encoder_forward(cfg, w, ids), head, pooling, cfg.norm_eps)


# ------------------------------------------------------------------------------------------------ golden fixture
def _bf16_to_f32(u16: np.ndarray) -> np.ndarray:
    return (u16.astype(np.uint32) << 16).view(np.float32)


def load_golden(path: str = GOLDEN) -> dict:
    """{"cfg": EncoderConfig, "hf_cfg": dict of ModernBertConfig keys, "encoder": bare-named encoder weights,
    "models": {"cls"|"mean": {"pooling", "classifier_bias", "head", "state_dict", "logits"}}, "ids": [pair ids]}.
    Weights are stored as the bf16 bit patterns of bf16-representable fp32 values (lossless, half the bytes)."""
    z = np.load(path)
    V, H, L, NH, I, P = (int(x) for x in z["cfg"])
    pad, cls_id, sep_id = (int(x) for x in z["special_ids"])
    cfg = O.EncoderConfig(vocab_size=V, hidden_size=H, num_hidden_layers=L, num_attention_heads=NH, intermediate_size=I,
                          pad_token_id=pad, cls_token_id=cls_id, sep_token_id=sep_id)
    hf_cfg = dict(vocab_size=V, hidden_size=H, num_hidden_layers=L, num_attention_heads=NH, intermediate_size=I,
                  max_position_embeddings=P, pad_token_id=pad, cls_token_id=cls_id, sep_token_id=sep_id,
                  bos_token_id=cls_id, eos_token_id=sep_id)
    enc = {k[len("enc:"):]: _bf16_to_f32(z[k]) for k in z.files if k.startswith("enc:")}
    n_pairs = int(z["n_pairs"])
    ids = [z[f"ids{i}"].astype(np.int32) for i in range(n_pairs)]
    models = {}
    for name in ("cls", "mean"):
        hd = {k.split(":", 2)[2]: _bf16_to_f32(z[k]) for k in z.files if k.startswith(f"head:{name}:")}
        bias = "head.dense.bias" in hd
        head = {"dense_w": hd["head.dense.weight"], "dense_b": hd.get("head.dense.bias"), "norm_w": hd["head.norm.weight"],
                "norm_b": None, "cls_w": hd["classifier.weight"], "cls_b": hd["classifier.bias"]}
        sd = {"model." + k: v for k, v in enc.items()}
        sd.update(hd)
        models[name] = {"pooling": name, "classifier_bias": bias, "head": head, "state_dict": sd,
                        "logits": z[f"logits:{name}"].astype(np.float32)}
    return {"cfg": cfg, "hf_cfg": hf_cfg, "encoder": enc, "models": models, "ids": ids}


def write_checkpoint(directory: str, fixture: dict, name: str, **config_overrides) -> None:
    """A ModernBertForSequenceClassification checkpoint directory (config.json + model.safetensors + the golden tokenizer)
    written with `safetensors.numpy` only -- no transformers needed."""
    import json
    import shutil

    from safetensors.numpy import save_file

    m = fixture["models"][name]
    os.makedirs(directory, exist_ok=True)
    cfg = dict(fixture["hf_cfg"], model_type="modernbert", architectures=["ModernBertForSequenceClassification"],
               classifier_pooling=m["pooling"], classifier_bias=m["classifier_bias"], classifier_activation="gelu",
               norm_bias=False, num_labels=int(m["head"]["cls_w"].shape[0]))
    cfg.update(config_overrides)
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({k: np.ascontiguousarray(v) for k, v in m["state_dict"].items()}, os.path.join(directory, "model.safetensors"))
    shutil.copy(os.path.join(os.path.dirname(GOLDEN), "tokenizer.json"), os.path.join(directory, "tokenizer.json"))
