"""float64 references of the six row launchers of csrc/norm_heads.hip, written from the arithmetic csrc/norm_heads.h documents
(not from the kernels' loops), and the per-element error bounds tests/test_rows_unit_gpu.py derives in its docstring.  CPU only:
numpy and math.  Every reference works on the fp32 values the kernel reads, lifted to float64, and takes `defect=`, the one
wrong step of a negative control (the names are listed at each function)."""
import math

import numpy as np

from unit16 import U, f32, from16, to16, trunc16

ERF_ULP, TANH_ULP = 16, 5      # OpenCL C single-precision limits of erf and tanh (see the test module's docstring)
SLOTS = 1024                   # register slots of a row: MAXV * 256
_erf = np.vectorize(math.erf, otypes=[np.float64])
_SQRT2 = math.sqrt(2.0)


def g(n):
    """n roundings in a chain: (1 + U)^n - 1 <= n U / (1 - n U)."""
    return n * U / (1.0 - n * U)


def lift(x):
    return None if x is None else np.asarray(f32(x), np.float64)


# ------------------------------------------------------------------ GELU
def gelu(x, defect=None):
    if defect == "gelu_tanh":
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + _erf(x / _SQRT2))


def gelu_bound(x, ex=0.0):
    """|gelu_erf(x~) - gelu(x)| for the kernel's 0.5f * x * (1.0f + erff(x * 0.70710678f)), |x~ - x| <= ex."""
    e = _erf(x / _SQRT2)
    # argument: the product rounds and the constant is itself rounded, each U relative on z; |z erf'(z)| <= 0.4839
    e1 = 2.0 * ERF_ULP * U * np.abs(e) + 2.0 * 0.4839 * U + U * np.abs(1.0 + e)
    return 0.5 * (np.abs(x) + ex) * e1 * (1.0 + U) + U * np.abs(gelu(x)) + 1.13 * ex      # sup |gelu'| = 1.1290


# ------------------------------------------------------------------ LayerNorm
def layer_norm(x, w, b, eps, defect=None):
    """LN(x) * w + b over the last axis, biased variance.  defects: var_H-1, eps_outside, one_pass_f32, padding_in_var,
    gain_first."""
    H = x.shape[-1]
    if defect == "gain_first" and w is not None:
        x, w = x * w, None
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    if defect == "var_H-1":
        var = (d * d).sum(-1, keepdims=True) / (H - 1)
    if defect == "padding_in_var":      # the unguarded loop: every padding slot holds 0 - mean
        var = ((d * d).sum(-1, keepdims=True) + (SLOTS - H) * mean * mean) / H
    if defect == "one_pass_f32":
        x32 = f32(x)
        m32 = (x32.sum(-1, keepdims=True, dtype=np.float32) / np.float32(H)).astype(np.float32)
        q32 = ((x32 * x32).sum(-1, keepdims=True, dtype=np.float32) / np.float32(H)).astype(np.float32)
        var = np.maximum((q32 - m32 * m32).astype(np.float64), 0.0)
    rstd = 1.0 / (np.sqrt(var) + eps) if defect == "eps_outside" else 1.0 / np.sqrt(var + eps)
    y = d * rstd
    if w is not None:
        y = y * w
    if b is not None:
        y = y + b
    return y, mean[..., 0]


def ln_bound(x, w, b, eps, ex=None):
    """(E_y [.., H], E_mean [..]) of the kernel's two-pass LayerNorm on inputs within ex of x: the module docstring's terms."""
    H = x.shape[-1]
    ex = np.zeros_like(x) if ex is None else np.broadcast_to(ex, x.shape)
    s1 = (np.abs(x) + ex).sum(-1, keepdims=True)
    m = x.mean(-1, keepdims=True)
    em = ex.mean(-1, keepdims=True) + g(21) * s1 / H          # 15 in-lane additions + 6 shuffle levels
    em = em + 2.0 * U * (np.abs(m) + em)                          # / H: one ulp
    d = x - m
    rho = U * (np.abs(d) + em + ex)                               # x - mean rounds once
    ed = em + ex + rho
    # sum d~^2 - sum d^2: the common shift (mean error) meets sum d = 0 and stays second order
    ds = (2.0 * np.abs(d) * (ex + rho) + (em + ex + rho) ** 2).sum(-1, keepdims=True)
    a = ((np.abs(d) + ed) ** 2).sum(-1, keepdims=True)
    var = (d * d).mean(-1, keepdims=True)
    evar = (ds + g(23) * a) / H                                   # product (or fma) + 15 + 6 additions
    evar = evar + 2.0 * U * (var + evar)                          # / H: one ulp
    s = var + eps
    es = evar + U * (s + evar)
    q = es / s
    assert float(q.max()) < 0.5, "the variance is not resolved at all: no first-order bound"
    er = (1.0 - q) ** -0.5 * (1.0 + 4.0 * U) - 1.0               # sqrtf and 1 / x: one ulp each
    r = s ** -0.5
    aw = 1.0 if w is None else np.abs(w)
    y0 = d * r * aw
    ey = r * aw * (ed * (1.0 + er) + np.abs(d) * er)
    ey = ey + g(2) * (np.abs(y0) + ey)                            # * rstd, * w
    if b is not None:
        y, _ = layer_norm(x, w, b, eps)
        ey = ey + U * (np.abs(y) + ey)
    return ey, em[..., 0]


def split_hi_lo(y32, f16, defect=None):
    """(hi, lo) float64 of an fp32 value: hi = T(x), lo = T(x - hi).  defect: hi_trunc."""
    y32 = f32(y32)
    hi = trunc16(y32, f16) if defect == "hi_trunc" else from16(to16(y32, f16), f16)
    lo = from16(to16(y32.astype(np.float64) - hi, f16), f16)
    return hi, lo


def split3_image(hi, lo, defect=None):
    """[hi | lo | hi], leading dimension 3 H.  defect: split3_weight_order = [hi | hi | lo]."""
    return np.concatenate([hi, hi, lo] if defect == "split3_weight_order" else [hi, lo, hi], axis=-1)


def layernorm(h, w, bias, eps, gelu_first=False, defect=None):
    """launch_layernorm: returns (y, mean, E_y, E_mean)."""
    x = lift(h)
    w, bias = lift(w), lift(bias)
    ex = None
    if gelu_first:
        ex = gelu_bound(x)
        x = gelu(x, defect)
    y, mean = layer_norm(x, w, bias, eps, defect)
    ey, em = ln_bound(x, w, bias, eps, ex)
    return y, mean, ey, em


# ------------------------------------------------------------------ embedding gather + LayerNorm
def embed_ln(ids, E, w, eps, P=None, pos=None, type_row=None, type_ids=None, bias=None, defect=None):
    """launch_embed_ln: h = LN((E[ids] + type) + P[pos]) * w + bias.  defects: pos_from_row, type_row0 (+ layer_norm's)."""
    E, P, type_row = lift(E), lift(P), lift(type_row)
    x = E[ids]
    ex = np.zeros_like(x)
    if P is not None:
        if type_row is not None:
            t = type_row[type_ids] if (type_ids is not None and defect != "type_row0") else type_row[0][None, :]
            x = x + t
            ex = U * np.abs(x)
        x = x + P[np.arange(len(ids)) if defect == "pos_from_row" else pos]
        ex = ex + U * (np.abs(x) + ex)
    y, _ = layer_norm(x, lift(w), lift(bias), eps, defect)
    ey, _ = ln_bound(x, lift(w), lift(bias), eps, ex)
    return y, ey


# ------------------------------------------------------------------ pooling
def _pool(y, ey, n_div=None):
    """Mean over the token axis 0 as the kernels take it: per-wave accumulation, a fixed 4-way add, * (1 / n)."""
    n = y.shape[0] if n_div is None else n_div
    v = y.sum(0) / n
    k = -(-y.shape[0] // 4)
    ev = (ey.sum(0) + g(k + 3) * (np.abs(y) + ey).sum(0)) / n
    return v, ev + 3.0 * U * (np.abs(v) + ev)       # 1 / n to one ulp, one multiply


def dot_bound(x, ex, wc):
    """sum x w over the last axis, 16 in-lane products and additions + 6 shuffle levels, inputs within ex."""
    return (ex * np.abs(wc)).sum(-1) + g(23) * ((np.abs(x) + ex) * np.abs(wc)).sum(-1)


def classify(x, ex, Wc, bc, defect=None):
    """(logits [.., L], bound) of x . Wc^T + bc.  defect: no_cls_bias."""
    Wc, bc = lift(Wc), lift(bc)
    z = x @ Wc.T
    ez = np.stack([dot_bound(x, ex, Wc[c]) for c in range(Wc.shape[0])], -1)
    out = z if defect == "no_cls_bias" else z + bc
    return out, ez + U * (np.abs(z + bc) + ez)


def range_pool(h, lnw, eps, start, end, mode, Wc=None, bc=None, defect=None):
    """launch_range_pool: list of (out, bound) per range.  defects: end_exclusive, mean_then_ln, no_cls_bias (+ layer_norm's).
    A mode 1 range whose mean vector is exactly zero returns (zeros, zeros): the 1e-12 floor applies."""
    h, lnw = lift(h), lift(lnw)
    res = []
    for s, e in zip(start, end):
        x = h[s:(e if defect == "end_exclusive" else e + 1)]
        if lnw is None:
            y, ey = x, np.zeros_like(x)
        elif defect == "mean_then_ln":
            y, _ = layer_norm(x.mean(0, keepdims=True), lnw, None, eps)
            ey = np.zeros_like(y)
        else:
            y, _ = layer_norm(x, lnw, None, eps, defect)
            ey, _ = ln_bound(x, lnw, None, eps)
        v, ev = _pool(y, ey)
        if mode == 0:
            res.append(classify(v, ev, Wc, bc, defect))
        elif mode == 1:
            q = (v * v).sum()
            if q == 0.0:
                res.append((np.zeros_like(v), np.zeros_like(v)))
                continue
            eq = (2.0 * np.abs(v) * ev + ev * ev).sum() + g(23) * ((np.abs(v) + ev) ** 2).sum()
            rel = eq / q
            assert rel < 0.5
            es = (1.0 - rel) ** -0.5 * (1.0 + 4.0 * U) - 1.0      # sqrtf and 1 / x: one ulp each
            sc = 1.0 / max(math.sqrt(q), 1e-12)
            out = v * sc
            eo = sc * (ev * (1.0 + es) + np.abs(v) * es)
            res.append((out, eo + U * (np.abs(out) + eo)))
        else:
            res.append((v, ev))
    return res


def ln_classifier(x, lnw, eps, Wc, bc, lnb=None, gelu_first=False, defect=None):
    """launch_ln_classifier: (logits, bound).  defects: gelu_tanh, no_cls_bias (+ layer_norm's)."""
    y, _, ey, _ = layernorm(x, lnw, lnb, eps, gelu_first, defect)
    return classify(y, ey, Wc, bc, defect)


def pooler_classifier(h, first_row, Wp, bp, Wc, bc, defect=None):
    """launch_pooler_classifier: (logits, bound, worst tanh argument error share).  defects: no_tanh, no_cls_bias."""
    x, Wp, bp = lift(h)[np.asarray(first_row)], lift(Wp), lift(bp)
    z = x @ Wp.T
    ez = g(23) * (np.abs(x) @ np.abs(Wp).T)
    a = z + bp
    ea = ez + U * (np.abs(a) + ez)
    p = a if defect == "no_tanh" else np.tanh(a)
    ep = ea + 2.0 * TANH_ULP * U * np.abs(np.tanh(a))      # |tanh'| <= 1
    return classify(p, ep, Wc, bc, defect)


def seq_pool(h, lnw, eps, seq_row, seq_len, pool_mean, defect=None):
    """Phase 1 of launch_seq_head: (pooled [n, H], bound).  defects: drop_tail, cls_row+1 (+ layer_norm's)."""
    h, lnw = lift(h), lift(lnw)
    out, err = [], []
    for r0, n in zip(seq_row, seq_len):
        if not pool_mean:
            r0, n = (r0 + 1 if defect == "cls_row+1" else r0), 1
        keep = n - n % 4 if defect == "drop_tail" else n
        x = h[r0:r0 + keep]
        y, _ = layer_norm(x, lnw, None, eps, defect)
        ey, _ = ln_bound(x, lnw, None, eps)
        v, ev = _pool(y, ey, n_div=n)
        out.append(v)
        err.append(ev)
    return np.asarray(out), np.asarray(err)


def seq_head_logits(pooled, WdT, bd, wn, bn, eps, Wc, bc, defect=None):
    """Phase 2 of launch_seq_head on the pooled rows it is GIVEN: (logits, bound).  defects: gelu_tanh, no_cls_bias."""
    p, WdT, bd = lift(pooled), lift(WdT), lift(bd)
    H = p.shape[-1]
    z = p @ WdT
    ez = g(H) * (np.abs(p) @ np.abs(WdT))                   # one fmaf chain of H steps per column, from zero
    if bd is not None:
        z = z + bd
        ez = ez + U * (np.abs(z) + ez)
    x = gelu(z, defect)
    ex = gelu_bound(z, ez)
    y, _ = layer_norm(x, lift(wn), lift(bn), eps)
    ey, _ = ln_bound(x, lift(wn), lift(bn), eps, ex)
    return classify(y, ey, Wc, bc, defect)


# ------------------------------------------------------------------ input families
def make_rows(rng, family, rows, H, eps=1e-5):
    """fp32 rows of one of the three families: unit variance; mean 100 over sigma 0.01 with a few outlier channels; near-constant
    rows whose variance is of the order of eps."""
    z = rng.standard_normal((rows, H))
    if family == "unit":
        x = z
    elif family == "offset":
        x = 100.0 + 0.01 * z
        for c in sorted({1 % H, 77 % H, 200 % H}):
            x[:, c] += 0.5 * rng.standard_normal(rows)
    elif family == "const":
        x = rng.uniform(0.5, 2.0, (rows, 1)) * np.sign(rng.standard_normal((rows, 1))) + math.sqrt(eps) * z
    else:
        raise ValueError(family)
    return f32(x)

