"""Float64 attention reference and per-element error bound shared by the two attention unit suites: attend() holds the fused
Wqkv + RoPE + attention kernel's arithmetic (tests/test_qkv_attn_unit_gpu.py, whose module docstring derives its bound) and,
with kernel="attention", the standalone kernel's (csrc/attention.hip; tests/test_attn_unit_gpu.py derives that bound)."""
import numpy as np

from unit16 import U, from16, half_ulp, out16_bound, to16, trunc16


def attend(q, Eq, k, Ek, v, Ev, qi, kj, S, local, window, f16, p16=None, strict=True, exact_p=None, kernel="qkv", **kw):
    """Softmax(q k^T) v over keys with relative index kj admitted for the query at qi (j < S; banded |i - j| <= window), and
    the per-element bound.  p16: rounding of P to apply in the reference.  exact_p ("round" / "trunc"): the crafted case whose
    16-bit P is predictable bit for bit (test_lazy_reference): the reference rounds P itself and the bound grants P nothing.
    kernel: "qkv" = the fused kernel's arithmetic (everything below); "attention" = the standalone kernel's (attend_standalone)."""
    if kernel == "attention":
        assert p16 is None and not np.any(Eq) and not np.any(Ek) and not np.any(Ev), "the standalone kernel reads exact operands"
        return attend_standalone(q, k, v, qi, kj, S, local, window, f16, strict=strict, exact_p=exact_p, **kw)
    assert kernel == "qkv" and not kw
    s = q @ k.T
    ok = (kj[None, :] < S) & np.ones((len(qi), 1), bool)
    if local:
        ok &= np.abs(qi[:, None] - kj[None, :]) <= window
    s = np.where(ok, s, -np.inf)
    smax = s.max(1, keepdims=True)
    d = s - smax
    if exact_p:
        # every move of the reference is an integer, so the 16-bit rounding of P = 2^(s - m) is that of 2^frac(s), whatever the
        # schedule of the moves was; fp32 computes s - m exactly and v_exp_f32 is good to an ulp: no tie may lie that close
        assert np.all(smax == np.round(smax)) and np.all(np.where(ok, d * 8 == np.round(d * 8), True))
        n = np.floor(np.where(ok, d, 0.0))
        m2 = np.exp2(np.where(ok, d, 0.0) - n)
        lower = trunc16(m2, f16)
        at = (m2 - lower) / (2 * half_ulp(m2, f16))
        assert np.all((at == 0) | (np.abs(at - 0.5) > 1e-3)), "2^frac too close to a 16-bit tie"
        m16 = lower if exact_p == "trunc" else from16(to16(m2, f16), f16)
        p = np.where(ok, m16 * np.exp2(n), 0.0)
    else:
        p = np.exp2(d)
        if p16 is not None:
            p = p16(p)
    w = p / p.sum(1, keepdims=True)
    o = w @ v
    aq, ak = np.abs(q), np.abs(k)
    Es = Eq @ ak.T + aq @ Ek.T + Eq @ Ek.T + 2 * 66 * U * (aq @ ak.T + np.abs(smax))
    eta = np.exp2(np.minimum(Es, 60.0)) - 1 + (2.0 ** -11 if f16 else 2.0 ** -8) + 4 * U
    sub = 2.0 ** -25 if f16 else 0.0
    # additions that can round: the live keys (a masked P is an exact zero); a key 2^-30 below the row's maximum adds at most
    # its own magnitude to the error, whether it rounds away or not
    heavy = ok & (d >= -30)
    n_keys = (heavy if exact_p else ok).sum(1, keepdims=True)
    light = (np.where(ok & ~heavy, w, 0.0) @ np.abs(v)) if exact_p else 0.0
    if exact_p:
        eta, sub = np.zeros_like(eta), 0.0
    A = (w * eta).sum(1, keepdims=True) + ok.sum(1, keepdims=True) * sub
    assert not strict or np.all(A < 0.5), float(A.max())   # (a control's own bound is not used)
    A = np.minimum(A, 0.5)
    weta = w * eta + ok * sub
    err = np.zeros_like(o)
    if not exact_p:
        for i0 in range(0, len(qi), 64):   # sum_j w_j eta_j |v_j - o_i|, 64 queries at a time
            sl = slice(i0, i0 + 64)
            err[sl] = np.einsum("ij,ijd->id", weta[sl], np.abs(v[None, :, :] - o[sl, None, :]))
    err = err / (1 - A) + (w * (1 + eta)) @ Ev / (1 - A) + 2 * (n_keys + 16) * U * (w @ np.abs(v)) * 2 + light + 3 * U * np.abs(o)
    return o, out16_bound(o, err, f16)


def attend_standalone(q, k, v, qi, kj, S, local, window, f16, strict=True, exact_p=None, psum16=False, exact_o=False, drop=None):
    """csrc/attention.hip on exact 16-bit operands q, k [., 64], v [keys, 64]; returns (ref, bound) [len(qi), 64].

    What differs from the fused kernel (the derivation is in tests/test_attn_unit_gpu.py):
      * the row sum is built from the fp32 P, the P . V MFMA reads the 16-bit P: the rounding delta_j of P does NOT cancel, the
        output carries sum_j w_j delta_j v_j, granted as u16 sum_j w_j |v_j| (u16 = 2^-8 bf16, 2^-11 fp16);
      * the running maximum is exact per row, so P <= 1 and the row sum is >= 1; an fp16 P below 2^-14 is subnormal (2^-25
        absolute per key), a P below 2^-126 flushes;
      * one rescale of l (multiply, add) and of O (multiply) per 64-key tile, n_t = ceil(n_keys_spanned / 64) tiles at the most.
    exact_p ("round" / "trunc"): crafted scores whose 16-bit P is predictable bit for bit: the reference rounds (or, the
    control, truncates) P itself IN THE UNITS OF ITS TILE (2^(s - running maximum after that tile)) and the bound grants P
    nothing.  psum16 (control): the row sum built from the rounded P, the fused kernel's arithmetic.  exact_o: where the fp32
    error interval of the value to be stored holds no rounding tie of the 16-bit format the stored bits are predictable too:
    the reference is the rounded value and the bound the fp32 error alone."""
    assert not (psum16 or exact_o) or exact_p
    s = q @ k.T
    ok = (kj[None, :] < S) & np.ones((len(qi), 1), bool)
    if local:
        ok &= np.abs(qi[:, None] - kj[None, :]) <= window
    if drop is not None:   # a control's wrongly skipped keys
        ok &= ~drop
    s = np.where(ok, s, -np.inf)
    smax = s.max(1, keepdims=True)
    d = s - smax
    tile = kj // 64
    n_t = int(tile.max() - tile.min()) + 1
    u16 = 2.0 ** -11 if f16 else 2.0 ** -8
    sub = 2.0 ** -25 if f16 else 2.0 ** -126
    aq, ak, av = np.abs(q), np.abs(k), np.abs(v)
    if exact_p:
        # the running maximum after each tile, per row: integers by construction, so P in its tile's units is 2^(integer) times
        # P in the final units, and is rounded in ITS units (a subnormal fp16 P rounds on an absolute grid)
        tiles = np.unique(tile)
        run = np.full((len(qi), 1), -np.inf)
        m_tile = np.empty_like(s)
        for t in tiles:
            run = np.maximum(run, s[:, tile == t].max(1, keepdims=True))
            m_tile[:, tile == t] = run
        live = ok & np.isfinite(m_tile)
        assert np.all(np.where(live, m_tile == np.round(m_tile), True)) and np.all(smax == np.round(smax))
        assert np.all(np.where(live, s * 8 == np.round(s * 8), True))   # fp32 forms s - m exactly
        with np.errstate(invalid="ignore"):
            x = np.exp2(np.where(live, s - m_tile, -np.inf))     # P as the kernel sees it when it rounds it
        lower = trunc16(x, f16)
        at = (x - lower) / (2 * half_ulp(np.maximum(x, 1e-300), f16))
        assert np.all((at < 1e-3) | (np.abs(at - 0.5) > 1e-3) & (at < 1 - 1e-3)), "P too close to a 16-bit tie"
        x16 = lower if exact_p == "trunc" else from16(to16(x, f16), f16)
        with np.errstate(invalid="ignore"):
            scale = np.exp2(np.where(live, m_tile - smax, 0.0))
        p16, p = x16 * scale, np.exp2(d)
        L = (p16 if psum16 else p).sum(1, keepdims=True)
        w = p16 / L
        o = w @ v
        # fp32: v_exp_f32 is good to an ulp (2 U) in the row sum only -- the rounded P does not move
        err = 2 * (64 + 5 * n_t) * U * (w @ av) + (2 * n_t + 40) * U * np.abs(o)
        if exact_o:
            h = half_ulp(np.abs(o), f16)
            frac = np.abs(o) / h
            dist = np.abs(np.mod(frac, 2.0) - 1.0) * h          # to the nearest tie (an odd multiple of half an ulp)
            same_binade = np.floor(np.log2(np.maximum(np.abs(o) - err, 1e-300))) == np.floor(np.log2(np.maximum(np.abs(o) + err, 1e-300)))
            sure = (dist > 2 * err) & same_binade
            return np.where(sure, from16(to16(o, f16), f16), o), np.where(sure, err, out16_bound(o, err, f16))
        return o, out16_bound(o, err, f16)
    p = np.exp2(d)
    w = p / p.sum(1, keepdims=True)
    o = w @ v
    # scores: 64 products accumulated in fp32 from zero (twice the sequential count for the MFMA's internal order); the
    # subtraction of the maximum rounds once: U |d| in the exponent; v_exp_f32 is good to an ulp (2 U)
    Es = 2 * 64 * U * (aq @ ak.T) + U * np.abs(np.where(ok, d, 0.0))
    eta = np.where(ok, np.exp2(np.minimum(Es, 60.0)) - 1 + 2 * U, 0.0)
    A = (w * eta).sum(1, keepdims=True)
    assert not strict or np.all(A < 0.5), float(A.max())
    A = np.minimum(A, 0.5)
    weta = w * eta
    err = np.zeros_like(o)
    for i0 in range(0, len(qi), 64):   # sum_j w_j eta_j |v_j - o_i|, 64 queries at a time
        sl = slice(i0, i0 + 64)
        err[sl] = np.einsum("ij,ijd->id", weta[sl], np.abs(v[None, :, :] - o[sl, None, :]))
    p_round = (w * (1 + eta)) @ av * u16 + sub * (ok @ av)        # sum_j w_j (1 + eta_j) |delta_j| |v_j|, the row sum being >= 1
    err = (err + p_round) / (1 - A) + 2 * (64 + 5 * n_t) * U * (w @ av) + (2 * n_t + 38) * U * np.abs(o)
    return o, out16_bound(o, err, f16)
