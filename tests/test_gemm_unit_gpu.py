"""The GEMM alone (vrag_debug_gemm_run, csrc/gemm_bf16.hip) against float64 on the SAME 16-bit operands the kernel reads, for
every epilogue the encoder launches and every tile configuration launch_t chooses outside the top-k search.

Each check is the kernel's stated arithmetic (gemm_bf16.h), not the model around it: the LayerNorm fold is checked as
rstd * (A . W'^T - mu * s) on the given A, the split residual stream by chaining launches the way the encoder does (no decoder of
the byte plane in the test).  Error bounds are derived per element:
  accumulation   2 K 2^-24 (|A| . |W|^T)[m, n], plus 2^-24 |x| for every fp32 operation of the epilogue on x;
  16-bit output  + half an ulp of the output type at |ref| (truncation or double rounding fails it);
  split stream   + 2^-16 |v| (bf16 planes) or 2^-19 |v| (fp16) per sub-layer, plus fp16's subnormal spacing;
  transcendentals + gelu_fast's documented 6e-7 (common.h) and a few fp32 ulps for erff / log1pf.
Negative controls check, on the same outputs, that each bound rejects the nearest wrong kernel (a K-step or the bias dropped,
the byte plane dropped, RoPE's partner d + 16, truncation).  `-rP` prints the worst error / bound ratio per epilogue form and
tile configuration."""
import ctypes as C
import math

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib
from unit16 import U, f32, from16, half_ulp, make_ledger, out16_bound, to16, trunc16

pytestmark = pytest.mark.gpu

EPI_F32, EPI_BF16, EPI_F32_GELU, EPI_RESIDUAL, EPI_GEGLU, EPI_QKV_ROPE, EPI_SPLADE = 0, 1, 2, 3, 4, 5, 6
BIG_ROWS = 1 << 30      # small-batch threshold that keeps every shape on the launch-bound configurations
Q_SCALE = np.float32(0.125 * 1.4426950408889634)   # what the encoder passes: head_dim^-1/2 * log2 e

# launch_t's configurations (BM, BN, WM, WN, NS, HW, KCH) and their grid caps
KSPLIT, KCH64, KCH128 = (64, 64, 1, 1, 8, 3, 0), (64, 64, 1, 1, 4, 0, 1), (128, 128, 2, 2, 4, 0, 1)
SMALL8, SMALL4 = (128, 128, 4, 2, 4, 0, 0), (128, 128, 2, 2, 4, 0, 0)
TILE256, TILE128 = (256, 256, 2, 4, 2, 0, 0), (128, 128, 2, 2, 2, 0, 0)
ALL_CONFIGS = {KSPLIT: 1024, KCH64: 1024, KCH128: 256, SMALL8: 256, SMALL4: 256, TILE256: 256, TILE128: 512}

_SEEN = set()                                  # (config, f16) of every launch of the module
_WORST, record, control = make_ledger()        # (form, config, f16) -> worst error / bound


def expected_config(epi, M, N, hidden=0, small_rows=8192):
    """launch_t's choice, restated from its inequalities (gemm_bf16.hip)."""
    if M <= small_rows:
        if epi == EPI_RESIDUAL:
            if -(-M // 128) * (N // 128) <= 128:
                return KSPLIT if -(-M // 64) * (N // 64) <= 256 else KCH64
            return KCH128
        return SMALL8 if epi in (EPI_QKV_ROPE, EPI_GEGLU, EPI_BF16) else SMALL4
    if N % 256 == 0 and M >= 256 and (epi != EPI_QKV_ROPE or hidden % 256 == 0):
        return TILE256
    return TILE128


# ------------------------------------------------------------------ the hook
def run(epi, M, N, K, f16, rows=None, row0=0, small_rows=-1, hidden=0, rope_rows=0, n_seqs=0, fin_eps=1e-5, act_gelu=0,
        expect=None, **bufs):
    """One launch through vrag_debug_gemm_run; in / out arrays are updated in place.  Returns (config, f16 saturation flag)."""
    dbg = _lib.load_debug()
    a = _lib.DebugGemmArgs()
    for name, arr in bufs.items():
        if arr is None:
            continue
        assert isinstance(arr, np.ndarray) and arr.flags.c_contiguous and arr.flags.writeable, name
        setattr(a, name, arr.ctypes.data)
    a.epi, a.M, a.N, a.K, a.f16, a.act_gelu = epi, M, N, K, int(f16), act_gelu
    a.row0, a.rows = row0, rows if rows is not None else -(-M // 256) * 256
    a.hidden, a.rope_rows, a.n_seqs, a.small_rows = hidden, rope_rows, n_seqs, small_rows
    a.q_scale, a.fin_eps = float(Q_SCALE), fin_eps
    status = dbg.vrag_debug_gemm_run(C.byref(a), 0)
    if status == -2:   # VRAG_ERR_HIP: a failed launch or a clobbered canary: nothing more goes onto this device
        msg = dbg.vrag_last_error()
        pytest.exit(f"vrag_debug_gemm_run: {msg.decode() if msg else status}", returncode=3)
    _lib.check_debug("vrag_debug_gemm_run", status)
    cfg = tuple(a.config)
    _SEEN.add((cfg, bool(f16)))
    thr = 8192 if small_rows < 0 else small_rows
    assert cfg == (expect or expected_config(epi, M, N, hidden, thr)), (epi, M, N, cfg)
    return cfg, a.f16_saturated


def operands(rng, M, N, K, f16, rows=None, sa=1.0, sw=1.0, pad=None):
    """A [rows, K] (rows >= M; rows M.. zero or `pad`-scaled random), W [N, K] as bits, and their float64 values (A: M rows)."""
    rows = rows or -(-M // 256) * 256
    a = np.zeros((rows, K))
    a[:M] = rng.standard_normal((M, K)) * sa
    a[M:] = rng.uniform(-1, 1, (rows - M, K)) * (pad or 0.0)   # drawn either way: the same operands with or without `pad`
    A = to16(a, f16)
    W = to16(rng.standard_normal((N, K)) * sw, f16)
    return A, W, from16(A[:M], f16), from16(W, f16)


def sample_rows(M, bm):
    """Rows the float64 reference is computed on: all of them for small M, else the first and last row of every row tile and
    every residue of row mod 64."""
    if M <= 1024:
        return np.arange(M)
    r = set(range(64)) | {M - 1}
    for t in range(0, M, bm):
        r |= {t, min(t + bm, M) - 1}
    return np.array(sorted(r))


def acc_ref(Af, Wf, rows):
    a = Af[rows]
    return a @ Wf.T, 2 * Af.shape[1] * U * (np.abs(a) @ np.abs(Wf).T)


# ------------------------------------------------------------------ EPI_F32 / EPI_F32_GELU
F32_CASES = [  # M, N, K, bias, small_rows
    (1, 128, 64, False, -1), (17, 384, 192, True, -1), (64, 768, 320, True, -1), (257, 768, 1152, True, -1),
    (256, 768, 128, True, 0), (255, 384, 768, False, 0), (7300, 1152, 64, True, BIG_ROWS), (7300, 1152, 64, True, 0)]


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("M,N,K,bias,small", F32_CASES)
def test_f32(M, N, K, bias, small, f16):
    rng = np.random.default_rng(M * 7 + N + K + f16)
    A, W, Af, Wf = operands(rng, M, N, K, f16)
    b = f32(rng.standard_normal(N)) if bias else None
    out = np.zeros((A.shape[0], N), np.float32)
    cfg, sat = run(EPI_F32, M, N, K, f16, small_rows=small, A=A, W=W, bias=b, out_f32=out)
    assert sat == 0
    rows = sample_rows(M, cfg[0])
    acc, e = acc_ref(Af, Wf, rows)
    ref = acc + (b if bias else 0)
    bound = e + 2 * U * np.abs(ref) + 1e-30
    record("F32" + ("+bias" if bias else ""), cfg, f16, out[rows], ref, bound)
    if bias:
        control("F32 bias dropped", out[rows] - b, ref, bound)
    # one K-step of 64 dropped
    k0 = 64 * (K // 128)
    ks = slice(k0, k0 + 64)
    control("F32 K-step dropped", out[rows] - Af[rows][:, ks] @ Wf[:, ks].T, ref, bound)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("M,N,K,small", [(16, 128, 128, -1), (65, 768, 768, -1), (300, 384, 64, 0)])
def test_f32_gelu(M, N, K, small, f16):
    rng = np.random.default_rng(M + N + K + f16)
    A, W, Af, Wf = operands(rng, M, N, K, f16, sw=1 / math.sqrt(K) * 2)
    b = f32(rng.standard_normal(N))
    out = np.zeros((A.shape[0], N), np.float32)
    cfg, _ = run(EPI_F32_GELU, M, N, K, f16, small_rows=small, A=A, W=W, bias=b, out_f32=out)
    acc, e = acc_ref(Af, Wf, np.arange(M))
    x = acc + b
    ref = 0.5 * x * (1 + np.vectorize(math.erf)(x / math.sqrt(2)))
    ex = e + U * np.abs(x)
    bound = 1.13 * ex + 0.5 * np.abs(x) * 8 * U + 4 * U * np.abs(ref) + 1e-30
    record("F32_GELU+bias", cfg, f16, out[:M], ref, bound)
    control("F32_GELU bias dropped", 0.5 * acc * (1 + np.vectorize(math.erf)(acc / math.sqrt(2))), ref, bound)


# ------------------------------------------------------------------ LayerNorm-fold inputs
def fold_inputs(rng, M, K, N, f16, W, rows, finalize):
    """Fold operands as the encoder builds them: A = op16(h - c) for a per-row shift c; ln_s = row sums of W'.  With
    `finalize`, the slice-major partial statistics of (h - c) for the consumer-side finalisation (ln_mu / ln_rstd then come
    out of the kernel); otherwise ln_mu / ln_rstd are given."""
    h = rng.standard_normal((M, K)) * 1.5 + rng.standard_normal((M, 1)) * 2
    c = f32(np.zeros(rows))
    c[:M] = h.mean(1) + rng.standard_normal(M) * 0.3
    x = f32(h - c[:M, None])
    a = np.zeros((rows, K))
    a[:M] = x
    A = to16(a, f16)
    s = f32(from16(W, f16).sum(1))
    mu, rstd = f32(np.zeros(rows)), f32(np.ones(rows))
    st = None
    if finalize:
        st = np.zeros((K // 64, rows, 2), np.float32)
        xs = x.astype(np.float32).reshape(M, K // 64, 64)
        st[:, :M, 0] = xs.sum(2, dtype=np.float32).T
        st[:, :M, 1] = (xs * xs).sum(2, dtype=np.float32).T
    else:
        mu[:M] = x.mean(1)
        rstd[:M] = 1 / np.sqrt(x.var(1) + 1e-5)
    return A, c, s, mu, rstd, st


def check_finalize(form, cfg, f16, M, K, st, c_in, mu, rstd, shift, shift_prev, eps=1e-5):
    """ln_mu / ln_rstd / ln_shift / ln_shift_prev as the consumer GEMM's finalisation writes them."""
    npart = K // 64
    s1 = st[:, :M, 0].astype(np.float64).sum(0)
    s2 = st[:, :M, 1].astype(np.float64).sum(0)
    d = s1 / K
    var = np.maximum(s2 / K - d * d, 0)
    e_d = (npart + 2) * U * np.abs(st[:, :M, 0]).astype(np.float64).sum(0) / K
    record(form + " ln_mu", cfg, f16, mu[:M], d, e_d + 1e-30)
    e_var = (npart + 3) * U * s2 / K + 2 * np.abs(d) * e_d + 3 * U * (d * d + var + eps)
    r_ref = 1 / np.sqrt(var + eps)
    record(form + " ln_rstd", cfg, f16, rstd[:M], r_ref, r_ref * (0.5 * e_var / (var + eps) + 4 * U))
    record(form + " ln_shift", cfg, f16, shift[:M], c_in[:M].astype(np.float64) + d, e_d + U * np.abs(c_in[:M] + d) + 1e-30)
    if shift_prev is not None:
        assert np.array_equal(shift_prev[:M], c_in[:M])


def fold_ref(acc, e, mu, rstd, s):
    """rstd * (acc - mu s) and its bound (mu, rstd, s: the fp32 values the kernel read)."""
    mu, rstd, s = mu[:, None].astype(np.float64), rstd[:, None].astype(np.float64), s[None, :].astype(np.float64)
    t = acc - mu * s
    v = rstd * t
    return v, np.abs(rstd) * (e + 2 * U * (np.abs(acc) + np.abs(mu * s))) + U * np.abs(v)


# ------------------------------------------------------------------ EPI_BF16
BF16_CASES = [  # M, N, K, small_rows
    (15, 384, 192, -1), (63, 768, 768, -1), (256, 128, 64, -1), (257, 768, 1152, -1), (257, 768, 320, 0), (255, 384, 128, 0)]


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("form", ["plain", "bias", "bias+gelu", "fold+finalize", "fold+bias", "fold+bias+gelu"])
@pytest.mark.parametrize("M,N,K,small", BF16_CASES)
def test_bf16_out(M, N, K, small, form, f16):
    rng = np.random.default_rng(M * 3 + N + K + f16 + len(form))
    rows = -(-M // 256) * 256
    A, W, Af, Wf = operands(rng, M, N, K, f16, sw=1 / math.sqrt(K) * 2)
    bias = f32(rng.standard_normal(N) * 0.5) if "bias" in form else None
    gelu = int("gelu" in form)
    thr = 8192 if small < 0 else small
    finalize = "finalize" in form and M <= thr   # consumer finalisation: small-row configuration only
    fold = {}
    if "fold" in form:
        A, c, s, mu, rstd, st = fold_inputs(rng, M, K, N, f16, W, rows, finalize)
        Af = from16(A[:M], f16)
        shift, shift_prev = c.copy(), f32(np.full(rows, 7.0))
        fold = dict(ln_mu=mu, ln_rstd=rstd, ln_s=s, stats_in=st, ln_shift=shift if finalize else None,
                    ln_shift_prev=shift_prev if finalize else None)
    out = np.zeros((rows, N), np.uint16)
    cfg, sat = run(EPI_BF16, M, N, K, f16, small_rows=small, act_gelu=gelu, A=A, W=W, bias=bias, out_bf16=out, **fold)
    assert sat == 0
    acc, e = acc_ref(Af, Wf, np.arange(M))
    v = acc
    if fold:
        if finalize:
            check_finalize("BF16 " + form, cfg, f16, M, K, st, c, mu, rstd, shift, shift_prev)
        v, e = fold_ref(acc, e, mu[:M], rstd[:M], s)
    if bias is not None:
        v = v + bias
        e = e + U * np.abs(v)
    pre = v
    if gelu:
        ref = 0.5 * v * (1 + np.vectorize(math.erf)(v / math.sqrt(2)))
        e = 1.13 * e + 6e-7 + 4 * U * np.abs(v)
    else:
        ref = v
    bound = out16_bound(ref, e, f16)
    got = from16(out[:M], f16)
    record("BF16 " + form, cfg, f16, got, ref, bound)
    if bias is not None and not gelu:
        control("BF16 bias dropped", got - bias, ref, bound)
    if form == "plain" and K >= 128:
        ks = slice(64, 128)
        control("BF16 K-step dropped", from16(to16(acc - Af[:, ks] @ Wf[:, ks].T, f16), f16), ref, bound)
    if form == "plain" and K == 64:   # (a small accumulation term: the rounding allowance dominates the bound)
        # truncation instead of round-to-nearest-even: at most one ulp against a half-ulp allowance, so it cannot reach 10 x;
        # it must still break the bound, on a sizeable share of the elements
        wrong = trunc16(pre, f16)
        r = np.abs(wrong - ref) / bound
        _WORST[("control: truncation (max ratio)", None, f16)] = max(_WORST[("control: truncation (max ratio)", None, f16)],
                                                                    float(r.max()))
        assert r.max() > 1.5 and np.mean(r > 1) > 0.05, (float(r.max()), float(np.mean(r > 1)))


# ------------------------------------------------------------------ EPI_RESIDUAL (fp32 stream)
RES_CASES = [  # M, N, K, small_rows
    (1, 128, 64, -1), (16, 768, 192, -1), (65, 384, 320, -1), (255, 768, 768, -1), (1345, 768, 1152, -1), (2689, 768, 128, -1),
    (300, 768, 320, 0), (257, 384, 768, 0)]


def stats_check(form, cfg, f16, st, v64, e_v, M, N):
    """stats_part [N / 64][rows][2] against float64 slice sums of v (= the updated stream minus the shift)."""
    vs, es = v64.reshape(M, N // 64, 64), e_v.reshape(M, N // 64, 64)
    s1 = vs.sum(2).T
    s2 = (vs * vs).sum(2).T
    b1 = (es.sum(2) + 8 * U * np.abs(vs).sum(2)).T + 1e-30
    b2 = ((2 * np.abs(vs) * es + es * es).sum(2) + 12 * U * (vs * vs).sum(2)).T + 1e-30
    record(form + " stats sum", cfg, f16, st[:, :M, 0], s1, b1)
    record(form + " stats sumsq", cfg, f16, st[:, :M, 1], s2, b2)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("form", ["bias", "postln", "shift+resid+stats"])
@pytest.mark.parametrize("M,N,K,small", RES_CASES)
def test_residual(M, N, K, small, form, f16):
    rng = np.random.default_rng(M + N * 5 + K + f16 + len(form))
    rows = -(-M // 256) * 256
    A, W, Af, Wf = operands(rng, M, N, K, f16, sw=1 / math.sqrt(K))
    h = f32(rng.standard_normal((rows, N)) * 2 + 1)
    out = h.copy()
    kw = {}
    if form == "bias" or form == "postln":
        kw["bias"] = f32(rng.standard_normal(N) * 0.5)
    if form == "postln":
        kw.update(res_mu=f32(rng.standard_normal(rows)), res_rstd=f32(rng.uniform(0.5, 2, rows)),
                  res_g=f32(rng.uniform(0.5, 1.5, N)), res_b=f32(rng.standard_normal(N) * 0.1))
    if form == "shift+resid+stats":
        kw.update(ln_shift=f32(rng.standard_normal(rows) + 1), resid_bf16=np.zeros((rows, N), np.uint16),
                  stats_part=np.zeros((N // 64, rows, 2), np.float32))
    cfg, sat = run(EPI_RESIDUAL, M, N, K, f16, small_rows=small, A=A, W=W, out_f32=out, **kw)
    assert sat == 0
    acc, e = acc_ref(Af, Wf, np.arange(M))
    hin = h[:M].astype(np.float64)
    e_h = 0
    if form == "postln":
        mu, r = kw["res_mu"][:M, None].astype(np.float64), kw["res_rstd"][:M, None].astype(np.float64)
        g, b = kw["res_g"].astype(np.float64), kw["res_b"].astype(np.float64)
        hin = (hin - mu) * r * g + b
        e_h = 4 * U * ((np.abs(h[:M]) + np.abs(mu)) * np.abs(r) * g + np.abs(b))
    v = acc + (kw["bias"] if "bias" in kw else 0)
    ref = v + hin
    bound = e + U * np.abs(v) + e_h + U * np.abs(ref) + 1e-30
    record("RESIDUAL " + form, cfg, f16, out[:M], ref, bound)
    if "bias" in kw:
        control("RESIDUAL bias dropped", out[:M] - kw["bias"], ref, bound)
    if form == "shift+resid+stats":
        vk = out[:M].astype(np.float64) - kw["ln_shift"][:M, None]   # the kernel's own fp32 rows minus the shift
        ek = U * np.abs(vk)
        record("RESIDUAL resid_bf16", cfg, f16, from16(kw["resid_bf16"][:M], f16), vk, out16_bound(vk, ek, f16))
        stats_check("RESIDUAL", cfg, f16, kw["stats_part"], vk, ek, M, N)


# ------------------------------------------------------------------ EPI_RESIDUAL, split stream
def split_q(f16):
    return 2.0 ** -19 if f16 else 2.0 ** -16


def split_chain(rng, M, N, Ks, f16, rows=None, sw=0.05, h_scale=4.0, small=-1):
    """Leaves split (leg 0), arrives and leaves split (legs 1 .. n-2), arrives split and leaves fp32 rows (last leg), with
    per-row shifts that differ from row to row and from leg to leg.  Returns the per-leg records and the final fp32 rows."""
    rows = rows or -(-M // 256) * 256
    h0 = f32(rng.standard_normal((rows, N)) * h_scale + 3)
    shifts = [f32(h0.mean(1) + rng.standard_normal(rows) * 0.5 + i * 0.25) for i in range(len(Ks))]
    hi = np.zeros((rows, N), np.uint16)
    lo = np.zeros(rows * N, np.uint8)
    out = h0.copy()
    h_abs = h0[:M].astype(np.float64)   # float64 h + sum A_i W_i^T
    e_stream = np.zeros((M, N))         # |represented stream - exact| (absolute rows)
    legs = []
    for i, K in enumerate(Ks):
        A, W, Af, Wf = operands(rng, M, N, K, f16, rows=rows, sw=sw)
        acc, e = acc_ref(Af, Wf, np.arange(M))
        first, last = i == 0, i == len(Ks) - 1
        kw = dict(A=A, W=W, resid_bf16=hi)
        if not first:
            kw.update(lo_in=lo, ln_shift_prev=shifts[i - 1].copy())
        if not last:
            kw.update(lo_out=lo, ln_shift=shifts[i].copy(), stats_part=np.zeros((N // 64, rows, 2), np.float32))
        if first or last:
            kw["out_f32"] = out
        cfg, sat = run(EPI_RESIDUAL, M, N, K, f16, rows=rows, small_rows=small, **kw)
        assert sat == 0
        h_abs = h_abs + acc
        c_out = shifts[i][:M, None].astype(np.float64) if not last else 0.0
        v = h_abs - c_out
        c_in = shifts[i - 1][:M, None].astype(np.float64) if not first else 0.0
        e_v = e_stream + e + U * (np.abs(acc) + np.abs(c_in - c_out) + 3 * np.abs(v) + np.abs(h_abs))
        leg = dict(cfg=cfg, v=v, e_v=e_v, acc_e=e)
        if not last:
            leg.update(hi=from16(hi[:M], f16), stats=kw["stats_part"])
            e_stream = e_v + split_q(f16) * np.abs(v) * 1.01 + (2.0 ** -24 if f16 else 0) + U * np.abs(v)
        legs.append(leg)
    return legs, out, h_abs


SPLIT_CASES = [  # M, N, Ks (one per leg), small_rows
    (17, 768, (64, 1152), -1), (64, 384, (192, 320, 768), -1), (257, 768, (768, 1152, 768, 1152), -1), (1345, 768, (320, 128), -1),
    (2689, 768, (64, 192, 128), -1), (300, 768, (128, 320, 64), 0), (300, 384, (64, 192), 0)]


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("M,N,Ks,small", SPLIT_CASES)
def test_residual_split_stream(M, N, Ks, small, f16):
    rng = np.random.default_rng(M + N + sum(Ks) + f16)
    legs, out, h_abs = split_chain(rng, M, N, Ks, f16, small=small)
    for i, leg in enumerate(legs[:-1]):
        form = "RESIDUAL split " + ("leaves" if i == 0 else "both")
        record(form + " resid_bf16", leg["cfg"], f16, leg["hi"], leg["v"], out16_bound(leg["v"], leg["e_v"], f16))
        stats_check(form, leg["cfg"], f16, leg["stats"], leg["v"], leg["e_v"], M, N)
    last = legs[-1]
    record("RESIDUAL split arrives (fp32 rows)", last["cfg"], f16, out[:M], h_abs, last["e_v"] + 1e-30)


@pytest.mark.parametrize("f16", [False, True])
def test_split_stream_control_byte_plane(f16):
    """The split bound rejects the stream without its byte plane (the operand plane alone), on a case whose accumulation term
    is small against the stream's own precision (K = 64, small weights)."""
    rng = np.random.default_rng(11 + f16)
    M, N = 200, 384
    legs, out, h_abs = split_chain(rng, M, N, (64, 64, 64), f16, sw=0.02)
    record("RESIDUAL split arrives (fp32 rows)", legs[-1]["cfg"], f16, out[:M], h_abs, legs[-1]["e_v"] + 1e-30)
    leg = legs[0]
    bound = leg["e_v"] + split_q(f16) * np.abs(leg["v"]) * 1.01 + (2.0 ** -24 if f16 else 0)
    control("split stream without its byte plane", leg["hi"], leg["v"], bound)


# ------------------------------------------------------------------ EPI_GEGLU
def geglu_interleave(Wi):
    """capi.hip cvt_rows_bf16_kernel with interleave_I: each 64-row group = 32 input rows (x1), then the 32 gate rows (x2)."""
    I = Wi.shape[0] // 2
    out = np.zeros_like(Wi)
    for g in range(I // 32):
        out[g * 64:g * 64 + 32] = Wi[g * 32:g * 32 + 32]
        out[g * 64 + 32:g * 64 + 64] = Wi[I + g * 32:I + g * 32 + 32]
    return out


def gelu_erf64(x):
    return 0.5 * x * (1 + np.vectorize(math.erf)(x / math.sqrt(2)))


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("M,N,K,small", [(1, 384, 128, -1), (64, 2304, 768, -1), (257, 768, 320, -1), (256, 2304, 64, 0),
                                         (300, 384, 192, 0)])
def test_geglu(M, N, K, small, fold, f16):
    rng = np.random.default_rng(M + N + K + fold + f16)
    rows = -(-M // 256) * 256
    I = N // 2
    Wi = rng.standard_normal((N, K)) * 2 / math.sqrt(K)          # [input rows | gate rows], HF layout
    W = to16(geglu_interleave(Wi), f16)
    Wf = from16(W, f16)
    A, _, Af, _ = operands(rng, M, N, K, f16)
    kw = {}
    if fold:
        thr = 8192 if small < 0 else small
        fin = M <= thr
        A, c, s, mu, rstd, st = fold_inputs(rng, M, K, N, f16, W, rows, fin)
        Af = from16(A[:M], f16)
        shift = c.copy()
        kw = dict(ln_mu=mu, ln_rstd=rstd, ln_s=s, stats_in=st, ln_shift=shift if fin else None)
    out = np.zeros((rows, I), np.uint16)
    cfg, sat = run(EPI_GEGLU, M, N, K, f16, small_rows=small, A=A, W=W, out_bf16=out, **kw)
    assert sat == 0
    acc, e = acc_ref(Af, Wf, np.arange(M))
    if fold:
        if fin:
            check_finalize("GEGLU fold", cfg, f16, M, K, st, c, mu, rstd, shift, None)
        acc, e = fold_ref(acc, e, mu[:M], rstd[:M], s)
    # un-interleave: output feature f = 32 g + w <- rows 64 g + w (x1) and 64 g + 32 + w (x2)
    f = np.arange(I)
    i1 = (f // 32) * 64 + f % 32
    x1, x2, e1, e2 = acc[:, i1], acc[:, i1 + 32], e[:, i1], e[:, i1 + 32]
    g1 = gelu_erf64(x1)
    ref = g1 * x2
    e_g = 1.13 * e1 + 6e-7 + 4 * U * np.abs(x1)
    bound = out16_bound(ref, e_g * np.abs(x2) + (np.abs(g1) + e_g) * e2 + 3 * U * np.abs(ref), f16)
    record("GEGLU" + (" fold" if fold else ""), cfg, f16, from16(out[:M], f16), ref, bound)
    if not fold:   # the interleave's nearest slip: the partner half swapped (gelu on the gate instead of the input)
        control("GEGLU halves swapped", gelu_erf64(x2) * x1, ref, bound)


# ------------------------------------------------------------------ EPI_QKV_ROPE
def rope64(x, cos, sin, partner=32):
    """Rotate-half RoPE on [rows, 64] head slices: r[d] = x[d] cos[d % 32] -+ x[(d + partner) % 64] sin[d % 32] (minus for
    d < 32).  partner = 32 is the pairing (d, d + 32); 16 the nearest slip."""
    d = np.arange(64)
    c, s = np.concatenate([cos, cos], 1), np.concatenate([sin, sin], 1)
    return x * c + np.where(d < 32, -1.0, 1.0) * x[:, (d + partner) % 64] * s


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("fold,bias", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,hidden,K,small", [(16, 128, 128, -1), (65, 256, 256, -1), (255, 384, 384, -1),
                                              (257, 768, 768, -1), (256, 256, 64, 0), (257, 384, 192, 0), (300, 768, 128, 0)])
def test_qkv_rope(M, hidden, K, small, fold, bias, f16):
    rng = np.random.default_rng(M + hidden + K + 2 * fold + bias + f16)
    rows = -(-M // 256) * 256
    N = 3 * hidden
    A, W, Af, Wf = operands(rng, M, N, K, f16, sw=1 / math.sqrt(K))
    rope_rows = 96
    ang = rng.uniform(0, 2 * math.pi, (rope_rows, 32))
    cos, sin = f32(np.cos(ang)), f32(np.sin(ang))
    pos = np.zeros(rows, np.int32)
    pos[:M] = rng.integers(0, rope_rows, M)
    kw = dict(bias=f32(rng.standard_normal(N) * 0.3) if bias else None)
    if fold:
        thr = 8192 if small < 0 else small
        fin = M <= thr
        A, c, s, mu, rstd, st = fold_inputs(rng, M, K, N, f16, W, rows, fin)
        Af = from16(A[:M], f16)
        kw.update(ln_mu=mu, ln_rstd=rstd, ln_s=s, stats_in=st, ln_shift=c.copy() if fin else None)
    q, k, vt = (np.zeros((rows, hidden), np.uint16), np.zeros((rows, hidden), np.uint16), np.zeros((hidden, rows), np.uint16))
    cfg, sat = run(EPI_QKV_ROPE, M, N, K, f16, small_rows=small, hidden=hidden, rope_rows=rope_rows, A=A, W=W, q=q, k=k, vt=vt,
                   rope_cos=cos, rope_sin=sin, pos=pos, **kw)
    assert sat == 0
    acc, e = acc_ref(Af, Wf, np.arange(M))
    if fold:
        if fin:
            check_finalize("QKV fold", cfg, f16, M, K, st, c, mu, rstd, kw["ln_shift"], None)
        acc, e = fold_ref(acc, e, mu[:M], rstd[:M], s)
    if bias:
        acc = acc + kw["bias"]
        e = e + U * np.abs(acc)
    cz, sz = cos[pos[:M]].astype(np.float64), sin[pos[:M]].astype(np.float64)
    c64, s64 = np.abs(np.concatenate([cz, cz], 1)), np.abs(np.concatenate([sz, sz], 1))   # |cos|, |sin| per feature d of a head
    form = "QKV" + (" fold" if fold else "") + (" bias" if bias else "")
    for which, dst, scale in ((0, q, float(Q_SCALE)), (1, k, 1.0)):
        for hd in range(hidden // 64):
            cols = slice(which * hidden + hd * 64, which * hidden + hd * 64 + 64)
            x, ex = acc[:, cols], e[:, cols]
            ref = rope64(x, cz, sz) * scale
            xp, ep = np.roll(x, 32, axis=1), np.roll(ex, 32, axis=1)   # the rotation partner of every feature
            er = (c64 * ex + s64 * ep + 3 * U * (np.abs(x) * c64 + np.abs(xp) * s64)) * scale
            er = er + U * np.abs(ref)
            bound = out16_bound(ref, er, f16)
            got = from16(dst[:M, hd * 64:hd * 64 + 64], f16)
            record(form + (" q" if which == 0 else " k"), cfg, f16, got, ref, bound)
            if which == 0 and hd == 0 and not fold and not bias:
                control("RoPE partner d+16", rope64(x, cz, sz, partner=16) * scale, ref, bound)
                control("q scale dropped", ref / scale, ref, bound)
    xv, ev = acc[:, 2 * hidden:], e[:, 2 * hidden:]
    record(form + " v^T", cfg, f16, from16(vt[:, :M].T, f16), xv, out16_bound(xv, ev, f16))


# ------------------------------------------------------------------ EPI_SPLADE
def splade_tok_seq(M, rows, rng):
    """Sequence index per row, ascending, -1 for padding tokens: runs of one-token sequences inside one wave, gaps of padding
    tokens, and sequences that cross 16 / 32 / 64 / 128-row wave and tile boundaries."""
    ts = np.full(rows, -1, np.int32)
    r, s = 0, 0
    lens = [1] * 12 + [37, 5, 100, 1, 1, 70, 140, 3, 9, 200]
    i = 0
    while r < M:
        r += int(rng.integers(0, 4)) if i % 3 == 0 else 0   # padding tokens between some sequences
        n = min(lens[i % len(lens)], M - r)
        if n <= 0:
            break
        ts[r:r + n] = s
        r, s, i = r + n, s + 1, i + 1
    return ts, s


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("M,N,K,small", [(1, 128, 64, -1), (63, 384, 192, -1), (257, 768, 768, -1), (700, 384, 320, 0),
                                         (256, 768, 128, 0)])
def test_splade(M, N, K, small, f16):
    rng = np.random.default_rng(M + N + K + f16)
    rows = -(-M // 256) * 256
    A, W, Af, Wf = operands(rng, M, N, K, f16, sw=1 / math.sqrt(K))
    ts, n_seqs = splade_tok_seq(M, rows, rng)
    if M == 1:
        ts[0], n_seqs = 0, 1
    b = f32(rng.standard_normal(N) * 0.5)
    pre = f32(np.where(rng.uniform(size=(n_seqs, N)) < 0.3, 0, rng.uniform(0, 1.5, (n_seqs, N))))
    sp = pre.view(np.uint32).copy()
    cfg, sat = run(EPI_SPLADE, M, N, K, f16, small_rows=small, n_seqs=n_seqs, A=A, W=W, bias=b, tok_seq=ts, splade_rows=sp)
    assert sat == 0
    acc, e = acc_ref(Af, Wf, np.arange(M))
    got = sp.view(np.float32).astype(np.float64)
    ref = pre.astype(np.float64).copy()
    bound = np.full(ref.shape, 1e-30)
    for s in range(n_seqs):
        m = np.nonzero(ts[:M] == s)[0]
        x = acc[m].max(0) + b
        w = np.log1p(np.maximum(x, 0))
        ref[s] = np.maximum(ref[s], w)
        bound[s] += e[m].max(0) + U * np.abs(x) + 4 * U * w   # log1p(relu(.)) is 1-Lipschitz (and flat below 0)
    record("SPLADE", cfg, f16, got, ref, bound)
    assert np.all(got >= pre)   # the max with the pre-filled contents
    control("SPLADE bias dropped", np.stack([np.maximum(pre[s], np.log1p(np.maximum(acc[ts[:M] == s].max(0), 0)))
                                             for s in range(n_seqs)]), ref, bound)


# ------------------------------------------------------------------ contracts without float64
def _residual_outputs(form, M, N, K, f16, seed, rows, Mrun):
    """One residual launch over the first Mrun rows of a fixed rows-row problem; returns the first M rows of every output."""
    rng = np.random.default_rng(seed)
    A, W, _, _ = operands(rng, rows, N, K, f16, rows=rows, sw=1 / math.sqrt(K))
    h = f32(rng.standard_normal((rows, N)) * 2 + 1)
    hi = to16(h - 1, f16)
    lo = rng.integers(0, 256, rows * N).astype(np.uint8)
    c_prev, c = f32(rng.standard_normal(rows) + 1), f32(rng.standard_normal(rows) + 1)
    st = np.zeros((N // 64, rows, 2), np.float32)
    bias = f32(rng.standard_normal(N) * 0.3)
    kw = {
        "plain": dict(out_f32=h, bias=bias),
        "postln": dict(out_f32=h, bias=bias, res_mu=f32(rng.standard_normal(rows)), res_rstd=f32(rng.uniform(0.5, 2, rows)),
                       res_g=f32(rng.uniform(0.5, 1.5, N)), res_b=f32(rng.standard_normal(N) * 0.1), resid_bf16=hi, stats_part=st),
        "leaves": dict(out_f32=h, resid_bf16=hi, lo_out=lo, ln_shift=c, stats_part=st),
        "both": dict(resid_bf16=hi, lo_in=lo, lo_out=lo, ln_shift_prev=c_prev, ln_shift=c, stats_part=st),
        "arrives": dict(out_f32=h, resid_bf16=hi, lo_in=lo, ln_shift_prev=c_prev),
    }[form]
    cfg, _ = run(EPI_RESIDUAL, Mrun, N, K, f16, rows=rows, A=A, W=W, **kw)
    res = {}
    for n in ("out_f32", "resid_bf16", "stats_part", "lo_out"):
        if n in kw:
            v = kw[n]
            res[n] = v[:, :M].copy() if n == "stats_part" else (v[:M * N].copy() if n == "lo_out" else v[:M].copy())
    return cfg, res


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("form", ["plain", "postln", "leaves", "both", "arrives"])
def test_residual_forms_same_bits(form, f16):
    """The three launch-bound residual forms (K-split, 64 x 64 and 128 x 128 chain-ordered) give the same bits for the same rows:
    64 rows alone take the K-split, inside 1345 rows the 64 x 64 KCH form, inside 2689 rows the 128 x 128 one (N = 768)."""
    N, K, M = 768, 320, 64   # K = 320: five K-steps, chains of unequal length
    rows = 2816
    got = {}
    for Mrun in (64, 1345, 2689):
        cfg, res = _residual_outputs(form, M, N, K, f16, seed=5 + f16, rows=rows, Mrun=Mrun)
        got[cfg] = res
    assert set(got) == {KSPLIT, KCH64, KCH128}
    ref = got[KSPLIT]
    for cfg, res in got.items():
        for n, v in ref.items():
                assert np.array_equal(res[n].view(np.uint8), v.view(np.uint8)), (form, cfg, n)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("form", ["leaves", "both", "arrives"])
def test_split_micro_batches(form, f16):
    """A split residual launch over rows [0, M) gives the bits of two launches over [0, r0) and [r0, M) through offset pointers
    (byte plane at r0 * N bytes, statistics at row r0 of stats_ld), as the encoder addresses its micro-batches.  r0 is a
    multiple of 256: a launch writes whole tiles of its rows rounded up to 256 (micro-batches start on kRowPad rows)."""
    rng = np.random.default_rng(21 + f16)
    M, N, K, r0 = 700, 384, 192, 256
    rows = 1024
    A, W, _, _ = operands(rng, M, N, K, f16, rows=rows, sw=0.05)
    h = f32(rng.standard_normal((rows, N)) * 2 + 1)
    hi0 = to16(h - 1, f16)
    lo0 = rng.integers(0, 256, rows * N).astype(np.uint8)
    c_prev, c = f32(rng.standard_normal(rows) + 1), f32(rng.standard_normal(rows) + 1)

    def launch(parts):
        hi, lo, out = hi0.copy(), lo0.copy(), h.copy()
        st = np.zeros((N // 64, rows, 2), np.float32)
        kw = dict(A=A, W=W, resid_bf16=hi)
        if form in ("leaves", "both"):
            kw.update(lo_out=lo, ln_shift=c, stats_part=st)
        if form in ("arrives", "both"):
            kw.update(lo_in=lo, ln_shift_prev=c_prev)
        if form != "both":
            kw["out_f32"] = out
        for a, b in parts:
            run(EPI_RESIDUAL, b - a, N, K, f16, rows=rows, row0=a, **kw)
        return hi[:M], lo.reshape(rows, N)[:M], out[:M], st[:, :M]

    whole, split = launch([(0, M)]), launch([(0, r0), (r0, M)])
    for n, x, y in zip(("resid_bf16", "lo", "out_f32", "stats"), whole, split):
        if n == "lo" and form == "arrives":
            continue
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), n


PAD_CASES = ["F32", "BF16 fold+finalize", "RESIDUAL stats", "RESIDUAL split", "GEGLU fold", "QKV fold", "SPLADE"]


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("small", [-1, 0])
@pytest.mark.parametrize("kind", PAD_CASES)
def test_padding_rows_do_not_leak(kind, small, f16):
    """Rows [M, Mpad) of A hold large finite values instead of zeros: every valid output is bit-identical to the zero-padded run
    (statistics, SPLADE rows and the finalised LayerNorm rows included)."""
    M, K = 200 if small < 0 else 300, 128
    rows = 512 if M > 256 else 256

    def once(pad):
        rng = np.random.default_rng(31 + f16)
        N = 384
        kw, epi, extra = {}, EPI_F32, {}
        A, W, _, _ = operands(rng, M, N, K, f16, rows=rows, pad=pad)
        if kind == "F32":
            kw = dict(out_f32=np.zeros((rows, N), np.float32), bias=f32(rng.standard_normal(N)))
        elif kind in ("BF16 fold+finalize", "GEGLU fold", "QKV fold"):
            epi = {"BF16 fold+finalize": EPI_BF16, "GEGLU fold": EPI_GEGLU, "QKV fold": EPI_QKV_ROPE}[kind]
            _, c, s, mu, rstd, st = fold_inputs(rng, M, K, N, f16, W, rows, True)
            kw = dict(ln_mu=mu, ln_rstd=rstd, ln_s=s, stats_in=st, ln_shift=c)
            if epi == EPI_BF16:
                kw["out_bf16"] = np.zeros((rows, N), np.uint16)
            elif epi == EPI_GEGLU:
                kw["out_bf16"] = np.zeros((rows, N // 2), np.uint16)
            else:
                H = N // 3
                ang = rng.uniform(0, 6, (8, 32))
                kw.update(q=np.zeros((rows, H), np.uint16), k=np.zeros((rows, H), np.uint16), vt=np.zeros((H, rows), np.uint16),
                          rope_cos=f32(np.cos(ang)), rope_sin=f32(np.sin(ang)), pos=(np.arange(rows) % 8).astype(np.int32))
                extra = dict(hidden=H, rope_rows=8)
        elif kind.startswith("RESIDUAL"):
            epi = EPI_RESIDUAL
            kw = dict(out_f32=f32(rng.standard_normal((rows, N))), ln_shift=f32(rng.standard_normal(rows)),
                      resid_bf16=np.zeros((rows, N), np.uint16), stats_part=np.zeros((N // 64, rows, 2), np.float32))
            if kind == "RESIDUAL split":
                kw.update(lo_out=np.zeros(rows * N, np.uint8))
        else:
            epi = EPI_SPLADE
            ts, n_seqs = splade_tok_seq(M, rows, rng)
            kw = dict(tok_seq=ts, splade_rows=np.zeros((n_seqs, N), np.uint32), bias=f32(rng.standard_normal(N)))
            extra = dict(n_seqs=n_seqs)
        run(epi, M, N, K, f16, rows=rows, small_rows=small, A=A, W=W, **kw, **extra)
        res = {}
        for n, v in kw.items():
            if n in ("out_f32", "out_bf16", "q", "k", "resid_bf16", "ln_mu", "ln_rstd", "ln_shift"):
                res[n] = v[:M].copy()
            elif n == "vt":
                res[n] = v[:, :M].copy()
            elif n == "stats_part":
                res[n] = v[:, :M].copy()
            elif n == "splade_rows":
                res[n] = v.copy()
            elif n == "lo_out":
                res[n] = v.reshape(rows, N)[:192].copy()   # whole 64-row blocks of valid rows
        return res

    zero, big = once(None), once(3.0e4 if f16 else 1.0e8)
    for n in zero:
        assert np.array_equal(zero[n].view(np.uint8), big[n].view(np.uint8)), n


def test_f16_saturation_clamps_and_flags():
    """An fp16 output row built to exceed 65504 comes back as +-65504 (not inf) and raises the flag; a normal run clears it."""
    M, N, K = 64, 128, 64
    A = np.zeros((256, K))
    A[:M] = 0.25
    A[3] = 32.0                   # row 3: 64 x 32 x (+-32) = +-65536
    W = np.full((N, K), 0.25)
    W[: N // 2] = 32.0
    W[N // 2:] = -32.0
    A16, W16 = to16(A, True), to16(W, True)
    out = np.zeros((256, N), np.uint16)
    cfg, sat = run(EPI_BF16, M, N, K, True, A=A16, W=W16, out_bf16=out)
    got = from16(out[:M], True)
    assert sat == 1
    assert np.all(got[3, : N // 2] == 65504) and np.all(got[3, N // 2:] == -65504)
    assert np.all(np.isfinite(got))
    rest = np.delete(np.arange(M), 3)
    assert np.allclose(got[rest], from16(to16((A[:M] @ W.T)[rest], True), True), rtol=0, atol=0)
    out[:] = 0
    _, sat = run(EPI_BF16, M, N, K, True, A=to16(A * (A < 1), True), W=W16, out_bf16=out)
    assert sat == 0


@pytest.mark.parametrize("f16", [False, True])
def test_persistent_walk_all_configs(f16):
    """For every configuration whose grid cap the output tiles can exceed, one launch with more tiles than the cap: a persistent
    workgroup walks several tiles (float64 reference on sampled rows).  The 64 x 64 forms cannot: launch_t takes them for at
    most 512 tiles, under their cap of 1024."""
    assert max(-(-m // 64) * (768 // 64) for m in range(1, 2689) if -(-m // 128) * 6 <= 128) <= 1024
    M, K = 7300, 64
    cases = [(EPI_BF16, 2304, 0, TILE256), (EPI_F32, 1152, 0, TILE128), (EPI_BF16, 1152, BIG_ROWS, SMALL8),
             (EPI_F32, 1152, BIG_ROWS, SMALL4), (EPI_RESIDUAL, 1152, BIG_ROWS, KCH128)]
    for epi, N, small, want in cases:
        rng = np.random.default_rng(N + epi + f16)
        A, W, Af, Wf = operands(rng, M, N, K, f16, sw=0.125)
        rows = A.shape[0]
        assert -(-M // want[0]) * (N // want[1]) > ALL_CONFIGS[want]
        if epi == EPI_BF16:
            out = np.zeros((rows, N), np.uint16)
            cfg, _ = run(epi, M, N, K, f16, small_rows=small, expect=want, A=A, W=W, out_bf16=out)
        else:
            h = f32(rng.standard_normal((rows, N))) if epi == EPI_RESIDUAL else np.zeros((rows, N), np.float32)
            out = h.copy()
            cfg, _ = run(epi, M, N, K, f16, small_rows=small, expect=want, A=A, W=W, out_f32=out)
        rs = sample_rows(M, cfg[0])
        acc, e = acc_ref(Af, Wf, rs)
        if epi == EPI_BF16:
            record("walk BF16", cfg, f16, from16(out[rs], f16), acc, out16_bound(acc, e, f16))
        else:
            ref = acc + (h[rs] if epi == EPI_RESIDUAL else 0)
            record("walk " + ("RESIDUAL" if epi == EPI_RESIDUAL else "F32"), cfg, f16, out[rs], ref, e + 2 * U * np.abs(ref) + 1e-30)


def _boundary(pred, lo, hi):
    """Largest M in [lo, hi] with pred(M) true (pred true at lo, false at hi, monotone)."""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def test_zz_boundaries_and_coverage():
    """Row counts on both sides of every configuration switch of launch_t, computed from its inequalities at the N in use, take
    different configurations; together with the module's other launches every configuration ran for both operand types."""
    N = 768
    b_ksplit = _boundary(lambda m: -(-m // 64) * (N // 64) <= 256, 1, 8192)
    b_kch64 = _boundary(lambda m: -(-m // 128) * (N // 128) <= 128, 1, 8192)
    assert (b_ksplit, b_kch64) == (1344, 2688)
    plan = [(EPI_RESIDUAL, b_ksplit, N, -1), (EPI_RESIDUAL, b_ksplit + 1, N, -1),
            (EPI_RESIDUAL, b_kch64, N, -1), (EPI_RESIDUAL, b_kch64 + 1, N, -1),
            (EPI_BF16, 8192, 256, -1), (EPI_BF16, 8193, 256, -1),
            (EPI_F32, 8192, 256, -1), (EPI_F32, 8193, 256, -1),
            (EPI_F32, 255, 256, 0), (EPI_F32, 256, 256, 0)]
    for f16 in (False, True):
        got = []
        for epi, M, n, small in plan:
            rng = np.random.default_rng(M + n)
            A, W, Af, Wf = operands(rng, M, n, 64, f16, sw=0.125)
            rows = A.shape[0]
            kw = dict(out_f32=np.zeros((rows, n), np.float32)) if epi != EPI_BF16 else dict(out_bf16=np.zeros((rows, n), np.uint16))
            cfg, _ = run(epi, M, n, 64, f16, small_rows=small, A=A, W=W, **kw)
            got.append(cfg)
            # the last and first rows of the launch are computed right on either side of the switch
            rs = np.array([0, M - 1])
            acc, e = acc_ref(Af, Wf, rs)
            o = kw.get("out_f32")
            if o is not None:
                record("boundary", cfg, f16, o[rs], acc, e + 1e-30)
            else:
                record("boundary", cfg, f16, from16(kw["out_bf16"][rs], f16), acc, out16_bound(acc, e, f16))
        for i in range(0, len(plan), 2):
            assert got[i] != got[i + 1], plan[i]
    missing = [(cfg, f16) for cfg in ALL_CONFIGS for f16 in (False, True) if (cfg, f16) not in _SEEN]
    assert not missing, f"configurations that never ran: {missing}"
    assert {c for c, _ in _SEEN} <= set(ALL_CONFIGS), _SEEN
    print("\nworst error / bound per epilogue form, configuration (BM, BN, WM, WN, NS, HW, KCH) and operand type:")
    for (form, cfg, f16), r in sorted(_WORST.items(), key=lambda kv: (kv[0][0], str(kv[0][1]), str(kv[0][2]))):
        print(f"  {form:45s} {str(cfg):32s} {'fp16' if f16 else ('bf16' if f16 is not None else '')} {r:.3g}")
