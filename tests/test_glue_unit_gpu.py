"""The encoder's packing and glue kernels ALONE (vrag_debug_glue_run: the launchers of csrc/glue_kernels.h and permute_qkv_heads)
against numpy references of what their comments say they compute (tests/glue_ref.py), on the SAME fp32 values the kernels read.

Exact checks (array_equal on bits): cvt_rows and cvt_split3 hi = RNE_T(fl32(v * col_scale)) and lo = RNE_T(fl32(v' - float(hi)))
(the subtraction is exact in fp32), the interleave map, zero padding, the fp16 clamp and its word; ln_stats_finalize's shift_prev
and its agreement with the consumer GEMM's finalisation; pack_layout; splade_compact; permute_qkv_heads.  Every output buffer is
pre-filled with a canary and holds EXTRA rows behind what the launch covers: whatever the kernel must not write must come back
as it went in.

Bounded checks.  U = 2^-24, g(n) = n U / (1 - n U) a chain of n roundings, "one ulp" = 2 U relative for a division or a root.
  row_sum  against float64 of the ROUNDED row: ceil(cols / 256) in-lane additions, six shuffle levels, the two LDS adds:
           g(ceil(cols / 256) + 8) sum |hi|.  A row of zeros must give exactly 0.
  d        s1 is np partials added in order: g(np) sum |p1| / H, the division one ulp: E_d = g(np) sum |p1| / H + 2 U |d|.
  var      t1 = s2 / H the same way, E_t1 = g(np) sum |p2| / H + 2 U t1; d~^2 against d^2: 2 |d| E_d + E_d^2 and the product's
           rounding U d^2 (none if fused); the subtraction rounds once: E_var = e + U (|t1 - d^2| + e), e the sum of the terms
           before.  max(., 0) is 1-Lipschitz.  The kernel does not return var: it is read back as rstd^-2 - eps, which costs the
           sum's rounding and the two one-ulp steps, E_var + U s + 9 U (s + E_s), s = var + eps.
  rstd     two-sided against float64, and on the near-constant rows one-sided against eps^-1/2 (check_clamp: the excess over it is
           at most 6 U eps^-1/2 with the clamp, and ~ |var~| / 2 eps without).  var~ + eps rounds once: E_s = E_var + U (s + E_var).  The clamp guarantees var~ >= 0, so var~ + eps >= eps (1 - U)
           whatever E_var is, and rstd~ lies between (s + E_s)^-1/2 (1 - 4 U) and max(s - E_s, eps (1 - U))^-1/2 (1 + 4 U): no
           first-order assumption, so the near-constant rows (E_var ~ var, var ~ 0) are covered: there the upper end IS eps^-1/2.
  shift    c + d~ rounds once: E_d + U |c + d|.

Negative controls (CPU, unmarked): a reference with one named defect must fail its check on a named case; for the bounded checks
by at least 10 x.  Worst ratio on the named case: row_sum over the unrounded row (bf16, every value 1 + 2^-9, cols = 768) 2979,
variance over H - 1 (spread rows, H = 768) 909, shift_out = d 8.7e6, variance without the clamp (constructed rows, H = 768,
against the one-sided check) 3.3e5 fused / 3.1e5 not.  The exact checks' controls count the elements that differ.

`-rP` prints the worst error / bound ratio per bounded check.  Measured on an MI355X: see MEASURED below."""
import ctypes as C
import zlib

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib
import glue_ref as G
from unit16 import U, f32, from16, make_ledger, to16

gpu = pytest.mark.gpu

MEASURED = """NOT MEASURED: no MI355X run of this module has been recorded yet (`-rP` prints the table: the worst error / bound ratio of
row_sum, d, var, rstd and shift per shape and type)."""

EPS = 1e-5
EXTRA = 3                                   # canary rows behind what a launch covers
CAN32 = np.uint32(0x7A5C7A5C)
CAN16 = np.uint16(0x7A5C)
DT = ("bf16", "fp16")
COLS = [1, 63, 256, 257, 768]
_WORST, record, control = make_ledger()
PTRS = {n for n, t in _lib.DebugGlueArgs._fields_ if t is C.c_void_p}
INT_PTRS = {"packed", "seq_row", "seq_src", "seq_len", "ids", "pos", "tok_seq", "counts", "idx"}
ERR_INVALID, ERR_HIP, ERR_NO_DEVICE = -1, -2, -4


# ------------------------------------------------------------------ the hook
def can16(*shape):
    return np.full(shape, CAN16, np.uint16)


def can32(*shape):
    return np.full(shape, CAN32, np.uint32).view(np.float32)


def cani(*shape):
    return np.full(shape, CAN32, np.uint32).view(np.int32)


def is_canary(a):
    a = np.ascontiguousarray(a)
    return bool(np.all(a == CAN16)) if a.dtype == np.uint16 else bool(np.all(a.view(np.uint32) == CAN32))


def raw_run(op, **kw):
    """One call of the hook: arrays go in by struct field name (in / out arrays are updated in place), scalars are fields."""
    a = _lib.DebugGlueArgs()
    keep = []
    for name, v in kw.items():
        if name in PTRS:
            if v is None:
                continue
            assert isinstance(v, np.ndarray) and v.flags.c_contiguous, name
            assert v.dtype == (np.int32 if name in INT_PTRS else np.uint16 if name in ("dst", "dst_lo", "w", "w_out") else np.float32), name
            keep.append(v)
            setattr(a, name, v.ctypes.data)
        else:
            setattr(a, name, v)
    a.op = _lib.DEBUG_GLUE_OPS[op]
    a.f16_saturated = -1
    status = _lib.load_debug().vrag_debug_glue_run(C.byref(a), 0)
    del keep
    return status, a


def run(op, **kw):
    status, a = raw_run(op, **kw)
    if status == ERR_HIP:   # a failed launch or a clobbered canary: nothing more goes onto this device
        msg = _lib.load_debug().vrag_last_error()
        pytest.exit(f"vrag_debug_glue_run: {msg.decode() if msg else status}", returncode=3)
    _lib.check_debug("vrag_debug_glue_run", status)
    return a


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def same16(name, got, want, f16):
    """Bit equality of 16-bit images; where the reference holds a bf16 NaN the kernel's must be a NaN (its payload is free)."""
    want_nan = np.isnan(from16(want, f16))
    assert np.array_equal(np.isnan(from16(got, f16)), want_nan), f"{name}: NaN positions differ"
    bad = np.argwhere((got != want) & ~want_nan)
    assert bad.size == 0, f"{name}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]:#06x} want {want[tuple(bad[0])]:#06x}"


# ------------------------------------------------------------------ cvt_rows / cvt_split3
def family_rows(rng, cols, f16):
    """fp32 rows, one data family each: unit normal; halfway points of the type (ties to even); large normal; fp16: subnormal
    results and the ties at 2^-25 / bf16: halfway points again; +-0; small normal."""
    zeros = np.where(np.arange(cols) % 2 == 0, 0.0, -0.0)
    return f32(np.stack([rng.standard_normal(cols), G.halfway_values(rng, cols, f16), 100.0 * rng.standard_normal(cols),
                         G.f16_small_values(rng, cols) if f16 else G.halfway_values(rng, cols, f16), zeros,
                         1e-3 * rng.standard_normal(cols)]))


def cvt_launch(src, rows_dst, f16, I=0, col_scale=None, lo=True, row_sum=True):
    cols, out_rows = src.shape[1], rows_dst + EXTRA
    dst, dst_lo, rs = can16(out_rows, cols), (can16(out_rows, cols) if lo else None), (can32(out_rows) if row_sum else None)
    a = run("cvt_rows", src=src, col_scale=col_scale, dst=dst, dst_lo=dst_lo, row_sum=rs, rows_dst=rows_dst, rows_src=src.shape[0],
            cols=cols, interleave=int(I > 0), I=I, out_rows=out_rows, f16=int(f16))
    for name, o in (("dst", dst), ("dst_lo", dst_lo), ("row_sum", rs)):
        assert o is None or is_canary(o[rows_dst:]), f"{name}: rows at or beyond rows_dst were written"
    return dst[:rows_dst], (dst_lo[:rows_dst] if lo else None), (rs[:rows_dst] if row_sum else None), a.f16_saturated


def check_cvt(tag, src, rows_dst, f16, I=0, col_scale=None, lo=True, finite=True):
    hi, lo_bits, rs, sat = cvt_launch(src, rows_dst, f16, I, col_scale, lo)
    ref = G.cvt_rows(src, rows_dst, f16, I, col_scale)
    same16(tag + " hi", hi, ref["hi"], f16)
    if lo:
        same16(tag + " lo", lo_bits, ref["lo"], f16)
    assert sat == int(ref["sat"]), f"{tag}: clamp word {sat}, expected {int(ref['sat'])}"
    if finite:
        live = ref["row_abs"] > 0
        assert np.all(bits(rs[~live]) << 1 == 0), f"{tag}: the sum of a zero row must be exactly 0"
        if live.any():
            record("row_sum", src.shape[1], f16, rs[live], ref["row_sum"][live], G.row_sum_bound(src.shape[1], ref["row_abs"][live]))
    return hi, lo_bits, rs


@gpu
@pytest.mark.parametrize("f16", (False, True), ids=DT)
@pytest.mark.parametrize("cols", COLS)
def test_cvt_rows(cols, f16):
    rng = rng_for("cvt", cols, f16)
    src = family_rows(rng, cols, f16)
    n = src.shape[0]
    scale = f32(1.0 + 0.5 * rng.standard_normal(cols))
    for rows_dst in (n, n + 3):
        hi, lo, rs = check_cvt(f"cvt_rows cols={cols} rows_dst={rows_dst}", src, rows_dst, f16)
        assert not hi[n:].any() and not lo[n:].any(), "rows beyond rows_src must be zero bits"
        hi, lo, rs = check_cvt(f"cvt_rows*scale cols={cols} rows_dst={rows_dst}", src, rows_dst, f16, col_scale=scale)
        assert np.all(from16(hi[n:], f16) == 0) and np.all(from16(lo[n:], f16) == 0) and np.all(rs[n:] == 0)
    check_cvt(f"cvt_rows no lo cols={cols}", src, n, f16, lo=False)


RANGE_CASES = [  # name, values, clamp word
    ("in range", [65504.0, -65504.0, 1.0, 0.0], 0), ("65536", [65536.0, 1.0], 1), ("7e4", [7e4, 1.0], 1), ("-1e6", [1.0, -1e6], 1),
    ("+inf", [np.inf, 2.0], 1), ("-inf", [3.0, -np.inf], 1), ("nan", [np.nan, 1.0], 1), ("65504 + 1 ulp32", [65504.004, 1.0], 1)]


def range_src(values, cols):
    src = np.ones((2, cols), np.float32)
    src[1, -len(values):] = f32(values)      # the last columns: the last stride of the loop
    return src


@gpu
@pytest.mark.parametrize("op", ("cvt_rows", "cvt_split3"))
def test_fp16_range_is_pinned(op):
    """common.h: 65504 is stored and not flagged; anything above is stored as +-65504 and flagged; NaN as -65504 and flagged."""
    for cols in (63, 257):
        for name, values, word in RANGE_CASES:
            src = range_src(values, cols)
            if op == "cvt_rows":
                hi, lo, _ = check_cvt(f"fp16 {name}", src, 2, True, finite=False)
                sat = int(G.cvt_rows(src, 2, True)["sat"])
            else:
                img, sat = split3_check(f"fp16 {name}", src, 2, True)
                hi = img[:, :cols]
            assert sat == word, name
            want = np.clip(np.nan_to_num(f32(values), nan=-65504.0, posinf=65504.0, neginf=-65504.0), -65504.0, 65504.0)
            assert from16(hi[1, -len(values):], True).tolist() == want.tolist(), name


@gpu
@pytest.mark.parametrize("op", ("cvt_rows", "cvt_split3"))
def test_bf16_keeps_inf_and_nan(op):
    src = range_src([np.inf, -np.inf, np.nan, 3.0e38, -1.0], 257)
    if op == "cvt_rows":
        hi, _, _ = check_cvt("bf16 inf nan", src, 2, False, finite=False)
    else:
        hi = split3_check("bf16 inf nan", src, 2, False)[0][:, :257]
    v = from16(hi[1, -5:], False)
    assert v[0] == np.inf and v[1] == -np.inf and np.isnan(v[2]) and np.isfinite(v[3]) and v[4] == -1.0


@gpu
@pytest.mark.parametrize("f16", (False, True), ids=DT)
@pytest.mark.parametrize("I", (32, 40, 96, 100))
def test_cvt_rows_interleave(I, f16):
    """The Wi form: GeGLU interleave with the folded gain and the row sums, rows_dst as the encoder pads it."""
    rng = rng_for("interleave", I, f16)
    cols = 257
    src = f32(rng.standard_normal((2 * I, cols)))
    scale = f32(1.0 + 0.5 * rng.standard_normal(cols))
    base = 64 * -(-I // 32)
    for rows_dst in (base, -(-base // 256) * 256):
        hi, _, rs = check_cvt(f"interleave I={I} rows_dst={rows_dst}", src, rows_dst, f16, I=I, col_scale=scale, lo=False)
        r = np.arange(rows_dst)
        pad = (r >> 6) * 32 + (r & 31) >= I
        assert pad.sum() == rows_dst - 2 * I
        assert np.all(from16(hi[pad], f16) == 0) and np.all(rs[pad] == 0), "rows with f >= I must be zero"
        assert np.all(np.abs(from16(hi[~pad], f16)).sum(1) > 0)


def split3_check(tag, src, rows_dst, f16):
    cols, out_rows = src.shape[1], rows_dst + EXTRA
    dst = can16(out_rows, 3 * cols)
    a = run("cvt_split3", src=src, dst=dst, rows_dst=rows_dst, rows_src=src.shape[0], cols=cols, out_rows=out_rows, f16=int(f16))
    assert is_canary(dst[rows_dst:]), "cvt_split3: rows at or beyond rows_dst were written"
    ref, sat = G.cvt_split3(src, rows_dst, f16)
    same16(tag, dst[:rows_dst], ref, f16)
    assert a.f16_saturated == int(sat)
    return dst[:rows_dst], a.f16_saturated


@gpu
@pytest.mark.parametrize("f16", (False, True), ids=DT)
@pytest.mark.parametrize("cols", COLS)
def test_cvt_split3(cols, f16):
    src = family_rows(rng_for("split3", cols, f16), cols, f16)
    n = src.shape[0]
    for rows_dst in (n, n + 3):
        img, sat = split3_check(f"cvt_split3 cols={cols} rows_dst={rows_dst}", src, rows_dst, f16)
        assert sat == 0 and not img[n:].any(), "rows at and beyond rows_src must be zero bits"
        assert np.array_equal(img[:, :cols], img[:, cols:2 * cols])


# ------------------------------------------------------------------ ln_stats_finalize
FIN_H = [64, 128, 768, 1024]
FIN_ROWS = [1, 255, 256, 257]
FAMILIES = ["spread", "mean", "const"]


def negative_variance_rows(rng, rows, H):
    """Near-constant rows whose fp32  s2 / H - d^2  is NEGATIVE before the clamp, fused or not: drawn, then selected by running
    the kernel's fp32 arithmetic on the CPU (glue_ref.finalize_f32)."""
    parts, shifts, have = [], [], 0
    for _ in range(64):
        st, c = G.stats_rows(rng, "const", 8 * rows + 64, H)
        neg = (G.finalize_f32(st, H, EPS, True)[1] < 0) & (G.finalize_f32(st, H, EPS, False)[1] < 0)
        parts.append(st[:, neg])
        shifts.append(c[neg])
        have += int(neg.sum())
        if have >= rows:
            break
    st, c = np.concatenate(parts, 1)[:, :rows], np.concatenate(shifts)[:rows]
    assert st.shape[1] == rows, f"only {st.shape[1]} of {rows} rows with a negative fp32 variance"
    return np.ascontiguousarray(st), c


def fin_inputs(family, rows, H, seed=0):
    rng = rng_for("fin", family, rows, H, seed)
    return negative_variance_rows(rng, rows, H) if family == "const" else G.stats_rows(rng, family, rows, H)


def fin_launch(st, c, H, row0, ld, shift_mode, with_prev):
    """shift_mode: null / given / alias.  Returns the four outputs as [ld] arrays (prev may be None)."""
    n, rows = st.shape[0], st.shape[1]
    rng = rng_for("fin pad", rows, H, row0)
    part = f32(rng.standard_normal((n, ld, 2)) * 100.0)       # rows outside [row0, row0 + rows): never read
    part[:, row0:row0 + rows] = st
    mu, rstd, out, prev = can32(ld), can32(ld), can32(ld), (can32(ld) if with_prev else None)
    shift_in = None
    if shift_mode == "given":
        shift_in = f32(rng.standard_normal(ld))
        shift_in[row0:row0 + rows] = c
    elif shift_mode == "alias":
        out[row0:row0 + rows] = c
    run("ln_stats_finalize", part=part, mu=mu, rstd=rstd, shift_in=shift_in, shift_out=out, shift_prev=prev, rows=rows, ld=ld, row0=row0,
        H=H, np=n, alias_shift=int(shift_mode == "alias"), eps=EPS)
    for name, o in (("mu", mu), ("rstd", rstd), ("shift_out", out), ("shift_prev", prev)):
        if o is not None:
            assert is_canary(o[:row0]) and is_canary(o[row0 + rows:]), f"{name}: rows outside [row0, row0 + rows) were written"
    sl = slice(row0, row0 + rows)
    return mu[sl], rstd[sl], out[sl], (prev[sl] if with_prev else None)


def check_finalize(tag, H, st, c_used, mu, rstd, out, prev):
    d, var, r, shift, c = G.finalize(st, H, EPS, c_used)
    e_d, e_var, e_r, e_shift = G.finalize_bounds(st, H, EPS, c_used)
    assert np.all(np.isfinite(rstd)) and np.all(rstd > 0)
    record("d", H, None, mu, d, e_d)
    record("rstd", H, None, rstd, r, e_r)
    record("shift", H, None, out, shift, e_shift)
    epsf = float(np.float32(EPS))
    s = var + epsf
    e_s = e_var + U * (s + e_var)
    record("var (rstd^-2 - eps)", H, None, rstd.astype(np.float64) ** -2 - epsf, var, e_var + U * s + 9 * U * (s + e_s))
    if prev is not None:
        assert np.array_equal(bits(prev), bits(f32(c))), f"{tag}: shift_prev must be the incoming shift, bit for bit"


def check_clamp(H, rstd, rec=record):
    """The clamp, one-sided: var~ >= 0 puts var~ + eps at eps (1 - U) or above (the sum rounds), the root and the reciprocal are
    one ulp each: rstd~ <= eps^-1/2 (1 - U)^-1/2 (1 + 4 U) < eps^-1/2 (1 + 6 U).  Judged as the excess over eps^-1/2."""
    top = float(np.float32(EPS)) ** -0.5
    return rec("rstd over eps^-1/2 (clamp)", H, None, np.maximum(np.asarray(rstd, np.float64), top), np.full(len(rstd), top), 6 * U * top)


@gpu
@pytest.mark.parametrize("rows", FIN_ROWS)
@pytest.mark.parametrize("H", FIN_H)
def test_ln_stats_finalize(H, rows):
    i = 0
    for family in FAMILIES:
        st, c = fin_inputs(family, rows, H)
        for shift_mode in ("null", "given", "alias"):
            row0, with_prev = (0, 8)[i % 2], (i // 2) % 2 == 0       # over the nine launches: every value with every family
            i += 1
            mu, rstd, out, prev = fin_launch(st, c, H, row0, row0 + rows + 5, shift_mode, with_prev)
            check_finalize(f"finalize {family} {shift_mode} H={H} rows={rows}", H, st, None if shift_mode == "null" else c, mu, rstd, out, prev)
            if family == "const":
                check_clamp(H, rstd)


@gpu
@pytest.mark.parametrize("n", (2, 12, 16))
def test_finalize_kernel_and_consumer_gemm_write_the_same_bits(n):
    """gemm_bf16.hip claims its small-row consumer path finishes the statistics with "the same bits" as the finalize kernel."""
    K, N, M, rows = 64 * n, 128, 255, 256
    for family in FAMILIES:
        st_m, c_m = fin_inputs(family, M, K, seed=1)
        st = np.zeros((n, rows, 2), np.float32)
        st[:, :M] = st_m
        c = f32(np.zeros(rows))
        c[:M] = c_m
        rng = rng_for("same bits", n, family)
        g = _lib.DebugGemmArgs()
        A, W = to16(rng.standard_normal((rows, K)), False), to16(rng.standard_normal((N, K)) / 8, False)
        ls = f32(from16(W, False).sum(1))
        mu_g, rstd_g, shift_g, prev_g = f32(np.zeros(rows)), f32(np.ones(rows)), c.copy(), f32(np.full(rows, 7.0))
        out = np.zeros((rows, N), np.uint16)
        for name, arr in dict(A=A, W=W, ln_s=ls, stats_in=st, ln_mu=mu_g, ln_rstd=rstd_g, ln_shift=shift_g, ln_shift_prev=prev_g,
                              out_bf16=out).items():
            setattr(g, name, arr.ctypes.data)
        g.epi, g.M, g.N, g.K, g.rows, g.small_rows, g.fin_eps, g.q_scale = 1, M, N, K, rows, -1, EPS, 1.0     # EPI_BF16
        status = _lib.load_debug().vrag_debug_gemm_run(C.byref(g), 0)
        if status == ERR_HIP:
            pytest.exit("vrag_debug_gemm_run failed", returncode=3)
        _lib.check_debug("vrag_debug_gemm_run", status)
        assert tuple(g.config)[:2] == (128, 128) and tuple(g.config)[2] == 4, "not the small-row configuration"
        mu, rstd, shift, prev = fin_launch(st_m, c_m, K, 0, rows, "given", True)
        for name, a, b in (("ln_mu", mu, mu_g), ("ln_rstd", rstd, rstd_g), ("ln_shift", shift, shift_g), ("ln_shift_prev", prev, prev_g)):
            assert np.array_equal(bits(a), bits(b[:M])), f"{name} ({family}, np = {n}): the finalize kernel and the GEMM differ"


# ------------------------------------------------------------------ pack_layout
PAD_ID = 60001


def pack_case(n_seqs, seed=0):
    """Sequences at 8-aligned rows with alignment gaps, the first past row 0, one 256-aligned jump (a micro-batch boundary),
    lengths that include 1 and 8 k +- 1, ids stored in another order than the rows, fill_to beyond the last sequence."""
    rng = rng_for("pack", n_seqs, seed)
    pool = [1, 7, 9, 15, 17, 8, 63, 65, 31, 33, 16, 23, 25, 2, 64]
    lens = [pool[i % len(pool)] for i in range(n_seqs)]
    seq_row, r = [], 8
    for i, n in enumerate(lens):
        if n_seqs > 1 and i == (n_seqs + 1) // 2:
            r = -(-r // 256) * 256 + (256 if r % 256 == 0 else 0)
        seq_row.append(r)
        r = -(-(r + n) // 8) * 8 + (8 if i % 3 == 2 else 0)
    rows = seq_row[-1] + lens[-1] + 301
    rows += int(rows % 256 == 0)
    order = rng.permutation(n_seqs)
    seq_src, at = np.zeros(n_seqs, np.int32), 5
    for s in order:
        seq_src[s] = at
        at += lens[s] + int(rng.integers(0, 4))
    packed = rng.integers(0, 50000, at + 3).astype(np.int32)
    return packed, np.asarray(seq_row, np.int32), seq_src, np.asarray(lens, np.int32), rows


@gpu
@pytest.mark.parametrize("n_seqs", (1, 2, 3, 64))
def test_pack_layout(n_seqs):
    packed, seq_row, seq_src, seq_len, rows = pack_case(n_seqs)
    assert PAD_ID not in packed
    out_rows = rows + EXTRA
    ids, pos, tok = cani(out_rows), cani(out_rows), cani(out_rows)
    run("pack_layout", packed=packed, seq_row=seq_row, seq_src=seq_src, seq_len=seq_len, ids=ids, pos=pos, tok_seq=tok, n_seqs=n_seqs,
        n_packed=len(packed), rows=rows, out_rows=out_rows, pad_id=PAD_ID)
    want = G.pack_layout(packed, seq_row, seq_src, seq_len, rows, PAD_ID)
    for name, got, w in zip(("ids", "pos", "tok_seq"), (ids, pos, tok), want):
        assert np.array_equal(got[:rows], w), f"{name}: first difference at row {int(np.argmax(got[:rows] != w))}"
        assert is_canary(got[rows:]), f"{name}: rows behind `rows` were written"
    assert (tok[:rows] == -1).sum() == rows - seq_len.sum() and (ids[:seq_row[0]] == PAD_ID).all()


# ------------------------------------------------------------------ splade_compact
VS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1028, 30522, 50368]


def splade_rows(rng, V, ld, n_rows, thr):
    """Row 0 (of 3): every entry survives; row 1: all zero; the last row: mixed -- entries equal to thr (strict >), -0.0, the
    last entry a survivor.  The padding [V, ld) holds LARGE positive values: a lost mask becomes extra hits."""
    x = np.full((n_rows, ld), 1e30, np.float32)
    mixed = np.maximum(rng.standard_normal(V) - 0.5, 0.0)
    mixed[rng.integers(0, V, max(V // 16, 1))] = thr
    mixed[rng.integers(0, V, max(V // 16, 1))] = -0.0
    mixed[rng.integers(0, V, max(V // 64, 1))] = np.nextafter(np.float32(thr), np.float32(1))
    mixed[V - 1] = 1.0
    if V > 1:
        mixed[0] = thr
    if V > 2:
        mixed[1] = -0.0
    x[-1, :V] = mixed
    if n_rows == 3:
        x[0, :V] = rng.uniform(1.0, 2.0, V)
        x[1, :V] = 0.0
    return x


def compact_launch(x, V, thr, cap):
    n, out_rows = x.shape[0], x.shape[0] + EXTRA
    counts, idx, val = cani(out_rows), cani(out_rows, cap), can32(out_rows, cap)
    run("splade_compact", src=x, counts=counts, idx=idx, val=val, rows=n, out_rows=out_rows, V=V, ld=x.shape[1], thr=thr, cap=cap)
    assert is_canary(counts[n:]) and is_canary(idx[n:]) and is_canary(val[n:]), "rows behind the launch were written"
    return counts[:n], idx[:n], val[:n]


def check_compact(tag, x, V, thr, cap):
    counts, idx, val = compact_launch(x, V, thr, cap)
    want_n, want_i, want_v = G.splade_compact(x, V, thr, 1 << 30)
    assert np.array_equal(counts, want_n), f"{tag}: counts {counts} expected {want_n} (the total, stored or not)"
    for s in range(x.shape[0]):
        k = min(int(want_n[s]), cap)
        assert np.array_equal(idx[s, :k], want_i[s][:k]), f"{tag}: row {s} indices"
        assert np.array_equal(bits(val[s, :k]), bits(want_v[s][:k])), f"{tag}: row {s} values"
        assert is_canary(idx[s, k:]) and is_canary(val[s, k:]), f"{tag}: row {s}: slots behind its {k} pairs were written"


@gpu
@pytest.mark.parametrize("V", VS)
def test_splade_compact(V):
    for ld in sorted({-(-V // 4) * 4, -(-V // 256) * 256}):
        for n_rows in (1, 3):
            for thr in (0.0, 0.25):
                x = splade_rows(rng_for("splade", V, ld, n_rows, thr), V, ld, n_rows, thr)
                total = int(G.splade_compact(x, V, thr, 1 << 30)[0].max())
                assert total == (V if n_rows == 3 else total) and total >= 1
                check_compact(f"V={V} ld={ld} rows={n_rows} thr={thr} cap=count", x, V, thr, total)
                if total >= 2:      # overflow: the fullest row (row 0 of three: the next row's slots follow it) loses its last pair
                    check_compact(f"V={V} ld={ld} rows={n_rows} thr={thr} cap=count-1", x, V, thr, total - 1)


# ------------------------------------------------------------------ permute_qkv_heads
@gpu
@pytest.mark.parametrize("with_s", (False, True), ids=("no sums", "sums"))
@pytest.mark.parametrize("H", (64, 128, 320, 768))
def test_permute_qkv_heads(H, with_s):
    rng = rng_for("permute", H, with_s)
    w = rng.integers(0, 1 << 16, (3 * H, H)).astype(np.uint16)          # every bit pattern: the kernel moves rows, no arithmetic
    s = f32(rng.standard_normal(3 * H)) if with_s else None
    out_rows = 3 * H + EXTRA
    w_out, s_out = can16(out_rows, H), (can32(out_rows) if with_s else None)
    run("permute_qkv_heads", w=w, s=s, w_out=w_out, s_out=s_out, H=H, nh=H // 64, out_rows=out_rows)
    want_w, want_s = G.permute_qkv_heads(w, s, H)
    assert np.array_equal(w_out[:3 * H], want_w) and is_canary(w_out[3 * H:])
    if with_s:
        assert np.array_equal(bits(s_out[:3 * H]), bits(want_s)) and is_canary(s_out[3 * H:])


# ------------------------------------------------------------------ the hook's refusals (no launch: runs without a device too)
def refusal_cases():
    f = lambda *s: np.zeros(s, np.float32)
    i32 = lambda *v: np.asarray(v, np.int32)
    cvt = dict(src=f(4, 8), dst=can16(7, 8), dst_lo=can16(7, 8), row_sum=can32(7), rows_dst=4, rows_src=4, cols=8, out_rows=7)
    sp3 = dict(src=f(4, 8), dst=can16(7, 24), rows_dst=4, rows_src=4, cols=8, out_rows=7)
    fin = dict(part=f(2, 12, 2), mu=can32(12), rstd=can32(12), shift_out=can32(12), shift_prev=can32(12), rows=4, ld=12, row0=8, H=128, np=2,
               eps=EPS)
    pack = dict(packed=i32(*range(40)), seq_row=i32(8, 16), seq_src=i32(20, 0), seq_len=i32(7, 9), ids=cani(35), pos=cani(35),
                tok_seq=cani(35), n_seqs=2, n_packed=40, rows=32, out_rows=35, pad_id=PAD_ID)
    comp = dict(src=f(2, 8), counts=cani(5), idx=cani(5, 4), val=can32(5, 4), rows=2, out_rows=5, V=6, ld=8, thr=0.0, cap=4)
    perm = dict(w=np.zeros((384, 128), np.uint16), s=f(384), w_out=can16(387, 128), s_out=can32(387), H=128, nh=2, out_rows=387)
    base = {"cvt_rows": cvt, "cvt_split3": sp3, "ln_stats_finalize": fin, "pack_layout": pack, "splade_compact": comp,
            "permute_qkv_heads": perm}
    bad = [("cvt_rows", dict(src=None), "needs src"), ("cvt_rows", dict(dst=None), "needs src"), ("cvt_rows", dict(rows_src=0), "rows_src"),
           ("cvt_rows", dict(cols=0), "cols"), ("cvt_rows", dict(cols=-8), "cols"), ("cvt_rows", dict(rows_dst=0), "rows_dst"),
           ("cvt_rows", dict(interleave=1, I=0), "I (0)"), ("cvt_rows", dict(interleave=1, I=-32), "I (-32)"),
           ("cvt_rows", dict(out_rows=3), "out_rows"),
           ("cvt_split3", dict(src=None), "needs src"), ("cvt_split3", dict(dst=None), "needs src"), ("cvt_split3", dict(rows_src=-1), "rows_src"),
           ("cvt_split3", dict(cols=0), "cols"), ("cvt_split3", dict(out_rows=3), "out_rows"),
           ("ln_stats_finalize", dict(part=None), "needs part"), ("ln_stats_finalize", dict(mu=None), "needs part"),
           ("ln_stats_finalize", dict(rstd=None), "needs part"), ("ln_stats_finalize", dict(shift_out=None), "needs part"),
           ("ln_stats_finalize", dict(np=3), "np (3) * 64"), ("ln_stats_finalize", dict(H=130), "np (2) * 64"),
           ("ln_stats_finalize", dict(ld=11), "ld (11) below row0 + rows"), ("ln_stats_finalize", dict(row0=9), "below row0 + rows"),
           ("ln_stats_finalize", dict(rows=0), "rows (0)"), ("ln_stats_finalize", dict(alias_shift=1, shift_in=f(12)), "alias_shift"),
           ("pack_layout", dict(packed=None), "needs packed"), ("pack_layout", dict(seq_row=None), "needs packed"),
           ("pack_layout", dict(seq_src=None), "needs packed"), ("pack_layout", dict(seq_len=None), "needs packed"),
           ("pack_layout", dict(ids=None), "needs packed"), ("pack_layout", dict(pos=None), "needs packed"),
           ("pack_layout", dict(tok_seq=None), "needs packed"), ("pack_layout", dict(n_seqs=0), "n_seqs"),
           ("pack_layout", dict(seq_row=i32(16, 8)), "not ascending"), ("pack_layout", dict(seq_row=i32(8, 8)), "not ascending"),
           ("pack_layout", dict(seq_row=i32(8, 24)), "runs past rows"), ("pack_layout", dict(seq_len=i32(7, 17)), "runs past rows"),
           ("pack_layout", dict(seq_src=i32(34, 0)), "beyond the 40 packed ids"), ("pack_layout", dict(seq_src=i32(-1, 0)), "beyond the 40 packed ids"),
           ("pack_layout", dict(n_packed=20), "beyond the 20 packed ids"), ("pack_layout", dict(out_rows=31), "out_rows"),
           ("splade_compact", dict(src=None), "needs src"), ("splade_compact", dict(counts=None), "needs src"),
           ("splade_compact", dict(idx=None), "needs src"), ("splade_compact", dict(val=None), "needs src"),
           ("splade_compact", dict(V=0), "V (0)"), ("splade_compact", dict(V=9), "ld (8)"), ("splade_compact", dict(ld=4), "ld (4)"),
           ("splade_compact", dict(V=5, ld=6), "ld (6)"), ("splade_compact", dict(cap=0), "cap (0)"), ("splade_compact", dict(out_rows=1), "out_rows"),
           ("permute_qkv_heads", dict(w=None), "needs w"), ("permute_qkv_heads", dict(w_out=None), "needs w"),
           ("permute_qkv_heads", dict(s_out=None), "come together"), ("permute_qkv_heads", dict(H=96), "H (96)"),
           ("permute_qkv_heads", dict(nh=3), "64 * nh (3)"), ("permute_qkv_heads", dict(out_rows=383), "out_rows")]
    return base, bad


def test_hook_refusals_launch_nothing():
    """Everything that would address outside the hook's buffers is refused with its own message before a launch: the outputs
    still hold their canary.  The accepted base call of each op is not refused (without a device it stops at the device check)."""
    dbg = _lib.load_debug()
    have_gpu = _lib.load().vrag_device_count() > 0
    base, bad = refusal_cases()
    for op, change, needle in bad:
        kw = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in refusal_cases()[0][op].items()}
        kw.update(change)
        status, _ = raw_run(op, **kw)
        msg = (dbg.vrag_last_error() or b"").decode()
        assert status == ERR_INVALID and needle in msg, (op, change, status, msg)
        for name, v in kw.items():
            if isinstance(v, np.ndarray) and name in ("dst", "dst_lo", "row_sum", "mu", "rstd", "shift_out", "shift_prev", "ids", "pos",
                                                      "tok_seq", "counts", "idx", "val", "w_out", "s_out"):
                assert is_canary(v), f"{op} {change}: {name} was written by a refused call"
    for op, kw in base.items():
        status, _ = raw_run(op, **kw)
        if status == ERR_HIP:
            pytest.exit(f"vrag_debug_glue_run: {(dbg.vrag_last_error() or b'').decode()}", returncode=3)
        assert status == (0 if have_gpu else ERR_NO_DEVICE), (op, status, (dbg.vrag_last_error() or b"").decode())
    a = _lib.DebugGlueArgs()
    a.op = 6
    assert dbg.vrag_debug_glue_run(C.byref(a), 0) == ERR_INVALID and dbg.vrag_debug_glue_run(None, 0) == ERR_INVALID


# ------------------------------------------------------------------ CPU: the references check themselves
@pytest.mark.parametrize("name", G.SELF_CHECKS)
def test_glue_ref_self_check(name):
    getattr(G, name)()


@pytest.mark.parametrize("H", FIN_H)
def test_negative_variance_rows_are_negative_in_fp32(H):
    """The construction the GPU test relies on: before the clamp the kernel's own fp32 arithmetic, fused or not, goes negative on
    every row, the float64 variance of the same partials is ~0, and the bound still ends at eps^-1/2."""
    st, c = fin_inputs("const", 257, H)
    for fused in (True, False):
        d, pre, rstd = G.finalize_f32(st, H, EPS, fused)
        assert np.all(pre < 0) and np.all(np.isfinite(rstd))
        _, _, r, _, _ = G.finalize(st, H, EPS, c)
        assert np.all(np.abs(rstd - r) <= G.finalize_bounds(st, H, EPS, c)[2])
        check_clamp(H, rstd, rec=lambda *a: record(a[0] + " [CPU restatement]", *a[1:]))


def test_fp32_emulation_stays_inside_the_bounds():
    """The bounds admit the kernel's arithmetic as written (CPU restatement, both contraction choices), on every family."""
    for H in FIN_H:
        for family in FAMILIES:
            st, c = fin_inputs(family, 64, H)
            d64, _, r64, shift64, _ = G.finalize(st, H, EPS, c)
            e_d, _, e_r, e_shift = G.finalize_bounds(st, H, EPS, c)
            for fused in (True, False):
                d, _, rstd = G.finalize_f32(st, H, EPS, fused)
                assert np.all(np.abs(d - d64) <= e_d) and np.all(np.abs(rstd - r64) <= e_r)
                assert np.all(np.abs((c + d).astype(np.float32) - shift64) <= e_shift)


# ------------------------------------------------------------------ CPU: negative controls
def differ(a, b):
    return int(np.count_nonzero(np.asarray(a) != np.asarray(b)))


def test_cvt_controls():
    cols = 768
    src = np.full((4, cols), 1.0 + 2.0 ** -9, np.float32)
    ref = G.cvt_rows(src, 4, False)
    assert np.all(from16(ref["hi"], False) == 1.0)
    control("row_sum over the unrounded row (bf16, every value 1 + 2^-9, cols = 768)", G.cvt_rows(src, 4, False, defect="sum_unrounded")["row_sum"],
            ref["row_sum"], G.row_sum_bound(cols, ref["row_abs"]), need=1000.0)
    rng = rng_for("controls")
    scale = f32(1.0 + 0.5 * rng.standard_normal(257))
    for f16 in (False, True):
        src = family_rows(rng, 257, f16)
        ref = G.cvt_rows(src, 9, f16, col_scale=scale)
        assert differ(G.cvt_rows(src, 9, f16, col_scale=scale, defect="hi_trunc")["hi"], ref["hi"]) > 257          # hi truncated
        assert differ(G.cvt_rows(src, 9, f16, col_scale=scale, defect="lo_unscaled")["lo"], ref["lo"]) > 257       # lo from the unscaled value
        assert differ(G.cvt_rows(src, 9, f16, col_scale=scale, defect="pad_row0")["hi"][6:], ref["hi"][6:]) > 257  # padded rows copied from row 0
        assert differ(G.cvt_split3(src, 9, f16, "hi_trunc")[0], G.cvt_split3(src, 9, f16)[0]) > 257
        assert differ(G.cvt_split3(src, 9, f16, "order_hi_lo_hi")[0], G.cvt_split3(src, 9, f16)[0]) > 257
        # the halfway row alone separates truncation from rounding on about half of its entries, and nothing else would
        tie = src[1:2]
        assert 0.3 < differ(G.cvt_rows(tie, 1, f16, defect="hi_trunc")["hi"], G.cvt_rows(tie, 1, f16)["hi"]) / 257 < 0.7
    # interleave with f = g * 64 + w: the x1 half of the first group is still right, the second group is not: the case is I = 40
    src = f32(rng.standard_normal((80, 63)))
    assert differ(G.cvt_rows(src, 128, False, I=40, defect="f_g64")["hi"][:32], G.cvt_rows(src, 128, False, I=40)["hi"][:32]) == 0
    assert differ(G.cvt_rows(src, 128, False, I=40, defect="f_g64")["hi"][64:], G.cvt_rows(src, 128, False, I=40)["hi"][64:]) > 8 * 63


def test_finalize_controls():
    H = 768
    st, c = fin_inputs("spread", 64, H)
    _, _, r, shift, _ = G.finalize(st, H, EPS, c)
    _, _, e_r, e_shift = G.finalize_bounds(st, H, EPS, c)
    control("variance over H - 1 (spread rows, H = 768)", G.finalize(st, H, EPS, c, "var_H-1")[2], r, e_r, need=100.0)
    control("shift_out = d (spread rows, H = 768)", G.finalize(st, H, EPS, c, "shift_is_d")[3], shift, e_shift, need=1000.0)
    # without the clamp the constructed rows overshoot eps^-1/2: the two-sided bound cannot see it (its lower side is as wide as
    # the variance is unresolved), the one-sided check of check_clamp does
    st, c = fin_inputs("const", 64, H)
    top = float(np.float32(EPS)) ** -0.5
    for fused in (True, False):
        wrong = G.finalize_f32(st, H, EPS, fused, "no_clamp")[2].astype(np.float64)
        assert np.all(np.isfinite(wrong))
        control(f"variance without the clamp (constructed rows, H = 768, fused = {fused})", np.maximum(wrong, top), np.full(64, top),
                6 * U * top, need=1000.0)


def test_pack_layout_controls():
    packed, seq_row, seq_src, seq_len, rows = pack_case(3)
    ids, pos, tok = G.pack_layout(packed, seq_row, seq_src, seq_len, rows, PAD_ID)
    w_ids, w_pos, w_tok = G.pack_layout(packed, seq_row, seq_src, seq_len, rows, PAD_ID, "first_ge")
    # every row but the first of every sequence but the last (where the search runs off the end) becomes a pad row
    assert differ(w_tok, tok) == differ(w_ids, ids) == int((seq_len[:-1] - 1).sum()) > 0
    _, w_pos, _ = G.pack_layout(packed, seq_row, seq_src, seq_len, rows, PAD_ID, "pos_from_row")
    assert differ(w_pos, pos) == seq_len.sum()                                     # seq_row[0] > 0: no sequence starts at row 0


def test_splade_compact_controls():
    V, ld, thr = 1023, 1024, 0.25
    x = splade_rows(rng_for("splade control"), V, ld, 3, thr)
    n, idx, _ = G.splade_compact(x, V, thr, 1 << 30)
    n_ge, _, _ = G.splade_compact(x, V, thr, 1 << 30, "ge")
    assert n_ge[2] > n[2] and n_ge[0] == n[0]                     # entries equal to thr survive `>=`
    n_nm, idx_nm, _ = G.splade_compact(x, V, thr, 1 << 30, "no_mask")
    assert np.all(n_nm == n + (ld - V)) and idx_nm[1].tolist() == list(range(V, ld))     # the padding becomes hits
    n_cl, _, _ = G.splade_compact(x, V, thr, int(n[0]) - 1, "counts_clipped")
    assert n_cl[0] == n[0] - 1 and G.splade_compact(x, V, thr, int(n[0]) - 1)[0][0] == n[0]


def test_permute_controls():
    rng = rng_for("permute control")
    w = rng.integers(0, 1 << 16, (384, 128)).astype(np.uint16)
    s = f32(rng.standard_normal(384))
    good, bad = G.permute_qkv_heads(w, s, 128), G.permute_qkv_heads(w, s, 128, "head_part_swapped")
    assert differ(bad[0], good[0]) > 128 * 128 and differ(bad[1], good[1]) > 128


# ------------------------------------------------------------------ the -rP table
@gpu
def test_zz_worst_ratios():
    print("\nworst error / bound per (check, cols or H, type); every exact check of the module was array_equal")
    for (form, n, f16), r in sorted(_WORST.items(), key=lambda kv: (kv[0][0], kv[0][1] or 0, bool(kv[0][2]))):
        tag = "" if f16 is None else DT[bool(f16)]
        print(f"  {form:<58s} {str(n or ''):>5s} {tag:>5s} {r:10.4g}")
    for (form, n, f16), r in _WORST.items():
        if not form.startswith("control"):
            assert r <= 1.0, (form, n, f16, r)
