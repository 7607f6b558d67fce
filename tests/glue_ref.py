"""numpy references of the encoder's packing and glue kernels (csrc/glue_kernels.h, permute_qkv_heads of csrc/qkv_attn.h), written
from what their comments say they compute, and the error bounds tests/test_glue_unit_gpu.py derives in its docstring.  CPU only.
Every reference works on the fp32 values the kernel reads and takes `defect=`, the one wrong step of a negative control (the
names are listed at each function).  The conversions are bit-predictable, so their references return BITS."""
import numpy as np

from rows_ref import g
from unit16 import U, f32, from16, to16, trunc16

F16_MAX = np.float32(65504.0)
QNAN16 = {False: np.uint16(0x7FC0), True: np.uint16(0x7E00)}


# ------------------------------------------------------------------ 16-bit conversion as common.h documents it
def op16(v, f16, defect=None):
    """(bits, clamped) of Op<T>::to on fp32 values.  bf16: round to nearest even, inf stays inf, NaN stays a NaN (bits 0x7FC0
    here; the test compares NaN positions by isnan).  fp16: anything outside +-65504 is stored as +-65504 and flagged, NaN as
    -65504 and flagged.  defect: hi_trunc (round toward zero)."""
    v = f32(v)
    nan = np.isnan(v)
    if f16:
        clamped = bool(np.any(~(np.abs(v) <= F16_MAX)))
        with np.errstate(invalid="ignore"):
            v = np.where(nan, -F16_MAX, np.clip(v, -F16_MAX, F16_MAX)).astype(np.float32)
        if defect == "hi_trunc":
            return trunc16(v, True).astype(np.float16).view(np.uint16), clamped
        return to16(v, True), clamped
    if defect == "hi_trunc":
        bits = (np.where(nan, np.float32(0), v).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    else:
        bits = to16(np.where(nan, np.float32(0), v), False)
    return np.where(nan, QNAN16[False], bits).astype(np.uint16), False


def val16(bits, f16):
    """fp32 value of 16-bit bits (exact)."""
    return from16(bits, f16).astype(np.float32)


def split16(v, f16, defect=None, v_for_lo=None):
    """hi = T(v), lo = T(fl32(v - float(hi))): (hi bits, lo bits, clamped)."""
    v = f32(v)
    hi, c1 = op16(v, f16, defect)
    with np.errstate(invalid="ignore", over="ignore"):
        rem = (f32(v if v_for_lo is None else v_for_lo) - val16(hi, f16)).astype(np.float32)   # exact in fp32 where finite
    lo, c2 = op16(rem, f16)
    return hi, lo, c1 or c2


# ------------------------------------------------------------------ cvt_rows / cvt_split3
def interleave_source(r, I, defect=None):
    """The kernel comment's index map: each 64-row group = 32 input rows (x1) then the 32 matching gate rows (x2).
    Returns (source row, valid).  defect: f_g64 (f = g * 64 + w)."""
    gidx, w = r >> 6, r & 63
    f = gidx * 64 + w if defect == "f_g64" else gidx * 32 + (w & 31)
    return (f if w < 32 else I + f), f < I


def cvt_rows(src, rows_dst, f16, I=0, col_scale=None, defect=None):
    """dict(hi, lo: bits [rows_dst, cols]; row_sum, row_abs: float64 over the ROUNDED row; sat).  defects: hi_trunc, lo_unscaled,
    f_g64, pad_row0, sum_unrounded."""
    src = f32(src)
    rows_src, cols = src.shape
    x = np.zeros((rows_dst, cols), np.float32)
    for r in range(rows_dst):
        s, valid = interleave_source(r, I, defect) if I > 0 else (r, True)
        if valid and 0 <= s < rows_src:
            x[r] = src[s]
        elif defect == "pad_row0":
            x[r] = src[0]
    with np.errstate(invalid="ignore", over="ignore"):
        v = x if col_scale is None else (x * f32(col_scale)[None, :]).astype(np.float32)   # the multiply rounds in fp32 first
    hi, lo, sat = split16(v, f16, "hi_trunc" if defect == "hi_trunc" else None, x if defect == "lo_unscaled" else None)
    summed = v.astype(np.float64) if defect == "sum_unrounded" else from16(hi, f16)
    return dict(hi=hi, lo=lo, row_sum=summed.sum(1), row_abs=np.abs(from16(hi, f16)).sum(1), sat=sat)


def row_sum_bound(cols, row_abs):
    """row_sum against float64 of the rounded row: ceil(cols / 256) in-lane additions, six shuffle levels, two LDS adds."""
    return g(-(-cols // 256) + 6 + 2) * row_abs


def cvt_split3(src, rows_dst, f16, defect=None):
    """(bits [rows_dst, 3 cols] = [hi | hi | lo], sat); rows at and beyond rows_src are zero.  defects: hi_trunc, order_hi_lo_hi."""
    src = f32(src)
    rows_src, cols = src.shape
    x = np.zeros((rows_dst, cols), np.float32)
    n = min(rows_dst, rows_src)
    x[:n] = src[:n]
    hi, lo, sat = split16(x, f16, "hi_trunc" if defect == "hi_trunc" else None)
    return np.concatenate([hi, lo, hi] if defect == "order_hi_lo_hi" else [hi, hi, lo], axis=1), sat


# ------------------------------------------------------------------ 16-bit input families
def halfway_values(rng, n, f16):
    """fp32 values exactly halfway between two neighbouring finite values of the 16-bit type, both parities of the lower
    neighbour, both signs: round-to-nearest-EVEN decides every one of them."""
    if f16:
        b = rng.integers(0x0000, 0x7BFF, n).astype(np.uint16)      # subnormals included; b + 1 <= 0x7BFF = 65504
    else:
        b = rng.integers(0x0800, 0x7800, n).astype(np.uint16)      # 2^-111 .. 2^113: a row of them and its remainders stay normal fp32
    b[: n // 2] &= np.uint16(0xFFFE)
    b[n // 2:] |= np.uint16(0x0001)
    mid = (from16(b, f16) + from16(b + np.uint16(1), f16)) / 2.0
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid), "a halfway point must be an fp32 value"
    sign = np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0)
    return f32(mid * sign)


def f16_small_values(rng, n):
    """Values whose fp16 image is subnormal or zero, the ties at 2^-25 and 3 * 2^-25 and their fp32 neighbours included."""
    t = np.float32(2.0 ** -25)
    fixed = [t, -t, np.nextafter(t, np.float32(1)), np.nextafter(t, np.float32(0)), 3 * t, -3 * t, np.float32(2.0 ** -24),
             np.float32(2.0 ** -26), np.float32(1023.5 * 2.0 ** -24), np.float32(2.0 ** -14), np.nextafter(np.float32(2.0 ** -14), np.float32(0))]
    rnd = rng.uniform(-2.0 ** -14, 2.0 ** -14, max(n - len(fixed), 0))
    return f32(np.concatenate([f32(fixed), f32(rnd)])[:n])


# ------------------------------------------------------------------ ln_stats_finalize
def finalize(part, H, eps, shift_in=None, defect=None):
    """float64 of the fp32 partials [np, rows, 2]: (d, var, rstd, shift_out, shift_prev).  eps is taken as the fp32 value the
    kernel receives.  defects: var_H-1, shift_is_d."""
    p = np.asarray(f32(part), np.float64)
    s1, s2 = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    c = np.zeros_like(s1) if shift_in is None else np.asarray(f32(shift_in), np.float64)
    d = s1 / H
    var = np.maximum(s2 / H - d * d, 0.0)
    if defect == "var_H-1":
        var = var * H / (H - 1)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    return d, var, rstd, (d if defect == "shift_is_d" else c + d), c


def finalize_bounds(part, H, eps, shift_in=None):
    """(E_d, E_var, E_rstd, E_shift): the module docstring's terms.  "One ulp" = 2 U relative, the siblings' convention."""
    p = np.asarray(f32(part), np.float64)
    n = p.shape[0]
    d, var, rstd, shift, _ = finalize(part, H, eps, shift_in)
    tiny = 1e-30
    e_d = g(n) * np.abs(p[:, :, 0]).sum(0) / H + 2.0 * U * np.abs(d) + tiny
    t1 = p[:, :, 1].sum(0) / H
    e_t1 = g(n) * np.abs(p[:, :, 1]).sum(0) / H + 2.0 * U * np.abs(t1)
    e_t2 = 2.0 * np.abs(d) * e_d + e_d * e_d + U * d * d            # d~ * d~ against d * d, the product rounds (or is fused)
    e_pre = e_t1 + e_t2
    e_var = e_pre + U * (np.abs(t1 - d * d) + e_pre) + tiny          # the subtraction rounds; max(., 0) is 1-Lipschitz
    epsf = float(np.float32(eps))
    s = var + epsf
    e_s = e_var + U * (s + e_var)
    # var~ >= 0 whatever the errors (the clamp), so var~ + eps >= eps (1 - U): rstd~ lies between the two roots
    lo = (s + e_s) ** -0.5 * (1.0 - 4.0 * U)
    hi = np.maximum(s - e_s, epsf * (1.0 - U)) ** -0.5 * (1.0 + 4.0 * U)   # sqrtf and 1 / x: one ulp each
    e_rstd = np.maximum(hi - rstd, rstd - lo)
    e_shift = e_d + U * (np.abs(shift) + e_d) + tiny
    return e_d, e_var, e_rstd, e_shift


def finalize_f32(part, H, eps, fused, defect=None):
    """The kernel's arithmetic step by step in fp32 (partials added in slice order; `fused`: s2 / H - d * d as one fma):
    (d, var before the clamp, rstd).  Used to CONSTRUCT the rows whose variance comes out negative and for the control without
    the clamp.  defect: no_clamp."""
    p = f32(part)
    s1 = np.zeros(p.shape[1], np.float32)
    s2 = np.zeros(p.shape[1], np.float32)
    for i in range(p.shape[0]):
        s1 = (s1 + p[i, :, 0]).astype(np.float32)
        s2 = (s2 + p[i, :, 1]).astype(np.float32)
    d = (s1 / np.float32(H)).astype(np.float32)
    t1 = (s2 / np.float32(H)).astype(np.float32)
    if fused:
        pre = (t1.astype(np.float64) - d.astype(np.float64) * d.astype(np.float64)).astype(np.float32)   # d * d is exact in float64
    else:
        pre = (t1 - (d * d).astype(np.float32)).astype(np.float32)
    var = pre if defect == "no_clamp" else np.maximum(pre, np.float32(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        rstd = (np.float32(1) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    return d, pre, rstd


def partials_of(x, H):
    """Slice-major fp32 partials [H / 64, rows, 2] of fp32 rows x [rows, H]: per 64-feature slice, sum and sum of squares."""
    xs = f32(x).reshape(x.shape[0], H // 64, 64)
    st = np.zeros((H // 64, x.shape[0], 2), np.float32)
    st[:, :, 0] = xs.sum(2, dtype=np.float32).T
    st[:, :, 1] = (xs * xs).sum(2, dtype=np.float32).T
    return st


def stats_rows(rng, family, rows, H):
    """(partials, shift c) of one family.  spread: unit-variance rows around a shift close to their mean; mean: the mean is 50 x
    the spread and far from c; const: near-constant rows, |x| ~ 2, spread 1e-4 -- s2 / H - d^2 is pure rounding."""
    z = rng.standard_normal((rows, H))
    if family == "spread":
        x = 1.5 * z + 0.3 * rng.standard_normal((rows, 1))
    elif family == "mean":
        x = 50.0 * np.sign(rng.standard_normal((rows, 1))) + z
    elif family == "const":
        x = rng.uniform(1.5, 2.5, (rows, 1)) * np.sign(rng.standard_normal((rows, 1))) + 1e-4 * z
    else:
        raise ValueError(family)
    return partials_of(f32(x), H), f32(rng.standard_normal(rows))


# ------------------------------------------------------------------ pack_layout
def pack_layout(packed, seq_row, seq_src, seq_len, rows, pad_id, defect=None):
    """(ids, pos, tok_seq) [rows] int32.  defects: first_ge (the bisection returns the first sequence whose row is >= r),
    pos_from_row."""
    ids = np.full(rows, pad_id, np.int32)
    pos = np.zeros(rows, np.int32)
    tok = np.full(rows, -1, np.int32)
    if defect == "first_ge":
        for r in range(rows):
            s = int(np.searchsorted(seq_row, r, side="left"))
            s = min(s, len(seq_row) - 1)
            i = r - seq_row[s]
            if 0 <= i < seq_len[s]:
                ids[r], pos[r], tok[r] = packed[seq_src[s] + i], i, s
        return ids, pos, tok
    for s, (r0, src, n) in enumerate(zip(seq_row, seq_src, seq_len)):
        ids[r0:r0 + n] = packed[src:src + n]
        pos[r0:r0 + n] = np.arange(r0, r0 + n) if defect == "pos_from_row" else np.arange(n)
        tok[r0:r0 + n] = s
    return ids, pos, tok


# ------------------------------------------------------------------ splade_compact
def splade_compact(rows, V, thr, cap, defect=None):
    """(counts [n], list of index arrays, list of value arrays): per row the entries > thr of the first V, in index order, at
    most cap stored; counts = the total.  defects: ge, no_mask (the padding [V, ld) read as data), counts_clipped."""
    rows = f32(rows)
    counts, idx, val = [], [], []
    for row in rows:
        data = row if defect == "no_mask" else row[:V]
        hit = np.nonzero(data >= np.float32(thr) if defect == "ge" else data > np.float32(thr))[0].astype(np.int32)
        counts.append(min(len(hit), cap) if defect == "counts_clipped" else len(hit))
        idx.append(hit[:cap])
        val.append(row[hit[:cap]])
    return np.asarray(counts, np.int32), idx, val


# ------------------------------------------------------------------ permute_qkv_heads
def permute_qkv_heads(w, s, H, defect=None):
    """Rows q | k | v of all heads -> per head q(64) k(64) v(64): (w_out [3 H, H], s_out [3 H] or None).  defect: head_part_swapped."""
    orow = np.arange(3 * H)
    head, part, d = orow // 192, (orow % 192) // 64, orow % 64
    if defect == "head_part_swapped":
        head, part = part % (H // 64), head % 3
    src = part * H + head * 64 + d
    return w[src], (None if s is None else s[src])


# ------------------------------------------------------------------ self-checks (CPU; run by tests/test_glue_unit_gpu.py)
def check_op16_matches_the_documented_fp16_range():
    v = f32([65504.0, 65519.0, 65536.0, 7e4, -1e6, np.inf, -np.inf, np.nan, 0.0, -0.0])
    bits, sat = op16(v, True)
    assert sat
    assert from16(bits, True).tolist() == [65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0, -65504.0, -65504.0, 0.0, 0.0]
    assert bits[-1] == 0x8000 and bits[-2] == 0
    assert op16(f32([65504.0, -65504.0, 1.0]), True)[1] is False
    b, sat = op16(f32([np.inf, -np.inf, np.nan, 1.0]), False)
    assert not sat and b.tolist() == [0x7F80, 0xFF80, 0x7FC0, 0x3F80]


def check_halfway_values_round_to_even():
    rng = np.random.default_rng(0)
    for f16 in (False, True):
        v = halfway_values(rng, 512, f16)
        bits, _ = op16(v, f16)
        assert np.all(bits & 1 == 0), "a tie must land on the even neighbour"
        down = trunc16(v, f16)
        assert np.mean(from16(bits, f16) != down) > 0.3 and np.mean(from16(bits, f16) == down) > 0.3   # both directions occur
    t = np.float32(2.0 ** -25)
    assert op16(f32([t, 3 * t, np.nextafter(t, np.float32(1))]), True)[0].tolist() == [0, 2, 1]


def check_interleave_map_is_a_bijection_onto_the_features():
    for I in (32, 40, 96, 100):
        rows_dst = 64 * -(-I // 32)
        src = [interleave_source(r, I) for r in range(rows_dst)]
        used = sorted(s for s, ok in src if ok)
        assert used == list(range(2 * I))
        for r, (s, ok) in enumerate(src):
            if ok:
                assert (s < I) == ((r & 63) < 32) and s % I == (r >> 6) * 32 + (r & 31)


def check_split_lo_is_exact_remainder():
    rng = np.random.default_rng(1)
    v = f32(rng.standard_normal(4096))
    for f16 in (False, True):
        hi, lo, sat = split16(v, f16)
        assert not sat
        rem = v.astype(np.float64) - from16(hi, f16)
        assert np.array_equal(rem.astype(np.float32).astype(np.float64), rem)      # the subtraction is exact in fp32
        assert np.array_equal(lo, to16(rem, f16))


SELF_CHECKS = ("check_op16_matches_the_documented_fp16_range", "check_halfway_values_round_to_even",
               "check_interleave_map_is_a_bijection_onto_the_features", "check_split_lo_is_exact_remainder")
