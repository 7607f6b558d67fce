"""16-bit operand helpers and the error / bound ledger shared by the kernel unit tests (test_gemm_unit_gpu.py,
test_qkv_attn_unit_gpu.py, test_attn_unit_gpu.py, test_rows_unit_gpu.py with its references in rows_ref.py): bit-exact bf16 / fp16 conversion, the half-ulp allowance of a 16-bit store, and `record` / `control`,
which assert a per-element bound and note the worst error / bound ratio for the module's `-rP` table."""
from collections import defaultdict

import numpy as np

U = 2.0 ** -24          # fp32 unit roundoff


def to16(x, f16):
    """float64 -> 16-bit bits (round to nearest even through fp32)."""
    x32 = np.ascontiguousarray(x, np.float32)
    if f16:
        return x32.astype(np.float16).view(np.uint16)
    u = x32.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from16(b, f16):
    b = np.ascontiguousarray(b, np.uint16)
    if f16:
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def trunc16(x, f16):
    """The nearest wrong kernel of a 16-bit store: round toward zero instead of to nearest even."""
    x32 = np.ascontiguousarray(x, np.float32)
    if not f16:
        return from16((x32.view(np.uint32) >> 16).astype(np.uint16), False)
    h = x32.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x32.astype(np.float64))
    h[over] = np.nextafter(h[over], np.float16(0))
    return h.astype(np.float64)


def half_ulp(x, f16):
    e = np.floor(np.log2(np.maximum(np.abs(x), 1e-300)))
    return 2.0 ** (np.maximum(e, -14) - 11) if f16 else 2.0 ** (np.maximum(e, -126) - 8)


def out16_bound(ref, e, f16):
    return e + half_ulp(np.abs(ref) + e, f16)


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def make_ledger():
    """(worst, record, control) of one test module: worst[(form, config, f16)] = the worst error / bound ratio seen."""
    worst = defaultdict(float)

    def record(form, cfg, f16, got, ref, bound):
        err = np.abs(np.asarray(got, np.float64) - ref)
        ratio = float(np.max(err / bound)) if err.size else 0.0
        key = (form, cfg, f16)
        worst[key] = max(worst[key], ratio)
        bad = np.argwhere(~(err <= bound))
        assert bad.size == 0, (f"{form} cfg={cfg} f16={f16}: {len(bad)} elements over the bound, first at {tuple(bad[0])}: "
                               f"got {np.asarray(got).flat[np.ravel_multi_index(tuple(bad[0]), err.shape)]} "
                               f"ref {ref.flat[np.ravel_multi_index(tuple(bad[0]), err.shape)]} worst ratio {ratio:.3g}")
        return ratio

    def control(name, got_wrong, ref, bound, need=10.0):
        """Negative control: the nearest wrong kernel's output must exceed the bound by `need` x somewhere."""
        r = float(np.max(np.abs(np.asarray(got_wrong, np.float64) - ref) / bound))
        worst[("control: " + name, None, None)] = r
        assert r >= need, f"control {name}: the bound hides it (worst ratio {r:.3g} < {need})"
        return r

    return worst, record, control
