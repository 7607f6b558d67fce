"""The fused Wqkv + RoPE + attention kernel ALONE (vrag_debug_qkv_attn_run, csrc/qkv_attn.hip) against its stated arithmetic in
float64, on the SAME 16-bit operand bits the kernel reads; every row of every sequence is referenced.

Reference per (sequence, head): proj = x . W^T; with the fold rstd * (proj - mu * s); RoPE with partner d + 32, the position being
the token's index inside ITS sequence and cos / sin the passed table's rows at that position; q times q_scale; scores in log2
units; mask j < S and, banded, |i - j| <= window; exp2 softmax; P . V.  The rotary tables are genuine ones (rope_table of capi.hip:
the kernel rebuilds row 16 b + i from rows 16 b and i by angle addition, so a random table is wrong by design).

Scope: the hook runs the HARNESS build (-DVRAG_DEBUG_API) of qkv_attn.hip with debug_flags = 0; the product build of the same
source stays covered by the encoder suites (test_fused_attention_gpu.py, test_full_shapes_gpu.py) and test_kernel_resources.py.
The hook permutes the weights itself (permute_qkv_heads), so that kernel is under test too.

Bound, per output element (never tuned to what the kernel returns; U = 2^-24):
  projections  2 K U (|x| . |W|^T) for the fp32 accumulation over K, the fold as in test_gemm_unit_gpu.py (fold_ref);
  RoPE         cos / sin by angle addition differ from the table row at pos by the angle the fp32 roundings of 16 b f, i f and
               pos f leave, |fl(16 b f) + fl(i f) - fl(pos f)| (computed from the table's own angles), plus 6 U for the three fp32
               operations on four rounded table entries; the rotation adds 2 U per product pair and U for the scale;
  q, k, v      + half an ulp of the 16-bit type each (E_q, E_k, E_v);
  scores       E_s = E_q . |k|^T + |q| . E_k^T + E_q . E_k^T + 2 (64 + 2) U (|q| . |k|^T + max |s|): fp32 accumulation over 64
               with the running reference riding in the accumulator;
  P            relative error eta = 2^E_s - 1 (propagation through exp2) + half an ulp of P (2^-8 bf16, 2^-11 fp16) + 4 U (v_exp_f32,
               the subtraction of the moved reference); fp16 P below 2^-14 is subnormal: 2^-25 absolute against a row sum >= 1
               (the lazy reference keeps the row's largest P in [1, 2^8]);
  output       o~ - o = sum_j w_j eta_j (v_j - o) / (1 + sum_j w_j eta_j) exactly (the SAME P feeds the row sums, so a common
               factor cancels), hence sum_j w_j eta_j |v_j - o| / (1 - A), A = sum_j w_j eta_j + n_keys 2^-25 [fp16];
               + sum_j w_j E_v; + 2 (S + 16) U for the two fp32 accumulations over the keys and their rescales; + 3 U |o|;
               + half an ulp of the stored output.
No constant of the bound was measured: every term follows from the number formats and the operation counts above.

Negative controls (float64 reference with one defect, computed on the CPU; each must exceed the bound 10 x on its case):
band window - 1 / + 1, key j = S admitted, the previous sequence of the group admitted, the position taken from the workgroup
slot, RoPE partner d + 16, the mu * s term dropped, q_scale dropped, P truncated instead of rounded.  Two of them need their case:
  * a rotary embedding is relative: shifting the positions of q AND k by 64 * first_wave changes no score, so that defect shows
    only where the shifted position runs off the table (test_short_rotary_table, rope_rows = 17; with 10 rows every shifted
    position clamps to row 9 + i, a uniform shift again).  q ALONE at its slot position is rejected on the ragged case;
  * P truncated hides under the general bound: P is granted half an ulp, and the row sums are built from the very same P.  The
    crafted scores of test_lazy_reference make the 16-bit P predictable bit for bit, so that there the reference rounds P itself,
    the bound grants P nothing, and a truncated P is rejected.

`-rP` prints the worst error / bound ratio per case and per (row mod 64) class (a fragment-mapping slip shows as one class
standing out).  Measured on an MI355X: see MEASURED below."""
import ctypes as C
import math
from collections import defaultdict

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib
from attn_ref import attend
from unit16 import U, f32, from16, half_ulp, make_ledger, to16, trunc16

gpu = pytest.mark.gpu

MEASURED = """worst error / bound on an MI355X, all rows and heads; (row mod 64) classes as min / median / max @ class of the max
  ragged   bf16 global nofold 0.640 (0.442 / 0.540 / 0.640 @ 52)   fold 0.658 (0.439 / 0.546 / 0.658 @ 29)
           bf16 banded nofold 0.642 (0.495 / 0.569 / 0.642 @ 39)   fold 0.647 (0.455 / 0.562 / 0.647 @ 22)
           fp16 global nofold 0.777 (0.474 / 0.615 / 0.777 @ 35)   fold 0.743 (0.463 / 0.612 / 0.743 @ 16)
           fp16 banded nofold 0.760 (0.444 / 0.668 / 0.760 @ 22)   fold 0.766 (0.511 / 0.649 / 0.766 @ 8)
  band     bf16 nofold / fold: W=64 0.598 / 0.619, W=17 0.625 / 0.625, W=600 0.651 / 0.578
           fp16 nofold / fold: W=64 0.671 / 0.728, W=17 0.746 / 0.687, W=600 0.735 / 0.748; classes 0.16 .. 0.75
  rope_rows = 17 / 10   bf16 0.63 .. 0.65 / 0.57 .. 0.66, fp16 0.66 .. 0.73 / 0.72 .. 0.79 (classes 0 .. 16 only are live)
  lazy, 7.5 climb       global bf16 0.757 fp16 0.324; banded W=64 0.924 / 0.868, W=17 0.970 / 0.938 (fold = nofold: exact operands)
  lazy, exact P         0.980 .. 0.999 in every instantiation, every class within 0.03 of it: the stored output's own half ulp is
                        nearly all this bound grants, and a correctly rounded output comes that close to it
  garbage (sharp 2)     bf16 0.441 .. 0.470, fp16 0.399 .. 0.445
no class and no instantiation stands out.  Controls, smallest ratio over the instantiations that run them: band - 1 / + 1 267 / 205,
key j = S 85, previous sequence 927, q and k at the slot position 118, q alone 2177, partner d + 16 2705, mu * s dropped 454,
q_scale dropped 36, P truncated 23 (global) and 66 (banded, W = 17).
Properties the module holds the kernel to beside the reference: a sequence's bits do not depend on packer, wave slot, group or
buffer neighbours; in particular the query rows BEHIND a sequence inside its last wave (the next sequence's tokens, or garbage)
must not time a move of the softmax reference (test_garbage_rows_do_not_leak)."""

H, NH = 192, 3            # three heads; three 64-k stages, so weight buffer 0 is refilled
Q_SCALE = float(np.float32(0.125 * 1.4426950408889634))
THETA = {0: 160000.0, 1: 10000.0}     # global / banded layers
CANARY = 0x7A5C
_WORST, record, control = make_ledger()
_CLASS = defaultdict(lambda: np.zeros(64))   # case -> worst ratio per (row mod 64)
INSTANTIATIONS = [(f16, local, fold) for f16 in (False, True) for local in (0, 1) for fold in (False, True)]


def inst_id(v):
    f16, local, fold = v
    return f"{'fp16' if f16 else 'bf16'}-{'banded' if local else 'global'}-{'fold' if fold else 'nofold'}"


# ------------------------------------------------------------------ the hook
def pack(seq_row, seq_len, packer):
    """vrag_debug_pack_groups (host only): the [n_groups, 8, 4] wave descriptors."""
    dbg = _lib.load_debug()
    row, ln = np.ascontiguousarray(seq_row, np.int32), np.ascontiguousarray(seq_len, np.int32)
    out = np.full((len(row), 8, 4), -7, np.int32)
    n = dbg.vrag_debug_pack_groups(row.ctypes.data, ln.ctypes.data, len(row), packer, out.ctypes.data)
    assert n > 0, n
    assert np.all(out[n:] == -7)
    return out[:n]


def raw_run(inp, seqs, f16, local, window, packer=0, o=None, q_scale=Q_SCALE, null=(), **override):
    """One launch; returns (status, o bits [rows, H], groups [n_groups, 8, 4], f16_saturated)."""
    dbg = _lib.load_debug()
    a = _lib.DebugQkvAttnArgs()
    rows = inp["ln_rstd" if "x" not in inp else "x"].shape[0]
    o = np.full((rows, H), CANARY, np.uint16) if o is None else o
    seq_row = np.ascontiguousarray([r for r, _ in seqs], np.int32)
    seq_len = np.ascontiguousarray([n for _, n in seqs], np.int32)
    groups = np.zeros((len(seqs), 8, 4), np.int32)
    keep = [o, seq_row, seq_len, groups]
    for name in ("x", "w", "ln_s", "ln_mu", "ln_rstd", "rope_cos", "rope_sin"):
        arr = inp.get(name)
        if arr is not None:
            assert arr.flags.c_contiguous, name
            setattr(a, name, arr.ctypes.data)
    a.o, a.seq_row, a.seq_len, a.groups_out = o.ctypes.data, seq_row.ctypes.data, seq_len.ctypes.data, groups.ctypes.data
    a.rows, a.H, a.nh, a.rope_rows, a.n_seqs = rows, H, NH, inp["rope_sin"].shape[0], len(seqs)
    a.packer, a.local, a.window, a.f16, a.q_scale = packer, local, window, int(f16), q_scale
    for k, v in override.items():
        setattr(a, k, v)
    for k in null:
        setattr(a, k, None)
    status = dbg.vrag_debug_qkv_attn_run(C.byref(a), 0)
    del keep
    return status, o, groups[:max(a.n_groups, 0)], a.f16_saturated


def run(inp, seqs, f16, local, window, packer=0, **kw):
    status, o, groups, sat = raw_run(inp, seqs, f16, local, window, packer, **kw)
    if status == -2:   # VRAG_ERR_HIP: a failed launch or a clobbered canary: nothing more goes onto this device
        msg = _lib.load_debug().vrag_last_error()
        pytest.exit(f"vrag_debug_qkv_attn_run: {msg.decode() if msg else status}", returncode=3)
    _lib.check_debug("vrag_debug_qkv_attn_run", status)
    assert np.array_equal(groups, pack([r for r, _ in seqs], [n for _, n in seqs], packer))
    return o, groups, sat


# ------------------------------------------------------------------ operands
def rope_table(n, theta):
    """capi.hip's rope_table: fp32 angles p * inv_freq_j, cos / sin rounded to fp32.  Returns (cos, sin, angles)."""
    inv = (np.float32(1.0) / np.power(np.float32(theta), (2 * np.arange(32, dtype=np.float32)) / np.float32(64.0))).astype(np.float32)
    ang = (np.arange(n, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32)
    return f32(np.cos(ang.astype(np.float64))), f32(np.sin(ang.astype(np.float64))), ang


def place(lengths, rng, gaps=(0, 8, 24, 72)):
    """Rows for the sequences: buffer order shuffled against list order, 8-aligned, with gaps.  Returns (seqs, rows)."""
    order = rng.permutation(len(lengths))
    row, cur = [0] * len(lengths), int(rng.choice(gaps))
    for i in order:
        row[i] = cur
        cur += -(-lengths[i] // 8) * 8 + int(rng.choice(gaps))
    need = max(r + 64 * -(-n // 64) for r, n in zip(row, lengths))
    return list(zip(row, lengths)), -(-need // 256) * 256


def make_inputs(rng, rows, f16, local, fold, sharp=6.0, rope_rows=512, filler=1.0):
    """x [rows, H] unit variance everywhere (rows outside the sequences included: the kernel must mask them), Wqkv with q rows
    scaled by `sharp` (unit-variance q / k: sharp attention), fold statistics as the encoder builds them."""
    inp = {}
    if fold:
        h = rng.standard_normal((rows, H)) * 1.5 + rng.standard_normal((rows, 1)) * 2
        c = h.mean(1) + rng.standard_normal(rows) * 0.3
        x = (h - c[:, None]) * filler
    else:
        x = rng.standard_normal((rows, H)) * filler
    inp["x"] = to16(x, f16)
    w = rng.standard_normal((3 * H, H)) / math.sqrt(H)
    w[:H] *= sharp
    inp["w"] = to16(w, f16)
    if fold:
        xf = from16(inp["x"], f16)
        inp["ln_s"] = f32(from16(inp["w"], f16).sum(1))
        inp["ln_mu"] = f32(xf.mean(1))
        inp["ln_rstd"] = f32(1 / np.sqrt(xf.var(1) + 1e-5))
    inp["rope_cos"], inp["rope_sin"], inp["rope_ang"] = rope_table(rope_rows, THETA[local])
    return inp


def live_mask(rows, seqs):
    m = np.zeros(rows, bool)
    for r, n in seqs:
        m[r:r + n] = True
    return m


# ------------------------------------------------------------------ float64 reference and bound
def rope64(x, cos, sin, partner=32):
    """x [n, 64], cos / sin [n, 32]: q cos + rotate_half(q) sin with partner d + 32 (or the wrong kernel's d + 16)."""
    if partner == 32:
        x1, x2 = x[:, :32], x[:, 32:]
        return np.concatenate([x1 * cos - x2 * sin, x2 * cos + x1 * sin], 1)
    xr = x.reshape(-1, 2, 2, 16)
    c, s = cos.reshape(-1, 2, 16), sin.reshape(-1, 2, 16)
    a, b = xr[:, :, 0], xr[:, :, 1]
    return np.stack([a * c - b * s, b * c + a * s], 2).reshape(-1, 64)


def project(inp, f16, fold, rows_idx, pos, head, part, scale=1.0, exact=False, partner=32, drop_fold=False, slot_pos=None):
    """The kernel's 16-bit q (part 0), k (1) or v (2) of `head` for token rows `rows_idx` at positions `pos`, in float64, and the
    bound E of its distance to the kernel's value (half an ulp of the 16-bit rounding included)."""
    xf = from16(inp["x"][rows_idx], f16)
    wf = from16(inp["w"][part * H + head * 64: part * H + head * 64 + 64], f16)
    v = xf @ wf.T
    e = np.zeros_like(v) if exact else 2 * H * U * (np.abs(xf) @ np.abs(wf).T)
    if fold:
        mu, rs = inp["ln_mu"][rows_idx].astype(np.float64)[:, None], inp["ln_rstd"][rows_idx].astype(np.float64)[:, None]
        s = inp["ln_s"][part * H + head * 64: part * H + head * 64 + 64].astype(np.float64)[None, :]
        t = v - (0 if drop_fold else mu * s)
        e = np.abs(rs) * (e + 2 * U * (np.abs(v) + np.abs(mu * s))) + U * np.abs(rs * t)
        v = rs * t
    if part < 2:
        R = inp["rope_cos"].shape[0]
        if slot_pos is not None:   # the wrong kernel: position inside the workgroup, rows 16 b and i clamped as the kernel clamps
            pa, pb = np.minimum(16 * (slot_pos >> 4), R - 1), np.minimum(slot_pos & 15, R - 1)
            ang = inp["rope_ang"][pa].astype(np.float64) + inp["rope_ang"][pb].astype(np.float64)
            cos, sin = np.cos(ang), np.sin(ang)
            e_c = 0.0
        else:
            cos, sin = inp["rope_cos"][pos].astype(np.float64), inp["rope_sin"][pos].astype(np.float64)
            ang = inp["rope_ang"].astype(np.float64)
            e_c = 0.0 if exact else np.abs(ang[16 * (pos >> 4)] + ang[pos & 15] - ang[pos]) + 6 * U
        r = rope64(v, cos, sin, partner)
        ax = np.abs(v)
        amp = ax[:, :32] + ax[:, 32:]
        if not exact:
            e1 = e[:, :32] * np.abs(cos) + e[:, 32:] * np.abs(sin) + amp * (e_c + 2 * U)
            e2 = e[:, 32:] * np.abs(cos) + e[:, :32] * np.abs(sin) + amp * (e_c + 2 * U)
            e = (np.concatenate([e1, e2], 1) + U * np.abs(r)) * abs(scale)
        v = r * scale
    if exact:
        assert np.array_equal(from16(to16(v, f16), f16), v), "the crafted operands must be exact in 16 bits"
        return v, np.zeros_like(v)
    return v, e + half_ulp(np.abs(v) + e, f16)


def reference(inp, seq, head, f16, local, fold, window, q_scale=Q_SCALE, exact=False, defect=None, prev=None, kbase=0,
              exact_p=False):
    """(ref, bound) [S, 64] of one (sequence, head); `defect` names the one wrong step of a negative control."""
    r0, S = seq
    tok = np.arange(S)
    kw = dict(exact=exact)
    if defect == "partner16":
        kw["partner"] = 16
    if defect == "fold_dropped":
        kw["drop_fold"] = True
    sp = dict(slot_pos=64 * kbase + tok) if defect in ("slot_pos", "slot_pos_q") else {}
    q, Eq = project(inp, f16, fold, r0 + tok, tok, head, 0, scale=1.0 if defect == "q_scale" else q_scale, **kw, **sp)
    keys, kj = tok, tok
    S_eff, win = S, window
    if defect == "band-1":
        win = window - 1
    if defect == "band+1":
        win = window + 1
    if defect == "key_S":      # the first row behind the sequence let through
        keys, kj, S_eff = np.arange(S + 1), np.arange(S + 1), S + 1
    k, Ek = project(inp, f16, fold, r0 + keys, keys, head, 1, **kw, **(dict(slot_pos=64 * kbase + keys) if defect == "slot_pos" else {}))
    v, Ev = project(inp, f16, fold, r0 + keys, keys, head, 2, **kw)
    if defect == "key_S":      # the kernel zeroes V behind the sequence; the key's weight still enters the row sum
        v[S] = 0
    if defect == "prev_seq":   # the keys of the group's previous sequence, at their slots in front of this one
        pr0, pS, pbase = prev
        ptok = np.arange(pS)
        pk, pEk = project(inp, f16, fold, pr0 + ptok, ptok, head, 1, **kw)
        pv, pEv = project(inp, f16, fold, pr0 + ptok, ptok, head, 2, **kw)
        k, Ek, v, Ev = np.concatenate([pk, k]), np.concatenate([pEk, Ek]), np.concatenate([pv, v]), np.concatenate([pEv, Ev])
        kj = np.concatenate([ptok + 64 * (pbase - kbase), kj])
    p16 = (lambda p: trunc16(p, f16)) if defect == "p_trunc" and not exact_p else None
    mode = ("trunc" if defect == "p_trunc" else "round") if exact_p else None
    return attend(q, Eq, k, Ek, v, Ev, tok, kj, S_eff, local, win, f16, p16, strict=defect is None, exact_p=mode)


def check(case, inp, seqs, o, f16, local, fold, window, **kw):
    """Every row of every sequence and head against the reference; returns {(seq index, head): (ref, bound)}."""
    out = {}
    for si, (r0, S) in enumerate(seqs):
        for head in range(NH):
            ref, bound = reference(inp, (r0, S), head, f16, local, fold, window, **kw)
            got = from16(o[r0:r0 + S, head * 64:(head + 1) * 64], f16)
            ratio = (np.abs(got - ref) / bound).max(1)
            cls = _CLASS[case]
            np.maximum.at(cls, np.arange(S) % 64, ratio)
            record(case, None, f16, got, ref, bound)
            out[(si, head)] = (ref, bound)
    return out


def worst_control(name, inp, seqs, refs, f16, local, fold, window, defect, which=None, **kw):
    """The defect's worst ratio over the given sequences (all heads), through the ledger's control()."""
    best, arg = 0.0, None
    for si in (which if which is not None else range(len(seqs))):
        for head in range(NH):
            ref, bound = refs[(si, head)]
            extra = {k: (v[si] if isinstance(v, dict) else v) for k, v in kw.items()}
            wrong, _ = reference(inp, seqs[si], head, f16, local, fold, window, defect=defect, **extra)
            r = float((np.abs(wrong - ref) / bound).max())
            if r > best:
                best, arg = r, (wrong, ref, bound)
    assert arg is not None, name
    return control(f"{name} [{inst_id((f16, local, fold))}]", *arg)


# ------------------------------------------------------------------ ragged geometry: packing, placement, all eight instantiations
# lengths on and off the 64-token wave grid, in a list order at which BOTH packers meet assert_packing
RAGGED = [320, 128, 257, 17, 64, 8, 130, 449, 40, 63, 65, 200, 512, 1, 511, 192, 193, 384, 129]


def ragged_layout():
    rng = np.random.default_rng(2024)
    return place(RAGGED, rng)


def assert_packing(groups, seqs):
    """What the ragged case is there to reach, on the packing that actually ran."""
    n = len(groups)
    assert n > 8 and n % 8 != 0, n
    starts = {int(w[2]) for g in groups for w in g if w[1] > 0}
    assert starts >= set(range(8)), starts
    assert any(g[7][1] == 0 for g in groups), "no unused trailing wave"
    end_of = {r: r + -(-ln // 8) * 8 for r, ln in seqs}
    apart = False
    for g in groups:
        firsts = [(int(w[0]) - 64 * (i - int(w[2])), int(w[1])) for i, w in enumerate(g) if w[1] > 0 and int(w[2]) == i]
        for (ra, _), (rb, _) in zip(firsts, firsts[1:]):
            apart |= not (0 <= rb - end_of[ra] <= 72)
    assert apart, "every group's sequences are neighbours in the buffer"


def test_ragged_layout_reaches_every_branch():
    seqs, rows = ragged_layout()
    assert rows <= 6144
    for packer in (0, 1):
        assert_packing(pack([r for r, _ in seqs], [n for _, n in seqs], packer), seqs)


@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_ragged(inst):
    f16, local, fold = inst
    seqs, rows = ragged_layout()
    window = 64
    rng = np.random.default_rng(100 + 4 * f16 + 2 * local + fold)
    inp = make_inputs(rng, rows, f16, local, fold)
    o0, g0, sat0 = run(inp, seqs, f16, local, window, packer=0)
    assert sat0 == 0
    assert_packing(g0, seqs)
    case = "ragged " + inst_id(inst)
    refs = check(case, inp, seqs, o0, f16, local, fold, window)
    live = live_mask(rows, seqs)
    assert np.all(o0[~live] == CANARY), "the kernel wrote a row outside the sequences"
    # ---- placement-independent bits: the other packer, every sequence alone, other neighbours
    o1, g1, _ = run(inp, seqs, f16, local, window, packer=1)
    assert_packing(g1, seqs)
    assert not np.array_equal(g0, g1)
    assert np.array_equal(o0, o1), "packer 0 and packer 1 give different bits"
    slot0 = {int(w[0]): int(w[2]) for g in g0 for i, w in enumerate(g) if w[1] > 0 and int(w[2]) == i}
    slot1 = {int(w[0]): int(w[2]) for g in g1 for i, w in enumerate(g) if w[1] > 0 and int(w[2]) == i}
    assert sum(slot0[r] != slot1[r] for r, _ in seqs) >= 4, "the packers put too few sequences at different wave slots"
    rev = seqs[::-1]
    o2, _, _ = run(inp, rev, f16, local, window, packer=0)
    assert np.array_equal(o0, o2), "other neighbours in the group change the bits"
    for si in (0, 1, 6, 15):   # alone: wave slot 0, no neighbours
        o3, _, _ = run(inp, [seqs[si]], f16, local, window)
        r0, S = seqs[si]
        assert np.array_equal(o3[r0:r0 + S], o0[r0:r0 + S]), f"sequence {si} alone differs"
        assert np.all(np.delete(o3, np.s_[r0:r0 + S], 0) == CANARY)
    # ---- negative controls
    kbase = {si: slot0[r] for si, (r, _) in enumerate(seqs)}
    long = [i for i, (_, n) in enumerate(seqs) if n >= 128][:3]
    if local:
        worst_control("band window - 1", inp, seqs, refs, f16, local, fold, window, "band-1", which=long)
        worst_control("band window + 1", inp, seqs, refs, f16, local, fold, window, "band+1", which=long)
    behind = [i for i, (r, n) in enumerate(seqs) if n % 64 != 0 and n > 1][:4]
    worst_control("key j = S admitted", inp, seqs, refs, f16, local, fold, window, "key_S", which=behind)
    prevs = {}
    for g in g0:   # (row, len, first wave) of the sequence in front of each one in its group
        firsts = [(int(w[0]), int(w[1]), i) for i, w in enumerate(g) if w[1] > 0 and int(w[2]) == i]
        for a, b in zip(firsts, firsts[1:]):
            prevs[[r for r, _ in seqs].index(b[0])] = a
    assert prevs
    worst_control("previous sequence of the group admitted", inp, seqs, refs, f16, local, fold, window, "prev_seq",
                  which=sorted(prevs)[:3], prev=prevs, kbase=kbase)
    worst_control("RoPE partner d + 16", inp, seqs, refs, f16, local, fold, window, "partner16", which=long[:1])
    # q alone at its workgroup-slot position (q and k both shifted is a uniform shift RoPE cannot see: test_short_rotary_table)
    worst_control("q position from the workgroup slot", inp, seqs, refs, f16, local, fold, window, "slot_pos_q",
                  which=sorted(prevs)[:3], kbase=kbase)
    if fold:
        worst_control("mu * s fold term dropped", inp, seqs, refs, f16, local, fold, window, "fold_dropped", which=long[:1])


# ------------------------------------------------------------------ band edges
@gpu
@pytest.mark.parametrize("inst", [i for i in INSTANTIATIONS if i[1] == 1], ids=inst_id)
def test_band_edges(inst):
    f16, _, fold = inst
    rng = np.random.default_rng(300 + 2 * f16 + fold)
    seqs, rows = place([512, 200], rng)
    inp = make_inputs(rng, rows, f16, 1, fold)
    for window in (64, 17, 600):
        o, _, sat = run(inp, seqs, f16, 1, window)
        assert sat == 0
        refs = check(f"band W={window} " + inst_id(inst), inp, seqs, o, f16, 1, fold, window)
        if window == 600:   # wider than the sequence: the banded kernel must equal the global one bit for bit
            og, _, _ = run(inp, seqs, f16, 0, window)
            assert np.array_equal(o, og)
        else:
            worst_control(f"band {window} - 1", inp, seqs, refs, f16, 1, fold, window, "band-1")
            worst_control(f"band {window} + 1", inp, seqs, refs, f16, 1, fold, window, "band+1")


# ------------------------------------------------------------------ short rotary table
@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_short_rotary_table(inst):
    """rope_rows = 17 with S = 17 and rope_rows = 10 with S <= 10: the clamps on table rows 16 b and 0 .. 15.  The sequences sit
    behind a 64-token one in their group (wave slots >= 1): the case that catches a position taken from the workgroup slot."""
    f16, local, fold = inst
    for rope_rows, lengths in ((17, [17, 17, 9, 17]), (10, [10, 10, 3, 8, 10])):
        rng = np.random.default_rng(500 + rope_rows + 4 * f16 + 2 * local + fold)
        seqs, rows = place(lengths, rng)
        inp = make_inputs(rng, rows, f16, local, fold, rope_rows=rope_rows)
        o, groups, sat = run(inp, seqs, f16, local, 64)
        assert sat == 0 and len(groups) == 1
        refs = check(f"rope_rows={rope_rows} " + inst_id(inst), inp, seqs, o, f16, local, fold, 64)
        assert np.all(o[~live_mask(rows, seqs)] == CANARY)
        kbase = {si: si for si in range(len(seqs))}
        assert [int(w[2]) for w in groups[0][:len(seqs)]] == list(range(len(seqs)))
        if rope_rows == 10:   # every shifted position clamps to row 9 + i: a UNIFORM shift again, invisible by RoPE's nature
            continue
        worst_control(f"position from the workgroup slot (rope_rows {rope_rows})", inp, seqs, refs, f16, local, fold, 64,
                      "slot_pos", which=[1, len(seqs) - 1], kbase=kbase)


# ------------------------------------------------------------------ lazy softmax reference
def lazy_inputs(f16, pattern, rng, local):
    """Identity rotary table and selector weights: q / k / v are exact copies of crafted columns of x (q = columns 0..63, k =
    64..127, v = 128..191 for every head), q_scale = 1: the scores are exact, s[i, j] = base(tile of j) + c_i r_j with c_i in
    {1/2, 1, 2} and r_j <= 0 in quarters.  r = 0 at keys 0, 16, 32, 48 and 63 of every tile: every contiguous live part of a
    tile (a band edge, or a 35-key band inside one tile) holds one, so every (row, tile) maximum is base(tile).  Keys 8, 24, 40,
    56 carry the fractional scores; the others sit 40 c_i below.  The global kernel's live part of a tile is the whole tile: there
    key 0 alone has r = 0 and keys 8 and 40 the fractions, so that two or three keys carry a row."""
    S = 512
    x = np.zeros((S, H))
    j = np.arange(S)
    tile = j // 64
    base = {"climb": 7.5 * tile, "climb7": 7.0 * tile, "low_first": np.where(tile == 0, -200.0, 0.0),
            "high_first": np.where(tile == 0, 200.0, 0.0)}[pattern]
    x[:, 0] = 1.0
    x[:, 1] = rng.choice([0.5, 1.0, 2.0], S)
    x[:, 64] = base
    r = np.full(S, -40.0)
    r[((j % 16 == 0) | (j % 64 == 63)) if local else (j % 64 == 0)] = 0.0
    frac = (j % 16 == 8) if local else (j % 32 == 8)
    r[frac] = -0.25 * rng.integers(1, 8, int(frac.sum()))
    x[:, 65] = r
    x[:, 128:] = rng.standard_normal((S, 64))
    return x


@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_lazy_reference(inst):
    """Scores per 64-key tile (a) climbing by 7.5 log2 units: no move, then a move; (b) a first tile 200 below the rest: the
    'first reference far below zero' branch, then alpha flushing to 0; (c) a first tile 200 above the rest.  Banded with window
    17, rows 145 .. 191 of a wave meet their first live key in the wave's SECOND tile.  The fold instantiations run with
    mu = 0, rstd = 1: the operands stay exact.

    (b), (c) and a climb by 7 have integer tile maxima, so every move of the reference is an integer and P = 2^(s - m) rounds
    to 16 bits as 2^frac(s) does, whatever the schedule: there the reference rounds P itself and the bound grants P nothing
    (attend, exact_p).  No P is subnormal in fp16: a key is at most 2 * 1.75 below its tile's maximum when its tile is the
    highest so far, and 200 below (an exact fp32 zero) otherwise.  That is the case that rejects P truncated instead of rounded:
    under the general bound the half ulp granted to P, and the normalisation by the same P, hide it."""
    f16, local, fold = inst
    rng = np.random.default_rng(700 + 2 * f16 + local)
    patterns = ["climb", "climb7", "low_first", "high_first"]
    seqs = [(512 * i, 512) for i in range(len(patterns))]
    x = np.concatenate([lazy_inputs(f16, p, rng, local) for p in patterns])
    rows = len(x)
    w = np.zeros((3 * H, H))
    for part in range(3):
        for head in range(NH):
            w[part * H + head * 64 + np.arange(64), part * 64 + np.arange(64)] = 1.0
    inp = {"x": to16(x, f16), "w": to16(w, f16), "rope_cos": f32(np.ones((512, 32))), "rope_sin": f32(np.zeros((512, 32))),
           "rope_ang": np.zeros((512, 32), np.float32)}
    if fold:
        inp.update(ln_s=f32(w.sum(1)), ln_mu=f32(np.zeros(rows)), ln_rstd=f32(np.ones(rows)))
    assert np.array_equal(from16(inp["x"], f16)[:, :128], x[:, :128])
    for window in ((64, 17) if local else (0,)):
        o, _, sat = run(inp, seqs, f16, local, window, q_scale=1.0)
        assert sat == 0
        case = f"lazy W={window} " + inst_id(inst)
        check(case, inp, seqs[:1], o, f16, local, fold, window, q_scale=1.0, exact=True)
        refs = check(case + " exact P", inp, seqs[1:], o, f16, local, fold, window, q_scale=1.0, exact=True, exact_p=True)
        if local and window != 17:
            continue   # the narrow band (or the global kernel) is the case meant to catch it: few keys carry the row
        worst_control(f"P truncated instead of rounded (W={window})", inp, seqs[1:], refs, f16, local, fold, window, "p_trunc",
                      q_scale=1.0, exact=True, exact_p=True)


# ------------------------------------------------------------------ garbage rows, the O canary, fp16 saturation
@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_garbage_rows_do_not_leak(inst):
    """Every row of x, ln_mu and ln_rstd that belongs to no sequence -- the rows behind each sequence inside its last wave
    included -- holds large finite values instead of zeros: same live bits, same clamp flag, canary intact."""
    f16, local, fold = inst
    rng = np.random.default_rng(900 + 4 * f16 + 2 * local + fold)
    seqs, rows = place([200, 1, 65, 130, 449, 17, 320], rng)
    inp = make_inputs(rng, rows, f16, local, fold, sharp=2.0)   # softer attention: where a dropped q_scale shows most
    live = live_mask(rows, seqs)
    big = 3e4 if f16 else 1e8
    outs = []
    for fill in (0.0, big):
        cur = dict(inp)
        x = from16(inp["x"], f16)
        x[~live] = fill * np.sign(rng.standard_normal((int((~live).sum()), H)) + 0.5)
        cur["x"] = to16(x, f16)
        if fold:
            cur["ln_mu"], cur["ln_rstd"] = inp["ln_mu"].copy(), inp["ln_rstd"].copy()
            cur["ln_mu"][~live] = fill
            cur["ln_rstd"][~live] = fill
        for packer in (0, 1):
            outs.append(run(cur, seqs, f16, local, 64, packer=packer))
    o0, _, sat0 = outs[0]
    assert sat0 == 0
    refs = check("garbage " + inst_id(inst), inp, seqs, o0, f16, local, fold, 64)
    worst_control("q_scale dropped", inp, seqs, refs, f16, local, fold, 64, "q_scale", which=[0, 4])
    for o, _, sat in outs[1:]:
        assert np.array_equal(o, o0) and sat == sat0
    assert np.all(o0[~live] == CANARY)


@gpu
@pytest.mark.parametrize("local,fold", [(0, False), (1, True)])
def test_f16_saturation_clamps_and_flags(local, fold):
    rng = np.random.default_rng(11 + local)
    seqs, rows = place([130, 65], rng)
    inp = make_inputs(rng, rows, True, local, fold, sharp=1.0)
    x = from16(inp["x"], True)
    x[seqs[0][0] + 70] = 3e4 * np.sign(from16(inp["w"], True)[2 * H + 5])   # a LIVE row: v[70, 5] of head 0 leaves fp16's range
    inp["x"] = to16(x, True)
    if fold:
        inp["ln_mu"][:] = 0
        inp["ln_rstd"][:] = 1
    o, _, sat = run(inp, seqs, True, local, 64)
    assert sat == 1
    live = live_mask(rows, seqs)
    assert np.all(np.isfinite(from16(o[live], True)))
    assert np.all(o[~live] == CANARY)


# ------------------------------------------------------------------ refusals (argument checks come before any GPU call)
def test_refusals():
    """Each refused shape returns the argument error and launches nothing: o keeps its canary everywhere."""
    rng = np.random.default_rng(5)
    rows = 512
    good = [(0, 100), (128, 200)]
    inp = make_inputs(rng, rows, False, 0, True)

    def refused(seqs=good, drop=None, use=inp, **override):
        cur = {k: v for k, v in use.items() if k != drop}
        status, o, _, _ = raw_run(cur, seqs, False, 0, 64, **override)
        assert status == -1, (status, seqs, drop, override)
        assert np.all(o == CANARY)
        msg = _lib.load_debug().vrag_last_error()
        assert msg

    for name in ("x", "w", "rope_cos", "ln_s", "ln_rstd"):
        refused(drop=name)
    for name in ("rope_sin", "o", "seq_row", "seq_len", "groups_out"):
        refused(null=(name,))
    refused(H=128)                                     # H != 64 * nh
    refused(nh=2)
    refused(seqs=[(0, 0)])
    refused(seqs=[(0, 513)])
    refused(seqs=[(4, 100)])                           # seq_row % 8
    refused(seqs=[(0, 100), (96, 50)])                 # overlap
    refused(seqs=[(128, 50), (0, 129)])                # overlap, list order against buffer order
    refused(seqs=[(456, 50)])                          # 456 + 64 > 512: the wave reads 64 whole rows
    refused(seqs=[(0, 100), (448, 65)])                # 448 + 128 > 512
    small = {k: (v[:384] if k in ("x", "ln_mu", "ln_rstd") else v) for k, v in inp.items()}
    refused(seqs=[(0, 100)], use=small)                # rows % 256


# ------------------------------------------------------------------ the packers on the host
def test_packers_on_random_length_lists():
    rng = np.random.default_rng(77)
    for trial in range(300):
        n = int(rng.integers(1, 41))
        lens = rng.integers(1, 513, n) if trial % 3 else rng.choice([1, 63, 64, 65, 128, 448, 449, 512], n)
        rows = np.cumsum(np.concatenate([[0], (lens[:-1] + 7) // 8 * 8 + rng.integers(0, 4, n - 1) * 8]))
        perm = rng.permutation(n)
        lens, rows = lens[perm], rows[perm]
        count = []
        for packer in (0, 1):
            g = pack(rows, lens, packer)
            count.append(len(g))
            seen = defaultdict(list)
            for gi, grp in enumerate(g):
                for wi, (x, y, z, w) in enumerate(grp):
                    assert w == 0
                    if y == 0:
                        assert x == 0 and z == 0, "an unused wave is all-zero"
                        continue
                    assert 0 <= z <= wi < 8
                    seen[int(x) - 64 * (wi - int(z))].append((gi, wi, int(x), int(y), int(z)))
            assert sorted(seen) == sorted(int(r) for r in rows)
            for r, ln in zip(rows, lens):
                ws = seen[int(r)]
                need = -(-int(ln) // 64)
                assert len(ws) == need and len({gi for gi, *_ in ws}) == 1, "exactly once, in one group"
                z = ws[0][1]
                for j, (gi, wi, x, y, zz) in enumerate(sorted(ws, key=lambda t: t[1])):
                    assert (wi, x, y, zz) == (z + j, int(r) + 64 * j, int(ln), z)
            assert g.shape[1] == 8
        assert count[1] <= count[0], "best fit decreasing used more groups than first fit"
        assert count[1] >= -(-int(((lens + 63) // 64).sum()) // 8)


def test_pack_groups_refuses_bad_lengths():
    dbg = _lib.load_debug()
    out = np.zeros((2, 8, 4), np.int32)
    row = np.array([0, 512], np.int32)
    for bad in ([0, 5], [5, 513]):
        ln = np.array(bad, np.int32)
        assert dbg.vrag_debug_pack_groups(row.ctypes.data, ln.ctypes.data, 2, 0, out.ctypes.data) == -1
    ln = np.array([5, 6], np.int32)
    assert dbg.vrag_debug_pack_groups(row.ctypes.data, ln.ctypes.data, 2, 2, out.ctypes.data) == -1
    assert dbg.vrag_debug_pack_groups(None, ln.ctypes.data, 2, 0, out.ctypes.data) == -1


# ------------------------------------------------------------------ the -rP table
@gpu
def test_zz_worst_ratios():
    print("\nworst error / bound per case, and its (row mod 64) classes: min / median / max, the class of the max")
    for (form, _, f16), r in sorted(_WORST.items(), key=lambda kv: kv[0][0]):
        cls = _CLASS.get(form)
        tail = ""
        if cls is not None:
            tail = f"   classes {cls.min():.3f} / {np.median(cls):.3f} / {cls.max():.3f} @ {int(cls.argmax())}"
        print(f"  {form:<64s} {r:10.3f}{tail}")
    for form, cls in _CLASS.items():
        # a fragment-mapping slip shows as one class standing out: every class stays under the bound, so assert only that
        assert cls.max() <= 1.0, (form, int(cls.argmax()), float(cls.max()))
