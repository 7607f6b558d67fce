"""The standalone attention kernel ALONE (vrag_debug_attn_run_ex, csrc/attention.hip: attn_fwd_kernel, global and banded, bf16
and fp16) against its stated arithmetic in float64, on the SAME 16-bit operand bits the kernel reads, on the layout the encoder
packs: ragged lengths at 8-aligned rows, gaps and neighbours, finite garbage in every row and column outside the sequences.
Every live row of every sequence and head is referenced.

Reference per (sequence, head): scores q . k^T in log2 units (q already carries head_dim^-1/2 * log2 e); mask j < S and, banded,
|i - j| <= window; exp2 softmax; P . V.  (attn_ref.attend, kernel="attention".)

Bound, per output element (never tuned to what the kernel returns; U = 2^-24, u16 = 2^-8 bf16 / 2^-11 fp16, half an ulp of a
16-bit value relative to it).  q, k and v are the kernel's exact operands: E_q = E_k = E_v = 0.  That alone does not turn the
fused kernel's bound into this one's, because the arithmetic differs in three places:
  scores       64 products (exact in fp32) accumulated from ZERO by four MFMAs: 64 U (|q| . |k|^T), doubled for the MFMA's
               internal order: E_s = 2 * 64 U (|q| . |k|^T).  No reference rides in the accumulator.
  P            pv = exp2(s - m): the subtraction rounds once, U |s - m| in the exponent; v_exp_f32 is good to one ulp, 2 U:
               eta = 2^(E_s + U |s - m|) - 1 + 2 U, relative, on the fp32 P.  m is the row's own running maximum (each lane
               reduces ITS row, plus one cross-half exchange), exact per row: P <= 1, the row's largest P is 1 and the row
               sum is >= 1.  A masked key is an exact zero.
  P rounding   the row sum adds the fp32 pv, the P . V MFMA reads (T)pv.  In the fused kernel the same rounded P feeds both
               and a common factor cancels; here it does NOT: with pv_j (1 + delta_j) the 16-bit P,
                 o~ - o = [sum_j w_j eta_j (v_j - o) + sum_j w_j (1 + eta_j) delta_j v_j] / (1 + sum_j w_j eta_j),
               |delta_j| <= u16 and uncentred: the second sum is granted whole, u16 sum_j w_j (1 + eta_j) |v_j|.  A constant V
               does not come back exact (test_constant_v measures that term alone).  fp16 P below 2^-14 is subnormal: 2^-25
               absolute per key against a row sum >= 1 (in the units of an earlier tile P is LARGER, so 2^-25 there is at most
               2^-25 in the final units); a bf16 / fp32 P below 2^-126 flushes: 2^-126 per key.
  output       / (1 - A), A = sum_j w_j eta_j; fp32 accumulation of P . V: a product passes at most 64 additions inside its
               tile and, per later tile, one rescale multiply and four MFMA accumulations: (64 + 5 n_t) U sum_j w_j |v_j|,
               doubled as above; the row sum: at most 32 in-lane additions, per tile one multiply and one add (alpha is the
               SAME value for l and O: its own error cancels), the cross-half add: (34 + 2 n_t) U |o|; 1 / l and the final
               multiply 4 U |o|: together (38 + 2 n_t) U |o|; n_t = ceil(S / 64), at least the 64-key tiles a row meets;
               + half an ulp of the stored output.
No constant of the bound was measured.

Negative controls (float64 references with one defect, computed on the CPU, so they run without a GPU; each must exceed the
bound 10 x on its named case): band W - 1, band W + 1, key j = S admitted (the garbage row behind the sequence), key j = -1
admitted (the row in front), one 32-key half dropped at a band edge (the half that holds key q_lo + 31 + W of a 32-row
sub-tile), P truncated instead of rounded, the row sum built from the rounded P (the fused kernel's arithmetic: that control
proves the bound models THIS kernel).  The two P-rounding controls cannot reach 10 x under the general bound and get a crafted
case, as test_lazy_reference of the fused suite does:
  * the general bound grants P its half ulp, which is all a truncation costs.  test_exact_p crafts scores in quarters with integer
    tile maxima (exact in fp32; every move of the reference an integer), so the 16-bit P is predictable bit for bit: there the
    reference rounds P itself, in the units of P's own tile, and the bound grants P nothing;
  * the row sum from the rounded P changes a whole output row by one relative factor <= u16, and the stored output's own half
    ulp is >= u16 / 2 relative: NO 16-bit output can show it 10 x over a bound that grants the store half an ulp.  With the
    exact P of that crafted case the value to be stored is known to fp32 accuracy; where its fp32 error interval (doubled)
    holds no rounding tie of the 16-bit format the stored BITS are predictable: there the reference is the rounded value and
    the bound the fp32 terms alone (attend_standalone, exact_o).  The fused kernel's arithmetic moves some stored values
    across a tie, a whole ulp against a bound of a few hundred U, and is rejected.  (A V constant over the keys does not serve:
    the constant is itself a 16-bit value, half an ulp from the nearest tie, further than the factor <= u16 can move it.)

`-rP` prints the worst error / bound ratio per case and per (row mod 64) class.  Measured on an MI355X: see MEASURED below."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib
from attn_ref import attend
from unit16 import from16, make_ledger, to16

gpu = pytest.mark.gpu

MEASURED = """NOT MEASURED: no MI355X run of this module has been recorded yet (`-rP` prints the table: worst error / bound per case and
instantiation, the (row mod 64) classes, the constant-V ratio).  Controls, smallest ratio over the instantiations that run them
(CPU): band W - 1 / + 1 3130 / 3123 (W = 64), 44315 / 8619 (W = 17), band 0 + 1 2.1e6, key j = S 2901, key j = -1 1789, 32-key half
dropped 20337, P truncated 60 (fp16) / 667 (bf16), row sum from the rounded P 27 (fp16) / 483 (bf16)."""

H, NH = 192, 3            # three heads, a head stride that is no power of two
Q_SCALE = float(np.float32(0.125 * 1.4426950408889634))
SHARP = 6.0               # unit-variance q and k, q times 6: the hard case of test_attention_unit_gpu.py
CANARY = 0x7A5C
QB = 256                  # attention_q_block, global and banded
_WORST, record, control = make_ledger()
_CLASS = defaultdict(lambda: np.zeros(64))                   # case -> worst ratio per (row mod 64)
_CLASS_SUM = defaultdict(lambda: np.zeros((2, 64)))          # case -> (sum of ratios, count) per (row mod 64)
INSTANTIATIONS = [(f16, local) for f16 in (False, True) for local in (0, 1)]
_ZERO = np.zeros((1, 1))


def inst_id(v):
    f16, local = v
    return f"{'fp16' if f16 else 'bf16'}-{'banded' if local else 'global'}"


# ------------------------------------------------------------------ the hook
def expected_blocks(seqs):
    """The q-block descriptors of capi.hip's layout loop: one per QB rows of each sequence, in list order."""
    return np.asarray([(r, n, q0) for r, n in seqs for q0 in range(0, n, QB)], np.int32).reshape(-1, 3)


def raw_run(inp, seqs, f16, local, window, o=None, null=(), **override):
    """One launch; returns (status, o bits [rows, H], blocks [n_blocks, 3], f16_saturated)."""
    dbg = _lib.load_debug()
    a = _lib.DebugAttnArgs()
    rows = inp["q"].shape[0]
    o = np.full((rows, H), CANARY, np.uint16) if o is None else o
    seq_row = np.ascontiguousarray([r for r, _ in seqs], np.int32)
    seq_len = np.ascontiguousarray([n for _, n in seqs], np.int32)
    cap = int(sum(-(-max(int(n), 1) // QB) for n in seq_len))
    blocks = np.full((cap, 3), -7, np.int32)
    keep = [o, seq_row, seq_len, blocks]
    for name in ("q", "k", "vt"):
        assert inp[name].flags.c_contiguous and inp[name].dtype == np.uint16, name
        setattr(a, name, inp[name].ctypes.data)
    a.o, a.seq_row, a.seq_len, a.blocks_out = o.ctypes.data, seq_row.ctypes.data, seq_len.ctypes.data, blocks.ctypes.data
    a.rows, a.H, a.n_seqs, a.local, a.window, a.f16, a.blocks_cap = rows, H, len(seqs), local, window, int(f16), cap
    a.n_blocks, a.f16_saturated = -1, -1
    for k, v in override.items():
        setattr(a, k, v)
    for k in null:
        setattr(a, k, None)
    status = dbg.vrag_debug_attn_run_ex(C.byref(a), 0)
    del keep
    return status, o, blocks[:max(a.n_blocks, 0)], a.f16_saturated


def run(inp, seqs, f16, local, window):
    status, o, blocks, sat = raw_run(inp, seqs, f16, local, window)
    if status == -2:   # VRAG_ERR_HIP: a failed launch or a clobbered canary: nothing more goes onto this device
        msg = _lib.load_debug().vrag_last_error()
        pytest.exit(f"vrag_debug_attn_run_ex: {msg.decode() if msg else status}", returncode=3)
    _lib.check_debug("vrag_debug_attn_run_ex", status)
    assert np.array_equal(blocks, expected_blocks(seqs))
    return o, blocks, sat


# ------------------------------------------------------------------ operands
def place(lengths, rng, gaps=(0, 8, 24, 72), tail=0):
    """Rows for the sequences: buffer order shuffled against list order, 8-aligned, with gaps.  Returns (seqs, rows)."""
    order = rng.permutation(len(lengths))
    row, cur = [0] * len(lengths), int(rng.choice(gaps))
    for i in order:
        row[i] = cur
        cur += -(-lengths[i] // 8) * 8 + int(rng.choice(gaps))
    need = max(r + n for r, n in zip(row, lengths)) + tail
    return list(zip(row, lengths)), -(-need // 256) * 256


def live_mask(rows, seqs):
    m = np.zeros(rows, bool)
    for r, n in seqs:
        m[r:r + n] = True
    return m


def make_inputs(rng, rows, seqs, f16, sharp=SHARP, garbage=1.0):
    """Unit-variance q, k, v in EVERY row (the rows outside the sequences included: the kernel must mask them), the live q rows
    times sharp * q_scale.  garbage: the magnitude of the rows outside the sequences (1 = unit variance; else +- that value)."""
    live = live_mask(rows, seqs)
    q, k, v = (rng.standard_normal((rows, H)) for _ in range(3))
    q[live] *= sharp * Q_SCALE
    if garbage != 1.0:
        for x in (q, k, v):
            x[~live] = garbage * np.sign(x[~live])
    return {"q": to16(q, f16), "k": to16(k, f16), "vt": np.ascontiguousarray(to16(v, f16).T)}


def transplant(src, src_seqs, rng, rows, seqs, f16, garbage):
    """The SAME sequence bits at other rows among other garbage."""
    inp = make_inputs(rng, rows, seqs, f16, garbage=garbage)
    for (r0, n), (s0, m) in zip(seqs, src_seqs):
        assert n == m
        inp["q"][r0:r0 + n], inp["k"][r0:r0 + n] = src["q"][s0:s0 + n], src["k"][s0:s0 + n]
        inp["vt"][:, r0:r0 + n] = src["vt"][:, s0:s0 + n]
    return inp


# ------------------------------------------------------------------ float64 reference and bound
def reference(inp, seq, head, f16, local, window, defect=None, **kw):
    """(ref, bound) [S, 64] of one (sequence, head); `defect` names the one wrong step of a negative control."""
    r0, S = seq
    hs = slice(head * 64, head * 64 + 64)
    tok = np.arange(S)
    keys, S_eff, win = tok, S, window
    if defect == "band-1":
        win = window - 1
    if defect == "band+1":
        win = window + 1
    if defect == "key_S":       # the garbage row behind the sequence let through
        keys, S_eff = np.arange(S + 1), S + 1
    if defect == "key_-1":      # the row in front of the sequence let through
        keys = np.arange(-1, S)
    if defect == "half_dropped":   # the 32-key half that holds key q_lo + 31 + W of each 32-row sub-tile is skipped
        kw["drop"] = (keys[None, :] // 32) == ((32 * (tok // 32) + 31 + window) // 32)[:, None]
    if defect == "p_trunc":
        kw["exact_p"] = "trunc"
    if defect == "psum16":
        kw["psum16"] = True
    q = from16(inp["q"][r0:r0 + S, hs], f16)
    k = from16(inp["k"][r0 + keys, hs], f16)
    v = from16(inp["vt"][hs, r0 + keys].T, f16)
    return attend(q, _ZERO, k, _ZERO, v, _ZERO, tok, keys, S_eff, local, win, f16, strict=defect is None, kernel="attention", **kw)


def check(case, inp, seqs, o, f16, local, window, **kw):
    """Every row of every sequence and head against the reference; returns {(seq index, head): (ref, bound)}."""
    out = {}
    for si, (r0, S) in enumerate(seqs):
        for head in range(NH):
            ref, bound = reference(inp, (r0, S), head, f16, local, window, **kw)
            got = from16(o[r0:r0 + S, head * 64:(head + 1) * 64], f16)
            ratio = np.abs(got - ref) / bound
            np.maximum.at(_CLASS[case], np.arange(S) % 64, ratio.max(1))
            np.add.at(_CLASS_SUM[case][0], np.arange(S) % 64, ratio.mean(1))
            np.add.at(_CLASS_SUM[case][1], np.arange(S) % 64, 1.0)
            record(case, None, f16, got, ref, bound)
            out[(si, head)] = (ref, bound)
    return out


def worst_control(name, inp, seqs, f16, local, window, defect, which, heads=range(NH), **kw):
    """The defect's worst ratio over the given sequences, through the ledger's control()."""
    best, arg = -1.0, None
    for si in which:
        for head in heads:
            ref, bound = reference(inp, seqs[si], head, f16, local, window, **kw)
            wrong, _ = reference(inp, seqs[si], head, f16, local, window, defect=defect, **kw)
            r = float((np.abs(wrong - ref) / bound).max())
            if r > best:
                best, arg = r, (wrong, ref, bound)
    assert arg is not None, name
    return control(f"{name} [{inst_id((f16, local))}]", *arg)


# ------------------------------------------------------------------ ragged layout, all four instantiations
# on and off the 8-row, the 32-row sub-tile, the 64-key tile and the 256-row block grid; 64, 200, 512, 1000 are the lengths of
# test_attention_unit_gpu.py
RAGGED = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 129, 191, 193, 255, 256, 257, 300, 449, 513, 1000, 200, 512]
WINDOW = 64


def ragged_layout():
    return place(RAGGED, np.random.default_rng(2026))


def ragged_inputs(f16, local):
    seqs, rows = ragged_layout()
    return make_inputs(np.random.default_rng(100 + 2 * f16 + local), rows, seqs, f16), seqs, rows


def assert_reached(blocks, local, window):
    """What the ragged case is there to reach, on the descriptors that ran (the wave and tile arithmetic of attn_fwd_kernel)."""
    blocks = [tuple(int(x) for x in b) for b in blocks]
    assert any(S == 257 and q0 == 256 for _, S, q0 in blocks), "no one-row second q-block"
    inactive = set()
    for _, S, q0 in blocks:   # a wave is inactive when its first query row is dead: qw0 = q0 + 64 w global, q0 + 32 w banded
        step = 32 if local else 64
        inactive.add(sum(q0 + step * w >= S for w in range(4)))
    assert inactive >= {0, 1, 2, 3}, inactive
    assert any(S % 64 not in (0,) and S - q0 < QB for _, S, q0 in blocks), "no dead query rows inside a live wave"
    assert any(S % 8 for _, S, _ in blocks) and any(S % 32 == 1 for _, S, _ in blocks)
    tiles = []
    for _, S, q0 in blocks:
        lo, hi = (max(0, q0 - window) >> 6, min(S - 1, q0 + QB - 1 + window) >> 6) if local else (0, (S - 1) >> 6)
        tiles.append((lo, hi))
    assert any(hi - lo >= 3 for lo, hi in tiles), "the 3-slot ring never wraps"
    if local:
        assert {lo % 3 for lo, hi in tiles} == {0, 1, 2}, "a banded block's first tile never sits in some ring slot"
        assert [lo for (_, S, _), (lo, _) in zip(blocks, tiles) if S == 1000] == [0, 3, 7, 11]
    assert {t0 % 64 for t0, _, _ in blocks} == set(range(0, 64, 8)), "some t0 mod 64 is never used"


def test_ragged_layout_reaches_every_branch():
    seqs, rows = ragged_layout()
    assert rows <= 6144 and set(RAGGED) >= {64, 200, 512, 1000}
    order = np.argsort([r for r, _ in seqs])
    assert list(order) != sorted(order), "buffer order equals list order"
    gaps = {seqs[b][0] - (seqs[a][0] + -(-seqs[a][1] // 8) * 8) for a, b in zip(order, order[1:])}
    assert gaps == {0, 8, 24, 72}, gaps
    for local in (0, 1):
        assert_reached(expected_blocks(seqs), local, WINDOW)


def no_class_stands_out(case):
    """test_attention_unit_gpu.py's rule (no class above twice the mean), on error / bound ratios per (row mod 64)."""
    s, n = _CLASS_SUM[case]
    assert np.all(n > 0)
    per = s / n
    assert per.max() < 2.0 * s.sum() / n.sum(), (case, int(per.argmax()), per.round(3).tolist())


@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_ragged(inst):
    f16, local = inst
    inp, seqs, rows = ragged_inputs(f16, local)
    o, blocks, sat = run(inp, seqs, f16, local, WINDOW)
    assert_reached(blocks, local, WINDOW)
    assert sat == 0, "a dead row or an inactive wave set the fp16 clamp word"
    case = "ragged " + inst_id(inst)
    check(case, inp, seqs, o, f16, local, WINDOW)
    assert np.all(o[~live_mask(rows, seqs)] == CANARY), "the kernel wrote a row outside the sequences"
    no_class_stands_out(case)


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_ragged_controls(inst):
    f16, local = inst
    inp, seqs, _ = ragged_inputs(f16, local)
    at = {n: i for i, n in enumerate(RAGGED)}
    some = [at[n] for n in (33, 129, 300)]
    worst_control("key j = S admitted", inp, seqs, f16, local, WINDOW, "key_S", which=[at[n] for n in (7, 33, 65, 129)])
    assert all(seqs[i][0] > 0 for i in some)
    worst_control("key j = -1 admitted", inp, seqs, f16, local, WINDOW, "key_-1", which=some)
    if local:
        worst_control("band W - 1", inp, seqs, f16, local, WINDOW, "band-1", which=[at[300]])
        worst_control("band W + 1", inp, seqs, f16, local, WINDOW, "band+1", which=[at[300]])
        worst_control("32-key half dropped at the band edge", inp, seqs, f16, local, WINDOW, "half_dropped", which=[at[300]])


# ------------------------------------------------------------------ end of the buffer: all three address clamps bite
END_CASES = [(33, 40), (40, 40), (300, 304), (304, 304)]    # (length, rows - first row)


def end_inputs(f16, local, S, back):
    rows = 512
    seqs = [(0, 65), (rows - back, S)]
    assert seqs[1][0] % 8 == 0 and rows - 8 <= seqs[1][0] + S <= rows and seqs[1][0] + 64 * -(-S // 64) > rows
    return make_inputs(np.random.default_rng(40 + 2 * f16 + local + S), rows, seqs, f16), seqs, rows


@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_end_of_buffer(inst):
    """The last sequence ends on (or within 8 rows of) row rows - 1: its last 64-key tile runs past Tp, so the Q, K and V^T
    clamps all bite; the hook's canary behind o answers for the stores."""
    f16, local = inst
    for S, back in END_CASES:
        inp, seqs, rows = end_inputs(f16, local, S, back)
        o, _, sat = run(inp, seqs, f16, local, WINDOW)
        assert sat == 0
        check(f"end of buffer S={S} " + inst_id(inst), inp, seqs, o, f16, local, WINDOW)
        assert np.all(o[~live_mask(rows, seqs)] == CANARY)


# ------------------------------------------------------------------ band edges
BAND_LENGTHS = [31, 32, 33, 63, 64, 65, 95, 96, 97, 129, 200]
BAND_WINDOWS = (0, 17, 64, 600)


def band_inputs(f16):
    rng = np.random.default_rng(300 + f16)
    seqs, rows = place(BAND_LENGTHS, rng)
    return make_inputs(rng, rows, seqs, f16), seqs, rows


@gpu
@pytest.mark.parametrize("f16", (False, True), ids=("bf16", "fp16"))
def test_band_edges(f16):
    inp, seqs, rows = band_inputs(f16)
    for window in BAND_WINDOWS:
        o, _, sat = run(inp, seqs, f16, 1, window)
        assert sat == 0
        check(f"band W={window} " + inst_id((f16, 1)), inp, seqs, o, f16, 1, window)
        assert np.all(o[~live_mask(rows, seqs)] == CANARY)
        if window == 0:   # every row returns its own V row: P = 1 and l = 1 exactly, the store rounds nothing
            for r0, S in seqs:
                assert np.array_equal(o[r0:r0 + S], inp["vt"][:, r0:r0 + S].T)


@pytest.mark.parametrize("f16", (False, True), ids=("bf16", "fp16"))
def test_band_edge_controls(f16):
    inp, seqs, _ = band_inputs(f16)
    which = [BAND_LENGTHS.index(n) for n in (97, 200)]
    for window in (0, 17, 64):
        if window:
            worst_control(f"band {window} - 1", inp, seqs, f16, 1, window, "band-1", which=which)
            worst_control(f"half dropped at the band edge (W={window})", inp, seqs, f16, 1, window, "half_dropped", which=which)
        worst_control(f"band {window} + 1", inp, seqs, f16, 1, window, "band+1", which=which)


# ------------------------------------------------------------------ neighbours do not leak
LEAK_LENGTHS = [200, 1, 65, 130, 449, 33, 300, 7]


@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_neighbours_do_not_leak(inst):
    """The same sequence bits at two placements (other t0 mod 64, other neighbours), and once among garbage rows at the format's
    large finite values (+-65504 fp16, +-2^100 bf16) in q, k and V^T: bit-identical live rows, canary intact, no clamp flag."""
    f16, local = inst
    rng = np.random.default_rng(900 + 2 * f16 + local)
    seqs_a, rows_a = place(LEAK_LENGTHS, rng)
    for _ in range(100):
        seqs_b, rows_b = place(LEAK_LENGTHS, rng, tail=256)
        if sum(a[0] % 64 != b[0] % 64 for a, b in zip(seqs_a, seqs_b)) >= 6:
            break
    else:
        raise AssertionError("no second placement with other t0 mod 64")
    big = 65504.0 if f16 else 2.0 ** 100
    base = make_inputs(rng, rows_a, seqs_a, f16)
    runs = [(base, seqs_a, rows_a), (transplant(base, seqs_a, rng, rows_b, seqs_b, f16, 1.0), seqs_b, rows_b),
            (transplant(base, seqs_a, rng, rows_a, seqs_a, f16, big), seqs_a, rows_a),
            (transplant(base, seqs_a, rng, rows_b, seqs_b, f16, big), seqs_b, rows_b)]
    outs = []
    for i, (inp, seqs, rows) in enumerate(runs):
        o, _, sat = run(inp, seqs, f16, local, WINDOW)
        assert sat == 0, "garbage rows set the fp16 clamp word"
        assert np.all(o[~live_mask(rows, seqs)] == CANARY)
        outs.append([o[r0:r0 + n] for r0, n in seqs])
        if i == 0:
            check("neighbours " + inst_id(inst), inp, seqs, o, f16, local, WINDOW)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(a, b), "a sequence's bits depend on where it sits or on what lies beside it"


# ------------------------------------------------------------------ constant V: the P-rounding term alone
@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_constant_v(inst):
    """V constant over the keys of every sequence (per head and dimension): the reference returns the constant, and all that
    remains of the error is sum_j w_j delta_j c, the 16-bit rounding of P that the fp32 row sum does not share."""
    f16, local = inst
    rng = np.random.default_rng(1200 + 2 * f16 + local)
    seqs, rows = place([257, 65, 300, 9, 130], rng)
    inp = make_inputs(rng, rows, seqs, f16)
    c = to16(rng.standard_normal(H), f16)
    for r0, n in seqs:
        inp["vt"][:, r0:r0 + n] = c[:, None]
    o, _, sat = run(inp, seqs, f16, local, WINDOW)
    assert sat == 0
    refs = check("constant V " + inst_id(inst), inp, seqs, o, f16, local, WINDOW)
    for (si, head), (ref, _) in refs.items():
        assert np.allclose(ref, from16(c[head * 64:head * 64 + 64], f16)[None, :], rtol=1e-12, atol=0)


# ------------------------------------------------------------------ predictable P: rounding, and which P feeds the row sum
EXACT_PATTERNS = ["climb7", "low_first", "high_first"]


def exact_inputs(f16, local):
    """q = (c_i, 1, 0, ...), k = (r_j, base(tile of j), 0, ...): s[i, j] = c_i r_j + base, exact in fp32; c_i in {1/2, 1, 2},
    r_j <= 0 in quarters.  r = 0 at keys 0, 16, 32, 48 and 63 of every tile (banded: every contiguous live part of a tile holds
    one; global: key 0 alone), so every (row, tile) maximum is base(tile), an integer.  Keys 8, 24, 40, 56 (global: 8 and 40)
    carry the fractional scores, the others sit 40 c_i below."""
    rng = np.random.default_rng(700 + 2 * f16 + local)
    S = 512
    seqs = [(S * i, S) for i in range(len(EXACT_PATTERNS))]
    rows = S * len(seqs)
    q, k = np.zeros((rows, H)), np.zeros((rows, H))
    j = np.arange(S)
    tile = j // 64
    for (r0, _), pattern in zip(seqs, EXACT_PATTERNS):
        base = {"climb7": 7.0 * tile, "low_first": np.where(tile == 0, -200.0, 0.0), "high_first": np.where(tile == 0, 200.0, 0.0)}[pattern]
        r = np.full(S, -40.0)
        r[((j % 16 == 0) | (j % 64 == 63)) if local else (j % 64 == 0)] = 0.0
        frac = (j % 16 == 8) if local else (j % 32 == 8)
        r[frac] = -0.25 * rng.integers(1, 8, int(frac.sum()))
        for h in range(NH):
            q[r0:r0 + S, 64 * h] = rng.choice([0.5, 1.0, 2.0], S)
            q[r0:r0 + S, 64 * h + 1] = 1.0
            k[r0:r0 + S, 64 * h] = r
            k[r0:r0 + S, 64 * h + 1] = base
    v = rng.standard_normal((rows, H))
    inp = {"q": to16(q, f16), "k": to16(k, f16), "vt": np.ascontiguousarray(to16(v, f16).T)}
    assert np.array_equal(from16(inp["q"], f16), q) and np.array_equal(from16(inp["k"], f16), k)
    return inp, seqs


EXACT_WINDOW = 17


@gpu
@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_exact_p(inst):
    """The crafted case whose 16-bit P is predictable (module docstring): the kernel must ROUND P, in the units of P's tile, and
    build the row sum from the fp32 P.  Checked twice on the same output: under the bound that grants the store its half ulp,
    and with the stored bits predicted wherever no rounding tie lies inside the fp32 error interval."""
    f16, local = inst
    inp, seqs = exact_inputs(f16, local)
    o, _, sat = run(inp, seqs, f16, local, EXACT_WINDOW)
    assert sat == 0
    check("exact P " + inst_id(inst), inp, seqs, o, f16, local, EXACT_WINDOW, exact_p="round")
    check("exact P, exact store " + inst_id(inst), inp, seqs, o, f16, local, EXACT_WINDOW, exact_p="round", exact_o=True)


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=inst_id)
def test_exact_p_controls(inst):
    f16, local = inst
    inp, seqs = exact_inputs(f16, local)
    worst_control("P truncated instead of rounded", inp, seqs, f16, local, EXACT_WINDOW, "p_trunc", which=[0, 1, 2],
                  exact_p="round", exact_o=True)
    worst_control("row sum built from the rounded P", inp, seqs, f16, local, EXACT_WINDOW, "psum16", which=[0, 1, 2],
                  exact_p="round", exact_o=True)


# ------------------------------------------------------------------ refusals (argument checks come before any GPU call)
def test_refusals():
    """Each refused shape returns the argument error with a message of its own and launches nothing: o keeps its canary."""
    rng = np.random.default_rng(5)
    rows = 512
    good = [(0, 100), (128, 200)]
    inp = make_inputs(rng, rows, good, False)
    seen = set()

    def refused(seqs=good, use=inp, local=0, window=64, **kw):
        status, o, _, _ = raw_run(use, seqs, False, local, window, **kw)
        assert status == -1, (status, seqs, kw)
        assert np.all(o == CANARY)
        msg = _lib.load_debug().vrag_last_error()
        assert msg
        seen.add(msg.decode().split("(")[0].split("[")[0].rstrip("0123456789 -"))

    for name in ("q", "k", "vt", "o", "seq_row", "seq_len"):
        refused(null=(name,))
    refused(H=160)                                     # H % 64
    small = {k: (v[:384] if k != "vt" else np.ascontiguousarray(v[:, :384])) for k, v in inp.items()}
    refused(seqs=[(0, 100)], use=small)                # rows % 256
    refused(seqs=[(0, 0)])                             # seq_len < 1
    refused(seqs=[(4, 100)])                           # seq_row % 8
    refused(seqs=[(-8, 100)])
    refused(seqs=[(416, 97)])                          # 416 + 97 > 512
    refused(seqs=[(0, 100), (96, 50)])                 # overlap
    refused(seqs=[(128, 50), (0, 129)])                # overlap, list order against buffer order
    refused(local=1, window=-1)
    refused(blocks_cap=1)                              # blocks_out too small
    assert len(seen) >= 9, seen                        # each refusal speaks for itself
    status, o, blocks, _ = raw_run(inp, [(472, 40)], False, 0, 64, null=("q", "k", "vt"))   # the last row is allowed: only the nulls refuse
    assert status == -1 and np.all(o == CANARY)


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
        assert cls.max() <= 1.0, (form, int(cls.argmax()), float(cls.max()))
