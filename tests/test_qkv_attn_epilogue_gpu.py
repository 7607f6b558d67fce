"""The fused kernel's epilogue (csrc/qkv_attn.hip section 2: fold, RoPE, K / V^T to LDS, Q to registers) at the places where
keeping every table value in registers for all of its uses, and the select-free V^T body of the waves that lie wholly inside their
sequence, can go wrong.

Same debug entry point (vrag_debug_qkv_attn_run), float64 reference and per-element bound as tests/test_qkv_attn_unit_gpu.py:
this module loads a private copy of that one and sets the smallest geometry the kernel accepts on the copy (head dim 64, two
heads: H = 128, two 64-k stages), so nothing of the bound is restated or loosened here.

Sequence lengths: 1, 15, 16, 17 (edges of a 16-row tile), 63, 64, 65 (wave boundary; the wave that holds the sequence's end against
the wave wholly inside it), 449, 511, 512 (last wave partly or fully live).
  * ADJACENT layout: the sequences lie back to back in the packed buffer, and the first seven share one 8-slot group at adjacent
    wave slots, so the rows behind a sequence's end inside its last wave are the LIVE rows of the next one.  Every row of every
    sequence and head against the float64 reference.
  * APART layout: every sequence in 64-row slots of its own; the rows behind its end hold zeros, or garbage that makes q, k and
    V there huge (bf16: 1e30; fp16: 3e4, past fp16's range after the projection): finite outputs, the same bits, no clamp report.
  * placement: one sequence alone (wave slot 0) and behind a 448-token one (wave slot 7) gives the same bits.
All eight instantiations (bf16 / fp16, global / banded, fold on / off)."""
import importlib.util
import os

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401


def _unit_module(h, nh):
    """A private copy of the fused kernel's unit-test module at another geometry (its own ledger; the original is untouched)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_qkv_attn_unit_gpu.py")
    spec = importlib.util.spec_from_file_location(f"_qkv_attn_unit_h{h}", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.H, mod.NH = h, nh
    return mod


U = _unit_module(128, 2)
gpu = pytest.mark.gpu
WINDOW = 64
SHARED = [1, 15, 16, 17, 63, 64, 65]     # 1 + 1 + 1 + 1 + 1 + 1 + 2 waves: one group, wave slots 0 .. 7
LENGTHS = SHARED + [449, 511, 512]       # eight waves each: a group of their own


def adjacent_layout():
    """Back to back (8-row aligned, as the hook asks): behind a sequence's end comes the next sequence."""
    seqs, cur = [], 0
    for n in LENGTHS:
        seqs.append((cur, n))
        cur += -(-n // 8) * 8
    need = max(r + 64 * -(-n // 64) for r, n in seqs)
    return seqs, -(-need // 256) * 256


def apart_layout():
    """Whole 64-row slots per sequence: the rows behind its end belong to nobody."""
    seqs, cur = [], 0
    for n in LENGTHS:
        seqs.append((cur, n))
        cur += 64 * -(-n // 64)
    return seqs, -(-cur // 256) * 256


def test_layouts():
    seqs, rows = adjacent_layout()
    groups = U.pack([r for r, _ in seqs], [n for _, n in seqs], 0)
    assert len(groups) == 4
    assert [int(w[1]) for w in groups[0]] == SHARED + [65]                 # adjacent slots, different lengths
    assert [int(w[2]) for w in groups[0]] == [0, 1, 2, 3, 4, 5, 6, 6]
    assert all(r2 - r == -(-n // 8) * 8 for (r, n), (r2, _) in zip(seqs, seqs[1:]))
    # whose last wave reads live rows of the next sequence (63 and 511 fill theirs up to the 8-row alignment, 64 fills it)
    assert [n for (r, n), (r2, _) in zip(seqs, seqs[1:]) if r2 < r + 64 * -(-n // 64)] == [1, 15, 16, 17, 65, 449]
    seqs2, rows2 = apart_layout()
    live = U.live_mask(rows2, seqs2)
    assert all(not live[r + n:r + 64 * -(-n // 64)].any() for r, n in seqs2)
    assert rows % 256 == 0 and rows2 % 256 == 0


@gpu
@pytest.mark.parametrize("inst", U.INSTANTIATIONS, ids=U.inst_id)
def test_adjacent_sequences_against_float64(inst):
    f16, local, fold = inst
    seqs, rows = adjacent_layout()
    rng = np.random.default_rng(4100 + 4 * f16 + 2 * local + fold)
    inp = U.make_inputs(rng, rows, f16, local, fold)
    o, groups, sat = U.run(inp, seqs, f16, local, WINDOW)
    assert sat == 0, "f16_saturated on in-range inputs"
    assert len(groups) == 4 and [int(w[2]) for w in groups[0]] == [0, 1, 2, 3, 4, 5, 6, 6]
    case = "epilogue adjacent " + U.inst_id(inst)
    U.check(case, inp, seqs, o, f16, local, fold, WINDOW)
    worst = max(r for (form, _, _), r in U._WORST.items() if form == case)
    print(f"\n{case}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (case, worst)
    assert U._CLASS[case].max() <= 1.0
    assert np.all(o[~U.live_mask(rows, seqs)] == U.CANARY), "the kernel wrote a row outside the sequences"


@gpu
@pytest.mark.parametrize("inst", U.INSTANTIATIONS, ids=U.inst_id)
def test_rows_behind_the_end_contribute_nothing(inst):
    f16, local, fold = inst
    seqs, rows = apart_layout()
    rng = np.random.default_rng(4200 + 4 * f16 + 2 * local + fold)
    inp = U.make_inputs(rng, rows, f16, local, fold)
    live = U.live_mask(rows, seqs)
    big = 3e4 if f16 else 1e30
    outs = []
    for fill in (0.0, big):
        cur = dict(inp)
        x = U.from16(inp["x"], f16)
        x[~live] = fill * np.sign(rng.standard_normal((int((~live).sum()), U.H)) + 0.5)
        cur["x"] = U.to16(x, f16)
        if fold:
            cur["ln_mu"], cur["ln_rstd"] = inp["ln_mu"].copy(), inp["ln_rstd"].copy()
            cur["ln_mu"][~live] = fill
            cur["ln_rstd"][~live] = fill
        outs.append(U.run(cur, seqs, f16, local, WINDOW))
    (o0, _, sat0), (o1, _, sat1) = outs
    assert sat0 == 0 and sat1 == 0
    assert np.all(np.isfinite(U.from16(o1[live], f16)))
    assert np.array_equal(o1, o0), "garbage behind a sequence's end changed its bits"
    assert np.all(o0[~live] == U.CANARY)


@gpu
@pytest.mark.parametrize("inst", U.INSTANTIATIONS, ids=U.inst_id)
def test_wave_slot_0_and_7_give_the_same_bits(inst):
    f16, local, fold = inst
    rng = np.random.default_rng(4300 + 4 * f16 + 2 * local + fold)
    inp = U.make_inputs(rng, 512, f16, local, fold)
    for n in (1, 17, 63, 64):
        both, groups, _ = U.run(inp, [(0, 448), (448, n)], f16, local, WINDOW)
        assert len(groups) == 1 and int(groups[0][7][2]) == 7 and int(groups[0][7][1]) == n
        alone, groups, _ = U.run(inp, [(448, n)], f16, local, WINDOW)
        assert int(groups[0][0][1]) == n and int(groups[0][0][2]) == 0
        assert np.array_equal(both[448:448 + n], alone[448:448 + n]), f"S = {n}: wave slot 7 and wave slot 0 differ"
        assert np.all(alone[:448] == U.CANARY) and np.all(alone[448 + n:] == U.CANARY)
