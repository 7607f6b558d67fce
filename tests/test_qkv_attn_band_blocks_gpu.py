"""The banded fused Wqkv + RoPE + attention kernel's static tile bodies (csrc/qkv_attn.hip section 3: FIRST / MID / LAST score only
the 16 x 16 blocks that hold an in-band element when |i - j| <= 64) against its generic body, through the same hook as
tests/test_qkv_attn_unit_gpu.py (vrag_debug_qkv_attn_run) and with that module's operands, float64 reference, bound and ledger.

debug_flags = 32 (include/vrag_amd_debug.h) makes every wave take the generic body.  Per banded instantiation (bf16 / fp16, fold on
and off) and per layout:
  1. window 64 (the model's local_attention = 128): the output with the flag equals the output without it bit for bit
     (np.array_equal over the whole buffer, canary rows included).  A skipped block contributed p = exp2(-inf) = 0 and
     acc + 0 * v = acc, the kept operations are the same on the same operands in the same order;
  2. the same at window 32 and 128 (local_attention 64 and 256), where no static body applies and both runs are the generic one;
  3. every output within the unit test's bound of its float64 reference (check() of that module: no new tolerance);
  4. at window 64 a reference whose band is one key narrower or wider (the `band-1` / `band+1` defects of reference()) fails the
     bound on every layout that has a static body, and by 10 x (the unit test's demand of a control) on the worst of them: the
     keys at distance 64 and 65 sit in the diagonal blocks kb == c (65 at l15 = 0: in the dead block beside it), so these inputs
     do exercise the diagonal masks and the block selection.

Layouts: the smallest that reach every body and every hand-over between the wave paths.  A wave takes FIRST MID LAST when the
tiles in front of and behind its own lie inside the sequence, MID LAST as the sequence's first wave, FIRST MID as its last when
that is a full one, and the generic loop otherwise:
  512          six interior waves, wave 0 MID LAST, wave 7 FIRST MID
  192          one interior wave with both neighbours
  193, 129     the last tile crosses S: the wave in front of it and the wave that holds the end are generic, the others static
  128          MID LAST beside FIRST MID, no interior wave
  65, 64       generic only
  192 + 320    one workgroup, kbase != 0: two sequences' bands side by side in the K / V^T slots
  449, then 63 directly behind it in the buffer: garbage query rows behind a sequence's end inside its last wave."""
import numpy as np
import pytest

from test_qkv_attn_unit_gpu import CANARY, NH, check, control, inst_id, live_mask, make_inputs, place, reference, run

gpu = pytest.mark.gpu

FORCE_GENERIC = 32
BANDED = [(f16, 1, fold) for f16 in (False, True) for fold in (False, True)]
# (name, lengths or explicit (row, length) list, groups the first-fit packer must make)
LAYOUTS = [("512", [512], 1), ("192", [192], 1), ("193", [193], 1), ("129", [129], 1), ("128", [128], 1), ("65", [65], 1),
           ("64", [64], 1), ("192+320", [192, 320], 1), ("449|63", [(0, 449), (456, 63)], 2)]


def layout(spec, rng):
    if isinstance(spec[0], tuple):
        need = max(r + 64 * -(-n // 64) for r, n in spec)
        return list(spec), -(-need // 256) * 256
    return place(spec, rng)


def both_bodies(inp, seqs, rows, f16, fold, window, n_groups):
    """The launch without and with the flag: equal bits, no clamp, nothing written outside the sequences.  Returns o."""
    o, groups, sat = run(inp, seqs, f16, 1, window)
    og, _, satg = run(inp, seqs, f16, 1, window, debug_flags=FORCE_GENERIC)
    assert len(groups) == n_groups, groups
    assert sat == 0 and satg == 0
    assert np.array_equal(o, og), f"static and generic tile bodies give different bits (window {window}, {seqs})"
    assert np.all(o[~live_mask(rows, seqs)] == CANARY)
    return o


def worst_defect(inp, seqs, refs, f16, fold, window, defect):
    """(ratio, wrong, ref, bound) of the (sequence, head) on which the defective reference misses the bound by the most."""
    best = (0.0, None, None, None)
    for si, seq in enumerate(seqs):
        for head in range(NH):
            ref, bound = refs[(si, head)]
            wrong, _ = reference(inp, seq, head, f16, 1, fold, window, defect=defect)
            r = float((np.abs(wrong - ref) / bound).max())
            if r > best[0]:
                best = (r, wrong, ref, bound)
    return best


@gpu
@pytest.mark.parametrize("window", [64, 32, 128])
@pytest.mark.parametrize("inst", BANDED, ids=inst_id)
def test_static_bodies_equal_generic(inst, window):
    f16, _, fold = inst
    worst = {}
    for li, (name, spec, n_groups) in enumerate(LAYOUTS):
        rng = np.random.default_rng(4000 + 100 * li + 4 * f16 + 2 * fold)   # the same operands at every window
        seqs, rows = layout(spec, rng)
        inp = make_inputs(rng, rows, f16, 1, fold)
        o = both_bodies(inp, seqs, rows, f16, fold, window, n_groups)
        refs = check(f"band blocks {name} W={window} " + inst_id(inst), inp, seqs, o, f16, 1, fold, window)
        if window == 64 and max(n for _, n in seqs) >= 128:   # a sequence with a static body
            for defect in ("band-1", "band+1"):
                got = worst_defect(inp, seqs, refs, f16, fold, window, defect)
                assert got[0] > 1.0, f"{name}: the bound hides {defect} (worst ratio {got[0]:.3g})"
                if got[0] > worst.get(defect, (0.0,))[0]:
                    worst[defect] = got
    for defect, (_, wrong, ref, bound) in worst.items():
        control(f"band blocks {defect} [{inst_id(inst)}]", wrong, ref, bound)


def test_hook_refuses_other_debug_flags():
    """Only 0 and 32 leave the result what it is: the hook refuses the phase probes before anything is launched."""
    from test_qkv_attn_unit_gpu import raw_run
    rng = np.random.default_rng(6)
    inp = make_inputs(rng, 256, False, 1, False)
    for flags in (1, 2, 33, -1):
        status, o, _, _ = raw_run(inp, [(0, 100)], False, 1, 64, debug_flags=flags)
        assert status == -1, (flags, status)
        assert np.all(o == CANARY)
