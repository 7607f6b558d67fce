"""Span selection on the device (csrc/spans.hip) through the harness entry `vrag_debug_token_spans`: exactly the spans of
`spans_ref.select` (tests/test_highlighter_route_host.py holds that reference against `token_spans_to_char_spans`)."""
import ctypes as C
import math

import numpy as np
import pytest

from spans_ref import logits_of, plan_windows, random_job, select

pytestmark = pytest.mark.gpu
IP, LP, FP = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
TAU = np.float32(math.log(0.45 / 0.55))
MIN_SPAN, GAP = 5, 3


def run(logits, jobs, tau, min_span, gap, cap):
    """jobs = [(windows [(a, b, first)], offsets [n, 2])] with `first` relative to the job's own logits; returns (status, counts,
    spans) of one call over the concatenation."""
    from verbatim_rag_amd import _lib

    lib = _lib.load_debug()
    win = np.asarray([(j, a, b, base + first) for j, (base, (windows, _o)) in enumerate(jobs) for a, b, first in windows],
                     np.int32).reshape(-1, 4)
    wj, wa, wb, wf = (np.ascontiguousarray(win[:, i]) for i in range(4))
    job_off = np.zeros(len(jobs) + 1, np.int64)
    np.cumsum([len(o) for _base, (_w, o) in jobs], out=job_off[1:])
    offsets = np.ascontiguousarray(np.concatenate([np.asarray(o, np.int32).reshape(-1, 2) for _base, (_w, o) in jobs]))
    logits = np.ascontiguousarray(logits, np.float32)
    counts = np.full(len(jobs), -7, np.int32)
    spans = np.full((len(jobs), cap, 2), -7, np.int32)
    status = lib.vrag_debug_token_spans(
        logits.ctypes.data_as(FP), len(logits), wj.ctypes.data_as(IP), wa.ctypes.data_as(IP), wb.ctypes.data_as(IP), wf.ctypes.data_as(IP),
        len(wj), job_off.ctypes.data_as(LP), offsets.ctypes.data_as(IP), len(jobs), float(tau), min_span, gap, cap, counts.ctypes.data_as(IP),
        spans.ctypes.data_as(IP), 0)
    return status, counts, spans


def check(job_list, tau=TAU, min_span=MIN_SPAN, gap=GAP, seed=0):
    """job_list = [(margins, windows, offsets)]: one device call, every job equal to the reference."""
    rng = np.random.default_rng(seed)
    want = [select(m, w, o, tau, min_span, gap) for m, w, o in job_list]
    bases = np.concatenate([[0], np.cumsum([len(m) for m, _w, _o in job_list])])
    logits = np.concatenate([logits_of(m, rng) for m, _w, _o in job_list])
    cap = max(len(w) for w in want) + 1      # room for every job; the capacity protocol has its own test
    status, counts, spans = run(logits, [(int(b), (w, o)) for b, (_m, w, o) in zip(bases, job_list)], tau, min_span, gap, cap)
    assert status == 0
    assert counts.tolist() == [len(w) for w in want]
    for j, w in enumerate(want):
        assert [tuple(s) for s in spans[j, :len(w)].tolist()] == w, j
    return want


@pytest.mark.parametrize("n_jobs", [1, 70])
@pytest.mark.parametrize("n_ctx", [1, 63, 64, 65, 130, 1000])
def test_random_jobs_equal_the_reference(n_jobs, n_ctx):
    """One wave per job, 64 context tokens per step: lengths around the step, more jobs than one workgroup holds; room 40 with
    doc_stride 0 / 20 / 30 covers a token by 1, 2 and 4 windows, and the last window is short."""
    rng = np.random.default_rng(n_jobs * 1000 + n_ctx)
    jobs = [random_job(rng, n_ctx if j % 3 == 0 else int(rng.integers(1, n_ctx + 1)), 40, (0, 20, 30)[j % 3], TAU, MIN_SPAN, GAP,
                       hot_rate=(0.5, 0.15, 0.85)[(j // 3) % 3]) for j in range(n_jobs)]
    want = check(jobs)
    if n_jobs == 70 and n_ctx >= 130:
        assert sum(len(w) for w in want) > n_jobs      # the comparison is not one of empty lists


@pytest.mark.parametrize("doc_stride,cover", [(0, 1), (20, 2), (30, 4)])
def test_window_coverage_and_the_maximum(doc_stride, cover):
    """Only ONE of the windows that cover a token is hot: the maximum decides, whichever window it is."""
    n_ctx, room = 255, 40
    wins = plan_windows(n_ctx, room, doc_stride)
    depth = np.zeros(n_ctx, int)
    for a, b in wins:
        depth[a:b] += 1
    assert depth.max() == cover and (wins[-1][1] - wins[-1][0]) < room      # the last window is short
    rng = np.random.default_rng(cover)
    offsets = np.stack([np.arange(n_ctx) * 2, np.arange(n_ctx) * 2 + 2], axis=1).astype(np.int32)
    windows, first = [], 0
    for a, b in wins:
        windows.append((a, b, first + 3))
        first += 3 + b - a + 1
    for pick in range(cover):
        margins = np.full(first, TAU - 2, np.float32)
        hot_tokens = rng.random(n_ctx) < 0.5
        for t in np.nonzero(hot_tokens)[0]:
            covering = [(a, b, f) for a, b, f in windows if a <= t < b]
            a, b, f = covering[min(pick, len(covering) - 1)]
            margins[f + t - a] = TAU + 1
        want = check([(margins, windows, offsets)], seed=pick)
        assert len(want) == 1 and len(want[0]) > 3


def test_all_hot_all_cold_and_a_run_that_reaches_the_last_token():
    n_ctx = 200
    offsets = np.stack([np.arange(n_ctx) * 3, np.arange(n_ctx) * 3 + 2], axis=1).astype(np.int32)      # 1 character between tokens
    windows = [(a, b, 10 + a) for a, b in [(0, n_ctx)]]
    hot = np.full(n_ctx + 10, TAU + 1, np.float32)
    cold = np.full(n_ctx + 10, TAU - 1, np.float32)
    tail = cold.copy()
    tail[10 + 150:] = TAU + 1
    want = check([(hot, windows, offsets), (cold, windows, offsets), (tail, windows, offsets)])
    assert want == [[(0, 3 * n_ctx - 1)], [], [(450, 3 * n_ctx - 1)]]
    # no windows at all: nothing covers a token, every token is cold
    assert check([(cold[:0], [], offsets)]) == [[]]


def test_nan_logit_inside_an_overlap_makes_the_token_cold():
    n_ctx, room = 100, 40
    wins = plan_windows(n_ctx, room, 20)
    windows, first = [], 0
    for a, b in wins:
        windows.append((a, b, first))
        first += b - a
    offsets = np.stack([np.arange(n_ctx) * 2, np.arange(n_ctx) * 2 + 2], axis=1).astype(np.int32)
    margins = np.full(first, TAU + 1, np.float32)
    t = 30      # covered by windows 0 (0..40) and 1 (20..60)
    a1, _b1, f1 = windows[1]
    margins[f1 + t - a1] = np.nan      # the other window says hot
    gap0 = check([(margins, windows, offsets)], gap=0)
    assert gap0 == [[(0, 60), (62, 200)]]      # merge_gap_chars = 0: the cold token's two characters keep the runs apart
    assert check([(margins, windows, offsets)], gap=2) == [[(0, 200)]]
    # NaN in the logits themselves, and infinities of equal sign (inf - inf)
    logits = logits_of(margins, np.random.default_rng(1))
    logits[f1 + 50 - a1] = (np.inf, np.inf)
    status, counts, spans = run(logits, [(0, (windows, offsets))], TAU, MIN_SPAN, 0, 8)
    assert status == 0 and counts.tolist() == [3] and spans[0, :3].tolist() == [[0, 60], [62, 100], [102, 200]]
    # logit[1] = +inf beside a finite logit[0] is a NaN row of the host's softmax: cold; (-inf, finite) is P = 1 there: hot
    logits[f1 + 50 - a1] = (-np.inf, 0.0)
    logits[f1 + 55 - a1] = (0.0, np.inf)
    status, counts, spans = run(logits, [(0, (windows, offsets))], TAU, MIN_SPAN, 0, 8)
    assert status == 0 and counts.tolist() == [3] and spans[0, :3].tolist() == [[0, 60], [62, 110], [112, 200]]


def test_capacity_is_reported_with_true_counts_and_the_retry_succeeds():
    n_ctx = 60
    offsets = np.stack([np.arange(n_ctx) * 10, np.arange(n_ctx) * 10 + 8], axis=1).astype(np.int32)
    margins = np.full(n_ctx, TAU - 1, np.float32)
    margins[[5, 20, 40]] = TAU + 1      # three spans of 8 characters, far apart
    windows = [(0, n_ctx, 0)]
    one = np.full(n_ctx, TAU - 1, np.float32)
    one[7] = TAU + 1
    jobs = [(0, (windows, offsets)), (n_ctx, (windows, offsets))]
    logits = np.concatenate([logits_of(margins, np.random.default_rng(0)), logits_of(one, np.random.default_rng(1))])
    status, counts, _spans = run(logits, jobs, TAU, MIN_SPAN, GAP, 1)
    assert status == -3 and counts.tolist() == [3, 1]      # VRAG_ERR_CAPACITY, counts exact
    status, counts, spans = run(logits, jobs, TAU, MIN_SPAN, GAP, int(counts.max()))
    assert status == 0 and counts.tolist() == [3, 1]
    assert spans[0].tolist() == [[50, 58], [200, 208], [400, 408]] and spans[1, 0].tolist() == [70, 78]


def test_tables_are_checked_before_the_launch():
    """A window that reads past the logits, past its job's context, or out of order is refused (VRAG_ERR_INVALID = -1)."""
    offsets = np.stack([np.arange(10), np.arange(10) + 1], axis=1).astype(np.int32)
    logits = np.zeros((10, 2), np.float32)
    assert run(logits, [(0, ([(0, 10, 0)], offsets))], TAU, 1, 0, 4)[0] == 0
    assert run(logits, [(0, ([(0, 10, 1)], offsets))], TAU, 1, 0, 4)[0] == -1      # rows 1 .. 11 of 10
    assert run(logits, [(0, ([(0, 11, 0)], offsets))], TAU, 1, 0, 4)[0] == -1      # 11 context tokens of 10
    assert run(logits, [(0, ([(5, 10, 0), (0, 5, 5)], offsets))], TAU, 1, 0, 4)[0] == -1
    assert run(logits, [(0, ([(0, 10, 0)], offsets))], TAU, 1, 0, 0)[0] == -1      # no capacity
