"""References of the v2 highlighter's device route.

`spec_offsets`: the offsets rule of `vrag_bpe_encode_offsets` in pure Python beside `bpe_cases.spec_ids` (its oracle is HF
`tokenizers`).  `select`: span selection over logit margins in vectorised numpy -- the reference of csrc/spans.hip; its own
oracle is `extractors.token_spans_to_char_spans` over the window maximum.  `random_job`: seeded jobs that hit the rule's edges."""
import numpy as np

from bpe_cases import spec_pieces


def spec_offsets(text, cfg):
    """[(start, end)] in code points of `text`, one per id of `spec_ids(text, cfg)`, or None when the device would flag it."""
    pieces = spec_pieces(text, cfg)
    if pieces is None:
        return None
    left, right, merged = cfg["merges"]
    rank = {(a, b): (r, m) for r, (a, b, m) in enumerate(zip(left, right, merged))}
    whole = {raw for raw, _i in cfg["whole"]}
    out, pos = [], 0
    for piece, run in pieces:
        raw = piece.encode("utf-8")
        if len(raw) > 64 and not run:
            return None
        if run or (cfg["ignore_merges"] and raw in whole):
            out.append((pos, pos + len(piece)))
            pos += len(piece)
            continue
        cp_of_byte = [k for k, ch in enumerate(piece) for _ in ch.encode("utf-8")]      # code point that holds every byte
        sym = [cfg["byte_ids"][b] for b in raw]
        width = [1] * len(sym)
        while len(sym) > 1:
            best = min(((rank[p][0], k) for k, p in enumerate(zip(sym, sym[1:])) if p in rank), default=None)
            if best is None:
                break
            k = best[1]
            sym[k:k + 2] = [rank[(sym[k], sym[k + 1])][1]]
            width[k:k + 2] = [width[k] + width[k + 1]]
        b0 = 0
        for w in width:
            out.append((pos + cp_of_byte[b0], pos + cp_of_byte[b0 + w - 1] + 1))
            b0 += w
        pos += len(piece)
    return out


def plan_windows(n_ctx, room, doc_stride):
    """Context-token slices [(a, b)] of the windows, by the loop of `GpuModelSpanExtractor._encode_windows`."""
    step = max(1, room - doc_stride)
    out, a = [], 0
    while True:
        b = min(n_ctx, a + room)
        out.append((a, b))
        if b >= n_ctx:
            return out
        a += step


def window_max(margins, windows, n_ctx):
    """M per context token: the maximum of the window margins that cover it, NaN where any of them is NaN, -inf where none does.
    `windows` = [(a, b, first)]: context tokens [a, b) at margins[first:first + b - a]."""
    M = np.full(n_ctx, -np.inf, np.float32)
    for a, b, first in windows:
        M[a:b] = np.maximum(M[a:b], margins[first:first + b - a])      # np.maximum propagates NaN, as the host route's does
    return M


def select(margins, windows, offsets, tau, min_span, gap):
    """Spans [(start, end)] of one job: hot = M > tau over tokens with end > start; runs of hot tokens that no cold token
    interrupts -> [first start, max end); runs joined while next.start - span.end <= gap; spans shorter than min_span dropped."""
    offsets = np.asarray(offsets, np.int64).reshape(-1, 2)
    M = window_max(np.asarray(margins, np.float32), windows, len(offsets))
    keep = offsets[:, 1] > offsets[:, 0]
    with np.errstate(invalid="ignore"):
        hot = (M > np.float32(tau))[keep]
    s, e = offsets[keep, 0], offsets[keep, 1]
    if not hot.any():
        return []
    edge = np.diff(np.concatenate([[0], hot.astype(np.int8), [0]]))
    first, last = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]      # runs [first, last)
    rs = s[first]
    re = np.maximum.reduceat(np.where(hot, e, np.iinfo(np.int64).min), first)      # cold tokens between two runs hold the minimum
    # merging: a new span starts beyond every earlier end (start > end + gap, gap >= 0, and every token has end > start), so
    # the running maximum of all run ends equals the current span's end
    assert gap >= 0, "select: the running maximum stands for the span's end only with gap >= 0"
    reach = np.maximum.accumulate(re)
    idx = np.nonzero(np.concatenate([[True], rs[1:] - reach[:-1] > gap]))[0]
    ms = rs[idx]
    me = np.maximum.reduceat(re, idx)
    ok = me - ms >= min_span
    return list(zip(ms[ok].tolist(), me[ok].tolist()))


def random_job(rng, n_ctx, room, doc_stride, tau, min_span, gap, hot_rate=0.5, nan_rate=0.0):
    """(margins float32 [T], windows [(a, b, first)], offsets int32 [n_ctx, 2]) of one seeded job.  Offsets walk through a text with
    zero-width tokens, tokens that share a character with the one before (start = previous end - 1), and gaps of -1, 0, gap and
    gap + 1 characters; token widths make single-token runs of min_span - 1 and min_span characters.  Every margin is at least
    1e-3 away from tau, so the probability form and the logit form of the comparison agree."""
    offsets = np.zeros((n_ctx, 2), np.int32)
    pos = 0
    for t in range(n_ctx):
        kind = rng.integers(0, 10)
        if kind == 0:
            offsets[t] = (pos, pos)                                        # zero width: skipped
            continue
        start = pos + int(rng.choice([-1, 0, 0, 0, 1, gap, gap + 1])) if t else 0
        start = max(start, 0)
        width = int(rng.choice([1, 2, 3, max(1, min_span - 1), max(1, min_span)]))
        offsets[t] = (start, start + width)
        pos = start + width
    wins = plan_windows(n_ctx, room, doc_stride)
    windows, first = [], 0
    for a, b in wins:
        first += int(rng.integers(0, 4))                                   # the question in front of the window
        windows.append((a, b, first))
        first += b - a + 1
    T = first
    hot = rng.random(T) < hot_rate
    # long stretches too: flip whole blocks so that runs span several tokens and steps
    for _ in range(max(1, T // 40)):
        a = int(rng.integers(0, T))
        hot[a:a + int(rng.integers(1, 30))] = rng.random() < hot_rate
    dist = (1e-3 + rng.random(T) * 4).astype(np.float32)
    margins = np.where(hot, np.float32(tau) + dist, np.float32(tau) - dist).astype(np.float32)
    if nan_rate:
        margins[rng.random(T) < nan_rate] = np.nan
    return margins, windows, offsets


def logits_of(margins, rng):
    """float32 [T, 2] whose fp32 difference logit[1] - logit[0] is exactly `margins` (logit[0] is a small integer)."""
    l0 = rng.integers(-3, 4, len(margins)).astype(np.float32)
    l1 = (margins + l0).astype(np.float32)
    fix = ~np.isnan(margins) & ((l1 - l0).astype(np.float32) != margins)
    l0 = np.where(fix, np.float32(0), l0)
    l1 = np.where(fix, margins, l1)
    return np.stack([l0, l1], axis=1).astype(np.float32)
