"""CPU: `checked_engine` on fake engines -- when the fp16 clamp report is asked, what a clamp does with and without a
`rebuild`, which lock is taken afterwards, the swap under concurrent callers, and the shared greedy batcher against the
rule the providers used to carry."""
import logging
import threading
import types

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd.checked_engine import CheckedEngines, greedy_batches
from verbatim_rag_amd.rerankers import GpuCrossEncoderReranker

from test_reranker_host import _tok

SATURATED = ("fp16 MFMA operands saturated on this checkpoint (activations beyond 65504): "
             "build the engine with operand_dtype='bf16'")


class RecordingLock:
    def __init__(self):
        self.acquired, self._lock = 0, threading.RLock()

    def __enter__(self):
        self._lock.acquire()
        self.acquired += 1

    def __exit__(self, *exc):
        self._lock.release()


class FakeEngine:
    """Clamps on every run while its operands are fp16, the way an outlier checkpoint does."""

    def __init__(self, operand_dtype, clamps=True, events=None, name=""):
        self.operand_dtype, self.clamps, self.name = operand_dtype, clamps, name
        self.lock = RecordingLock()
        self.asked = self.closed = 0
        self.events = events if events is not None else []

    def f16_saturated(self, reset=True):
        self.asked += 1
        return self.clamps and self.operand_dtype == "f16"

    def close(self):
        self.closed += 1
        self.events.append(("close", self.name))


def _fn(calls):
    def fn(engine):
        calls.append(engine)
        return engine.operand_dtype
    return fn


def test_bf16_engines_and_engines_without_the_report_are_never_asked():
    bf = FakeEngine("bf16")
    calls = []
    assert CheckedEngines([bf]).run(_fn(calls)) == "bf16"
    assert calls == [bf] and bf.asked == 0 and bf.lock.acquired == 1
    bare = types.SimpleNamespace(operand_dtype="f16")          # no f16_saturated, no lock: a private lock serves
    calls = []
    assert CheckedEngines([bare]).run(_fn(calls)) == "f16" and calls == [bare]


def test_fp16_without_a_clamp_runs_once():
    eng = FakeEngine("f16", clamps=False)
    calls = []
    owner = CheckedEngines([eng], rebuild=lambda: pytest.fail("no clamp, no rebuild"))
    assert owner.run(_fn(calls)) == "f16"
    assert calls == [eng] and eng.asked == 1 and eng.closed == 0 and owner.engines == [eng]


def test_clamp_with_rebuild_runs_again_on_the_bf16_engine_and_takes_its_lock(caplog):
    events = []
    old, new = FakeEngine("f16", events=events, name="old"), FakeEngine("bf16", events=events, name="new")
    swapped = []

    def rebuild():
        events.append(("rebuild", "new"))
        return new

    owner = CheckedEngines([old], rebuild, on_swap=lambda: swapped.append(owner.engines[0]))
    calls = []
    with caplog.at_level(logging.WARNING):
        assert owner.run(_fn(calls)) == "bf16"
    assert calls == [old, new] and owner.engines == [new] and swapped == [new]
    warnings = [r.getMessage() for r in caplog.records if "saturated" in r.getMessage()]
    assert len(warnings) == 1 and "operand_dtype='bf16'" in warnings[0]
    assert events == [("close", "old"), ("rebuild", "new")]      # never both resident
    assert owner.locks == [new.lock] and new.lock.acquired == 1 and old.lock.acquired == 1
    owner.run(_fn(calls))
    assert new.lock.acquired == 2 and old.lock.acquired == 1 and new.asked == 0 and calls[-1] is new


def test_clamp_on_a_handed_engine_raises_and_leaves_it_open():
    eng = FakeEngine("f16")
    owner = CheckedEngines([eng])
    with pytest.raises(RuntimeError) as exc:
        owner.run(lambda engine: 1)
    assert str(exc.value) == SATURATED
    assert eng.closed == 0 and owner.engines == [eng]


def test_two_engines_clamping_from_two_threads_are_rebuilt_once():
    olds = [FakeEngine("f16", name="a"), FakeEngine("f16", name="b")]
    built = []
    both_ran = threading.Barrier(2, timeout=30)

    def rebuild():
        built.append(FakeEngine("bf16"))
        return built[-1]

    owner = CheckedEngines(olds, rebuild)

    def fn(engine):
        if engine.operand_dtype == "f16":
            both_ran.wait()                                  # both sub-batches are on the old engines when the clamps are read
        return engine.operand_dtype

    got = [None, None]

    def work(which):
        got[which] = owner.run(fn, which)

    threads = [threading.Thread(target=work, args=(w,)) for w in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert got == ["bf16", "bf16"] and len(built) == 2 and owner.engines == built
    assert [e.closed for e in olds] == [0, 0]                # released by their last user, not by the owner


def test_failing_rebuild_propagates_and_later_calls_fail_cleanly():
    eng = FakeEngine("f16")

    def rebuild():
        raise MemoryError("no room for the bf16 engine")

    owner = CheckedEngines([eng], rebuild)
    calls = []
    with pytest.raises(MemoryError):
        owner.run(_fn(calls))
    assert eng.closed == 1 and calls == [eng]
    with pytest.raises(RuntimeError, match="rebuild that failed"):
        owner.run(_fn(calls))
    with pytest.raises(RuntimeError, match="rebuild that failed"):
        owner.engines
    assert calls == [eng]                                    # the closed handle is not touched again


def _parent_batches(lengths, max_seqs, max_tokens, max_ranges):
    """The rule `_EncoderProvider._batches` carried before the batcher was shared.  Where it raised on an item larger than
    the workspace, this records (i, i) and goes on behind the item, as the highlighter's copy of the loop did."""
    out, start = [], 0
    while start < len(lengths):
        tok, end = 0, start
        while end < len(lengths) and end - start < max_seqs and end - start < max_ranges \
                and tok + lengths[end] <= max_tokens:
            tok += lengths[end]
            end += 1
        if end == start:
            out.append((start, start))
            start += 1
            continue
        out.append((start, end))
        start = end
    return out


def test_greedy_batches_cut_where_the_three_loops_cut():
    rng = np.random.default_rng(20240607)
    bound = {"seqs": 0, "tokens": 0, "ranges": 0, "oversize": 0}
    for case in range(400):
        n = int(rng.integers(1, 60))
        max_tokens = int(rng.integers(20, 200))
        lengths = [int(x) for x in rng.integers(1, max(2, max_tokens // int(rng.integers(1, 8))), n)]
        max_seqs, max_ranges = 1000, 1000
        if case % 4 == 0:
            max_seqs = int(rng.integers(1, 6))
        elif case % 4 == 1:
            max_ranges = int(rng.integers(1, 6))
        elif case % 4 == 3:
            where = (0, n // 2, n - 1)[case // 4 % 3]         # one oversize item: start, middle, end
            lengths[where] = max_tokens + 1 + int(rng.integers(0, 5))
        want = _parent_batches(lengths, max_seqs, max_tokens, max_ranges)
        assert list(greedy_batches(lengths, max_seqs, max_tokens, max_ranges)) == want, (lengths, max_seqs, max_tokens, max_ranges)
        for a, b in want:                                    # which limit ended each batch: every kind must occur
            if a == b:
                bound["oversize"] += 1
            elif b < n and b - a == max_seqs:
                bound["seqs"] += 1
            elif b < n and b - a == max_ranges:
                bound["ranges"] += 1
            elif b < n:
                bound["tokens"] += 1
    assert all(v >= 20 for v in bound.values()), bound
    # without max_ranges (reranker, highlighter) the cap is max_seqs alone
    assert list(greedy_batches([5, 5, 5, 5, 5], 2, 100)) == [(0, 2), (2, 4), (4, 5)]
    assert list(greedy_batches([5, 5, 5], 10, 10)) == [(0, 2), (2, 3)]
    assert list(greedy_batches([], 4, 10)) == []


class FakePairEngine:
    max_seq_len, max_seqs, max_tokens, pair_labels = 64, 4, 100, 1
    shape = types.SimpleNamespace(cls_token_id=1, sep_token_id=2)

    def __init__(self, operand_dtype, value):
        self.operand_dtype, self.value = operand_dtype, value
        self.lock = threading.RLock()
        self.runs = self.closed = 0

    def pair_logits(self, seqs, type_ids):
        self.runs += 1
        return np.full((len(seqs), 1), self.value, np.float32)

    def f16_saturated(self, reset=True):
        return self.operand_dtype == "f16" and self.runs == 1     # the first pair_logits clamps

    def close(self):
        self.closed += 1


def test_reranker_raises_on_a_handed_engine_and_rescores_on_a_rebuilt_one():
    texts = ["w1 w2", "w5 w5 w5", "w5"]
    handed = GpuCrossEncoderReranker(FakePairEngine("f16", 7.0), _tok())
    with pytest.raises(RuntimeError, match="saturated"):
        handed.score("w5 what", texts)
    with pytest.raises(RuntimeError, match="saturated"):
        GpuCrossEncoderReranker(FakePairEngine("f16", 7.0), _tok()).score_batch(["w5 what"], [texts])
    assert handed.engine.closed == 0

    for call in ("score", "score_batch"):
        old, new = FakePairEngine("f16", 7.0), FakePairEngine("bf16", 3.0)
        new.max_seq_len = 32
        rr = GpuCrossEncoderReranker(old, _tok())
        rr._checked.rebuild = lambda: new
        got = rr.score("w5 what", texts) if call == "score" else rr.score_batch(["w5 what"], [texts])[0]
        assert got == [3.0, 3.0, 3.0]                        # the rebuilt engine's scores, none of the clamped ones
        assert rr.engine is new and old.closed == 1 and rr.max_length == 32
