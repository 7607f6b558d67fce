"""The rule "an fp16 engine is never silently wrong", once, for every wrapper that drives an encoder handle.

fp16 MFMA operands saturate at +-65504 instead of overflowing: a checkpoint with activation outliers beyond that comes back
with plausible, wrong numbers.  The library reports every clamp per handle (`vrag_encoder_f16_saturated`);
`CheckedEngines.run` is the only place that asks.  On the first report a wrapper that BUILT its engines (it passes
`rebuild`) gets them replaced by bf16 ones (fp32's exponent range) and its batch run again; a wrapper that was HANDED
its engine cannot rebuild it and raises.  Providers, span extractor and reranker all run their device sequences through
it.  `greedy_batches`, the workspace-sized prefix batcher those wrappers share, lives here too.
"""
from __future__ import annotations

import logging
import threading
from typing import Any, Callable, Iterator, List, Optional, Sequence, Tuple

logger = logging.getLogger(__name__)


class CheckedEngines:
    """The engines of one checkpoint behind one wrapper (`engines[0]` is the wrapper's `.engine`).

    rebuild: `() -> a bf16 engine of the same checkpoint`, or None when the engines were handed in.
    on_swap: called after the engines were replaced, for the wrapper to re-derive what it cached from the old ones."""

    def __init__(self, engines: Sequence[Any], rebuild: Optional[Callable[[], Any]] = None,
                 on_swap: Optional[Callable[[], None]] = None):
        self.rebuild, self._on_swap = rebuild, on_swap
        self._swap_lock = threading.Lock()
        self._set(engines)

    def _set(self, engines: Sequence[Any]) -> None:
        # one list of (engine, lock), replaced as a whole: a reader never pairs an engine with another engine's lock.
        # The lock is the handle's own (wrappers may share a handle); fake engines without one get a private lock.
        self._slots = [(e, getattr(e, "lock", None) or threading.Lock()) for e in engines]

    @property
    def engines(self) -> List[Any]:
        return [e for e, _lock in self._live()]

    @property
    def locks(self) -> List[Any]:
        return [lock for _e, lock in self._live()]

    def _live(self):
        if not self._slots:
            raise RuntimeError("the fp16 engine was closed for a bf16 rebuild that failed: construct the wrapper again "
                               "with operand_dtype='bf16'")
        return self._slots

    def run(self, fn: Callable[[Any], Any], which: int = 0) -> Any:
        """`fn(engine)` -- one device sequence, load -> run -> head -> read -- under the current engine's lock; when the
        engine reports an fp16 clamp, once more on the bf16 engine that replaced it (bf16 engines are never asked)."""
        while True:     # a second pass follows the owner's one swap (`rebuild` is spent by it); nothing follows that pass
            engine, lock = self._live()[which]
            with lock:
                if self._live()[which][0] is not engine:
                    continue                             # replaced while this thread waited for the lock
                out = fn(engine)
                if getattr(engine, "operand_dtype", "bf16") != "f16" or not hasattr(engine, "f16_saturated") \
                        or not engine.f16_saturated(reset=True):
                    return out
                self._to_bf16(engine, which)

    def _to_bf16(self, engine: Any, which: int) -> None:
        """The caller holds `engine`'s lock.  The first thread to notice replaces every engine; the others find it done."""
        with self._swap_lock:
            slots = self._live()
            if slots[which][0] is not engine:
                return
            if self.rebuild is None:
                raise RuntimeError("fp16 MFMA operands saturated on this checkpoint (activations beyond 65504): "
                                   "build the engine with operand_dtype='bf16'")
            logger.warning("fp16 MFMA operands saturated (activations beyond 65504): switching to bf16 operands "
                           "(construct the wrapper with operand_dtype='bf16' to skip the probe)")
            rebuild, self.rebuild = self.rebuild, None       # one swap per owner: what it yields is final
            if len(slots) == 1:
                # nobody else can be on this handle (its lock is held, and stays held until the new engine is in place:
                # a caller that arrives meanwhile waits on it, then finds the slot replaced): freed first, so the fp16
                # and the bf16 copy of weights + workspace are never resident together
                engine.close()
                try:
                    new = [rebuild()]
                except BaseException:
                    self._slots = []                         # the only handle is gone: later calls say so (_live)
                    raise
            else:
                # a sub-batch still running on an old handle keeps it alive and finishes on it; the old handles close
                # when their last user lets go (EncoderEngine.__del__)
                new = [rebuild() for _ in slots]
            self._set(new)
            if self._on_swap is not None:
                self._on_swap()


def greedy_batches(lengths: Sequence[int], max_seqs: int, max_tokens: int,
                   max_ranges: Optional[int] = None) -> Iterator[Tuple[int, int]]:
    """[start, end) of consecutive device batches: each the longest prefix of what is left with at most `max_seqs`
    (and `max_ranges`) items and `max_tokens` tokens.  An item that does not fit on its own is reported as the empty
    batch (i, i) and passed over; what to do about it is the caller's."""
    cap = max_seqs if max_ranges is None else min(max_seqs, max_ranges)
    start = 0
    while start < len(lengths):
        tok, end = 0, start
        while end < len(lengths) and end - start < cap and tok + lengths[end] <= max_tokens:
            tok += lengths[end]
            end += 1
        yield start, end
        start = max(end, start + 1)
