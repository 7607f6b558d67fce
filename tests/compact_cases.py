"""Shared by the compaction tests of the store (tests/test_compact_host.py over the CPU stand-ins, tests/test_compact_store_gpu.py
on the device): the sequence runner of tests/store_model.py extended -- by subclassing, store_model.py is untouched -- so that a
sequence also draws `compact()` steps, with `Model.compact()` beside each one, and the stand-ins extended by the compaction
calls of the device layers.

Around every `compact()` the same queries are asked before and after it: ids, score bits, texts, enhanced texts and metadata
must be identical (a compaction changes row numbers, never an answer).  The runner counts what the sequences reached:
`compact_dead` (a compaction that found dead rows), `compact_clean` (one that found none: it returns 0), `compact_then_add`
(an insert behind a compaction: the reclaimed room takes appends; the runner schedules one such pair per sequence when the draws
have not produced it by the first delete of the last two thirds) and `ivf_compact` (a compaction of a store
with a trained IVF overlay, whose `trained_rows` it must leave alone)."""
import numpy as np

import store_model as M

OPS = ("add", "delete", "query", "batch", "save_load", "filter_only", "compact")
OP_P = np.asarray([0.27, 0.12, 0.12, 0.36, 0.03, 0.03, 0.07])


class CompactDense(M.ModelDense):
    """`ModelDense` with `DenseShard.compact` / `.read`."""

    def compact(self, keep):
        keep = np.asarray(keep, dtype=bool)
        assert len(keep) == len(self.rows)
        self.rows = self.rows[keep]
        return len(self.rows)

    def read(self, first_row=0, n=None):
        return self.rows[first_row:None if n is None else first_row + n].copy()


class LastRowIntoFirstHole(CompactDense):
    """The defect of the negative control: the first hole is filled with the last live row -- the right rows, not their order."""

    def compact(self, keep):
        keep = np.asarray(keep, dtype=bool)
        kept = self.rows[keep]
        holes = np.nonzero(~keep)[0]
        if len(holes) and len(kept) > 1:
            at = int(keep[:holes[0]].sum())                   # where the first hole's successor lands
            if at < len(kept) - 1:
                kept = np.concatenate([kept[:at], kept[-1:], kept[at:-1]])
        self.rows = kept
        return len(kept)


def answers(results):
    """Everything a caller sees of a result list."""
    return [(r.id, float(r.score).hex(), r.text, r.enhanced_text, sorted(r.metadata.items())) for r in results]


class CompactRunner(M.Runner):
    def _around(self):
        """The questions asked on both sides of a compaction: three queries, each unfiltered and under a wide filter, in the
        configuration's first mode."""
        mode, weights, _w = self.modes[0]
        qs = self._queries(3)
        return [(q, self._store_kwargs(mode, weights, 10, flt, 60)) for q in qs for flt in (0, 4)]

    def _ask(self, asked):
        return [answers(self._single(q, kw)) for q, kw in asked]

    def _compact(self) -> None:
        st = self.store
        dead = sum(not r.alive for r in self.model.rows)
        live = len(self.model.rows) - dead
        asked = self._around()
        before = self._ask(asked)                              # flushes: the device holds every row
        trained = st.ivf_stats() if self.cfg.ivf else None
        reclaimed = self._call(st.compact)
        self.model.compact()
        self._changed()
        if reclaimed != dead or len(st) != live:
            self._fail("compact() count", [reclaimed, len(st)], [dead, live])
        after = self._ask(asked)
        for i, (b, a) in enumerate(zip(before, after)):
            if a != b:
                self._fail(f"query {i} around compact()", a, b)
        if trained is not None:
            now = st.ivf_stats()
            if now is None or now["trained_rows"] != trained["trained_rows"] or now["rows"] != live:
                self._fail("ivf_stats around compact()", [now], [dict(trained, rows=live)])
            if dead:
                self.cover.hit("ivf_compact")
        self.cover.hit("compact_dead" if dead else "compact_clean")
        self._after_compact = bool(dead)

    def _add(self, n, reuse, bulk):
        super()._add(n, reuse, bulk)
        if getattr(self, "_after_compact", False):
            self.cover.hit("compact_then_add")
        self._after_compact = False

    def _save_load(self):
        super()._save_load()
        self._after_compact = False                            # a load starts from fresh structures

    def _run(self, watch) -> None:
        rng = self.rng
        self._mode_p = np.asarray([w for _m, _x, w in self.modes], float) / sum(w for _m, _x, w in self.modes)
        self._filter_p = np.asarray([w for _e, _p, w in M.FILTERS], float) / sum(w for _e, _p, w in M.FILTERS)
        self.store = self._new_store()
        self.log.append(f"add {self.start}")
        self._add(self.start, reuse=False, bulk=True)
        due = []                                               # operations that follow without a draw
        while len(self.log) < self.n_ops:
            op = due.pop(0) if due else OPS[int(rng.choice(len(OPS), p=OP_P))]
            if op == "add":
                n = int(rng.choice(M.ADD_SIZES, p=self.cfg.size_p))
                reuse, bulk = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
                reuse = reuse and len(self.log) >= self.cfg.reuse_from
                self.log.append(f"add {n}{' reuse' if reuse else ''}{' bulk' if bulk else ''}")
                self._add(n, reuse, bulk)
            elif op == "delete":
                n = int(rng.choice((1, 5, 60), p=(0.4, 0.4, 0.2)))
                self.log.append(f"delete {n}")
                self._delete(n)
                # whatever the seed draws, every sequence compacts dead rows and inserts behind the compaction: the first delete
                # of its last two thirds that no such compaction has preceded is followed by one, and that by an insert
                if len(self.log) >= self.n_ops // 3 and not self.cover.seen.get("compact_then_add"):
                    due = ["compact", "add"]
            elif op == "save_load":
                self.log.append("save_load")
                self._save_load()
            elif op == "compact":
                self.log.append("compact")
                self._compact()
                self._observe()
            elif op == "filter_only":
                self._filter_only()
                self._observe()
            else:
                self._query_op(batch=op == "batch")
                self._observe()
            if watch.failed:
                raise M.StoreFault(f"{self._where()}: {watch.failed[0]}")
