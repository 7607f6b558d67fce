"""Shared by the list-filter tests (host and GPU): a seeded corpus of metadata with list values, the `json_contains` expressions
every route is compared on, and a numpy restatement of a `FilterProgram` with the "list_any" op over the arrays of
`store_columns.MetaColumn` (kinds, payloads, element offsets, string tables).  Test code: the package never imports it."""
import operator
import random

import numpy as np

from verbatim_rag_amd.store_columns import KIND_BOOL, KIND_NUMBER, KIND_STRING, MetaColumn
from verbatim_rag_amd.store_filter import STRING_COMPARE, parse_filter

KEYS = ("authors", "tags", "years", "flags", "year", "source", "score", "JSON_CONTAINS")   # the last: a key no row holds
AUTHORS = ("Adam Kovacs", "Paul Schmitt", "Gabor Recski", "Zoë Ölmez", "日本 太郎", "", "5", "true", "a%b", "Ada")
SOURCES = ("web", "journal", "arXiv", "Zürich", "book")
_MIXED = (5, 5.0, "5", True, False, 1, 0, -0.0, 2020, 2020.0, "2020", None, [5], {"v": 5}, "medical-nlp", "x", 1.5, float("inf"))
_NOT_A_LIST = (None, "Adam Kovacs", 5, True, {"0": "Adam Kovacs"}, 2020.0)


def _list_length(rng: random.Random) -> int:
    pick = rng.random()
    if pick < 0.12:
        return 0
    if pick < 0.80:
        return rng.randint(1, 5)
    if pick < 0.97:
        return rng.randint(6, 30)
    return rng.choice((31, 63, 64, 65, 70))                # around a wave's width, and the longest


def _list_value(rng: random.Random, pool):
    """A list of 0 - 70 elements of `pool` (duplicates happen), a tuple now and then; in three rows of ten no list at all."""
    pick = rng.random()
    if pick < 0.10:
        return None                                        # the key is left out
    if pick < 0.30:
        return rng.choice(_NOT_A_LIST)
    value = [rng.choice(pool) for _ in range(_list_length(rng))]
    return tuple(value) if rng.random() < 0.05 else value


def list_rows(n: int, seed: int):
    """`n` metadata dicts: four list-valued keys (strings, mixed kinds, numbers, booleans with strangers) and three scalar ones.
    No NaN and no int beyond float range, so every column is exact."""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        md = {"year": rng.choice((1999, 2020, 2020.0, 2024, 2026, "2024")), "source": rng.choice(SOURCES), "score": rng.randint(0, 100) / 100}
        for key, pool in (("authors", AUTHORS), ("tags", _MIXED), ("years", (1999, 2020, 2020.0, 2024, -0.0, 0, 2 ** 53)),
                          ("flags", (True, False, True, 1, 0, "true", None))):
            value = _list_value(rng, pool)
            if value is not None:
                md[key] = value
        if rng.random() < 0.1:
            del md["source"]
        rows.append(md)
    return rows


# every expression passes at least one row of list_rows(2000, seed=7) and rejects at least one (the host test asserts it)
EXPRESSIONS = (
    'json_contains(metadata["authors"], "Adam Kovacs")',
    "json_contains(authors, 'Zoë Ölmez')",
    'JSON_CONTAINS(authors, "")',
    'not json_contains(metadata["authors"], "Paul Schmitt")',
    'json_contains_any(authors, ["Gabor Recski", "nobody", "日本 太郎"])',
    'json_contains_all(authors, ["Adam Kovacs", "Paul Schmitt"])',
    'JSON_CONTAINS_ALL(metadata["authors"], ["Ada", "5", "true"])',
    "json_contains(tags, 5)",
    'json_contains(tags, "5")',
    "json_contains(tags, true)",
    "json_contains(tags, 1)",
    "json_contains(tags, 0) and not json_contains(tags, false)",
    "json_contains(tags, 2.02e3) or json_contains(tags, 1e999)",
    'json_contains_any(tags, [5, "5", true])',
    'json_contains_all(tags, [5, "5", true])',
    "json_contains(years, -0.0)",
    "json_contains(years, 9007199254740993)",
    "json_contains(flags, false) && not json_contains(flags, 0)",
    'json_contains(flags, "true")',
    'metadata["year"] >= 2024 && json_contains(metadata["tags"], "medical-nlp")',
    'json_contains(authors, "Ada") and source LIKE "%r%" and score < 0.5',
    'source in ["web", "book"] or json_contains_any(years, [1999, 2024])',
    'not (json_contains(authors, "Ada") or json_contains(tags, "x")) and year != 2020',
    '(json_contains(authors, "a%b") or source LIKE "Z_rich") and not json_contains_all(years, [2020, 0])',
    'authors == "Adam Kovacs" or json_contains(authors, "Adam Kovacs")',
    'json_contains(authors, "Adam Kovacs") and json_contains(tags, 5) and json_contains(years, 2020) and json_contains(flags, true)',
    'not not json_contains_any(JSON_CONTAINS, [1]) or json_contains(tags, "2020") and score >= 0.25',
)


def expected(expr: str, rows) -> np.ndarray:
    pred = parse_filter(expr)
    return np.asarray([bool(pred(md)) for md in rows], dtype=bool)


def columns_of(rows, keys):
    out = []
    for k in keys:
        c = MetaColumn(k)
        c.extend(rows)
        out.append(c)
    return out


_NUM = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}


def leaf_answers(lf, strings, kinds: np.ndarray, payload: np.ndarray, table=None) -> np.ndarray:
    """What leaf `lf` answers for each (kind, payload): the four cases include/vrag_amd.h states.  `table`: bool per dictionary
    code (default: the leaf's comparison applied to `strings`); a code at or beyond it answers 0."""
    out = np.full(len(kinds), bool(lf.other), dtype=bool)
    is_bool = kinds == KIND_BOOL
    out[is_bool] = np.asarray(lf.bools, dtype=bool)[payload[is_bool].astype(np.int64)]
    is_num = kinds == KIND_NUMBER
    if lf.num_op in ("never", "always"):
        out[is_num] = lf.num_op == "always"
    else:
        with np.errstate(invalid="ignore"):
            out[is_num] = _NUM[lf.num_op](payload[is_num].view(np.float64), np.float64(lf.bound))
    is_str = kinds == KIND_STRING
    if lf.str_op in ("never", "always"):
        out[is_str] = lf.str_op == "always"
    else:
        if table is None:
            table = [bool(STRING_COMPARE[lf.str_op](s, lf.text)) for s in strings]
        table = np.asarray(table, dtype=bool)
        codes = payload[is_str].astype(np.int64)
        known = codes < len(table)
        answer = np.zeros(len(codes), dtype=bool)
        answer[known] = table[codes[known]]
        out[is_str] = answer
    return out


def any_per_row(elem_off: np.ndarray, answers: np.ndarray) -> np.ndarray:
    """OR of `answers[elem_off[r]:elem_off[r + 1]]` per row; an empty range gives False."""
    n = len(elem_off) - 1
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(elem_off))
    out = np.zeros(n, dtype=bool)
    out[row_of[answers]] = True
    return out


def interpret(program, columns, n_rows=None) -> np.ndarray:
    """The program over `columns[i]` = the MetaColumn of `program.keys[i]`, rows [0, n_rows), in numpy."""
    n = (len(columns[0]) if columns else 0) if n_rows is None else n_rows
    stack = []
    for op, i in program.ops:
        if op == "leaf":
            col = columns[program.leaves[i].column]
            stack.append(leaf_answers(program.leaves[i], col.strings, col.kinds[:n], col.payload[:n]))
        elif op == "list_any":
            col = columns[program.leaves[i].column]
            off = col.elem_off[: n + 1]
            stack.append(any_per_row(off, leaf_answers(program.leaves[i], col.strings, col.elem_kinds[: off[-1]], col.elem_payload[: off[-1]])))
        elif op == "not":
            stack.append(~stack.pop())
        else:
            b, a = stack.pop(), stack.pop()
            stack.append(a & b if op == "and" else a | b)
    assert len(stack) == 1
    return stack[0]
