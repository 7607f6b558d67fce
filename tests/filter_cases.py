"""Shared by the filter-program tests (host and GPU): seeded random metadata and filter expressions over the whole grammar of
`store_filter.parse_filter`, the expected answers (the Python predicate, row by row) and a small numpy interpreter of
`FilterProgram` over `store_columns.MetaColumn`s.  The interpreter is test code: the package never imports it."""
import operator
import random

import numpy as np

from verbatim_rag_amd.store_columns import KIND_BOOL, KIND_NUMBER, KIND_STRING, MetaColumn
from verbatim_rag_amd.store_filter import STRING_COMPARE, parse_filter

KEYS = ("year", "source", "peer", "score", "tag", "misc")
# what parse_filter must keep refusing (tests/test_host_parity.py)
BAD_FILTERS = ("a >", "a >> 3", "a > [1]", 'metadata["x"] like "y%"', "document_id == ", 'document_id == "d1" extra', "", '== "d1"')

_NUMBERS = (2020, 2020.0, 1999, 2026, 0, -0.0, 0.0, 1.5, -2.5, 7, float("inf"), float("-inf"), 2 ** 53 + 1, 2 ** 53, 1e3, -1)
_STRINGS = ("", "web", "journal", "5", "2020", "2020.0", "Zürich", "日本語", "a", "b", "true", "Web")
_OTHERS = (None, [1, 2], ["web"], {"a": 1}, [])


def _value(rng: random.Random):
    pick = rng.random()
    if pick < 0.40:
        return rng.choice(_NUMBERS)
    if pick < 0.70:
        return rng.choice(_STRINGS)
    if pick < 0.85:
        return rng.choice((True, False))
    return rng.choice(_OTHERS)


def random_rows(n: int, seed: int):
    """`n` metadata dicts without a NaN: every key is missing in a fifth of the rows and holds a number, a string, a bool or
    something incomparable otherwise."""
    rng = random.Random(seed)
    return [{k: _value(rng) for k in KEYS if rng.random() < 0.8} for _ in range(n)]


def _literal(rng: random.Random) -> str:
    pick = rng.random()
    if pick < 0.45:
        v = rng.choice(_NUMBERS + (2.02e3,))
        if v in (float("inf"), float("-inf")):
            return "1e999" if v > 0 else "-1e999"          # the grammar's spelling of an infinity
        return rng.choice((repr(v), f"{float(v):e}")) if rng.random() < 0.5 else repr(v)
    if pick < 0.85:
        s = rng.choice(_STRINGS)
        return rng.choice(('"%s"', "'%s'")) % s
    return rng.choice(("true", "false", "True", "FALSE"))


def _field(rng: random.Random) -> str:
    key = rng.choice(KEYS)
    return rng.choice((key, f'metadata["{key}"]', f"metadata['{key}']"))


def _comparison(rng: random.Random) -> str:
    while True:
        op = rng.choice(("==", "!=", "<", "<=", ">", ">=", "in"))
        if op == "in":
            return f"{_field(rng)} in [{', '.join(_literal(rng) for _ in range(rng.randint(1, 4)))}]"
        lit = _literal(rng)
        if op in ("<", "<=", ">", ">=") and lit.lower() in ("true", "false"):
            continue                                       # the grammar refuses an ordering comparison with a boolean
        return f"{_field(rng)} {op} {lit}"


def _expression(rng: random.Random, depth: int) -> str:
    if depth == 0 or rng.random() < 0.25:
        return _comparison(rng)
    pick = rng.random()
    if pick < 0.2:
        return f"not {_expression(rng, depth - 1)}" if rng.random() < 0.5 else f"not ({_expression(rng, depth - 1)})"
    if pick < 0.3:
        return f"({_expression(rng, depth - 1)})"
    word = rng.choice(("and", "or", "&&", "||", "AND", "Or"))
    return f"({_expression(rng, depth - 1)}) {word} ({_expression(rng, depth - 1)})" if rng.random() < 0.7 else \
        f"{_expression(rng, depth - 1)} {word} {_expression(rng, depth - 1)}"


def random_expressions(n: int, seed: int):
    """`n` expressions of the grammar: every operator, `in` lists mixing kinds, not / and / or / parentheses nested up to six
    deep, both field spellings."""
    rng = random.Random(seed)
    return [_expression(rng, i % 7) for i in range(n)]


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


def interpret(program, columns) -> np.ndarray:
    """The program over `columns[i]` = the MetaColumn of `program.keys[i]`, in numpy."""
    n = len(columns[0]) if columns else 0
    stack = []
    for op, i in program.ops:
        if op == "leaf":
            lf = program.leaves[i]
            col = columns[lf.column]
            kinds, payload = col.kinds, col.payload
            out = np.full(n, lf.other, dtype=bool)
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
                table = np.asarray([bool(STRING_COMPARE[lf.str_op](s, lf.text)) for s in col.strings] + [False], dtype=bool)
                out[is_str] = table[payload[is_str].astype(np.int64)]
            stack.append(out)
        elif op == "not":
            stack.append(~stack.pop())
        else:
            b, a = stack.pop(), stack.pop()
            stack.append(a & b if op == "and" else a | b)
    assert len(stack) == 1
    return stack[0]
