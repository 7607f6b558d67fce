"""The subset of Milvus boolean filter expressions `GpuVectorStore` supports, compiled into Python predicates."""
from __future__ import annotations

import re
from typing import Any


_FILTER_TOKEN = re.compile(r"""\s*(?:(?P<meta>metadata\[\s*["'](?P<mkey>[^"']+)["']\s*\])|(?P<str>"[^"]*"|'[^']*')"""
                           r"""|(?P<num>-?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?)"""
                           r"""|(?P<op>==|!=|<=|>=|<|>|&&|\|\||[()\[\],])|(?P<word>\w+))""")


def _typed(value: Any):
    """Comparison key of a metadata value or a filter literal: JSON semantics, not text -- a number equals a number
    (2020 == 2020.0), a string equals a string ("5" != 5), booleans only booleans; anything else (None, a missing
    key, lists, dicts) equals nothing."""
    if isinstance(value, bool):
        return ("b", value)
    if isinstance(value, (int, float)):
        return ("n", float(value))
    if isinstance(value, str):
        return ("s", value)
    return None


def parse_filter(expr: str):
    """Compiles the subset of Milvus boolean expressions the store supports into `predicate(metadata: dict) -> bool`:
    `field == value`, `field != value`, `field in [v, ...]`, `field < / <= / > / >= value`, combined with `and` / `&&`,
    `or` / `||`, `not` and parentheses.  field = `metadata["key"]` (the Local dialect) or a bare `key` (the Cloud
    dialect: index.py:735-739); value = a quoted string, a number (`7`, `-2.5`, `1e3`) or `true` / `false`.
    Comparisons are typed like Milvus' JSON path match: numbers against numeric metadata, strings against text,
    booleans against booleans; a missing key equals nothing (so `!=` holds for it).  Anything else raises ValueError --
    a filter is never silently ignored."""
    toks, pos = [], 0
    while pos < len(expr):
        if expr[pos:].strip() == "":
            break
        m = _FILTER_TOKEN.match(expr, pos)
        if not m:
            raise ValueError(f"GpuVectorStore: cannot parse filter at {expr[pos:]!r}")
        pos = m.end()
        if m.group("meta"):
            toks.append(("field", m.group("mkey")))
        elif m.group("str"):
            toks.append(("val", m.group("str")[1:-1]))
        elif m.group("num"):
            toks.append(("val", float(m.group("num"))))
        elif m.group("op"):
            toks.append(("op", m.group("op")))
        else:
            w = m.group("word")
            if w.lower() in ("and", "or", "not", "in"):
                toks.append(("op", w.lower()))
            elif w.lower() in ("true", "false"):
                toks.append(("val", w.lower() == "true"))
            else:
                toks.append(("field", w))
    i = 0

    def peek():
        return toks[i] if i < len(toks) else (None, None)

    def take(kind=None, value=None):
        nonlocal i
        k, v = peek()
        if k is None or (kind and k != kind) or (value is not None and v != value):
            raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}")
        i += 1
        return v

    def comparison():
        if peek() == ("op", "("):
            take()
            f = disjunction()
            take("op", ")")
            return f
        if peek() == ("op", "not"):
            take()
            g = comparison()
            return lambda md: not g(md)
        key = take("field")
        op = take("op")
        if op in ("==", "!="):
            want = _typed(take("val"))
            if op == "!=":
                return lambda md: _typed(md.get(key)) != want
            f = lambda md: _typed(md.get(key)) == want   # noqa: E731
            f.lookup = (key, [want])                      # lets the store answer from a per-key value index
            return f
        if op == "in":
            take("op", "[")
            vals = [_typed(take("val"))]
            while peek() == ("op", ","):
                take()
                vals.append(_typed(take("val")))
            take("op", "]")
            vs = set(vals)
            f = lambda md: _typed(md.get(key)) in vs      # noqa: E731
            f.lookup = (key, vals)
            return f
        if op in ("<", "<=", ">", ">="):
            import operator

            cmp = {"<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}[op]
            kind, bound = _typed(take("val"))
            if kind == "b":
                raise ValueError(f"GpuVectorStore: ordering comparison with a boolean in filter {expr!r}")

            def ordered(md):
                have = _typed(md.get(key))
                return have is not None and have[0] == kind and cmp(have[1], bound)
            return ordered
        raise ValueError(f"GpuVectorStore: unsupported operator {op!r} in filter {expr!r}")

    def conjunction():
        f = comparison()
        while peek() in (("op", "and"), ("op", "&&")):
            take()
            g, h = f, comparison()
            f = (lambda a, b: lambda md: a(md) and b(md))(g, h)
        return f

    def disjunction():
        f = conjunction()
        while peek() in (("op", "or"), ("op", "||")):
            take()
            g, h = f, conjunction()
            f = (lambda a, b: lambda md: a(md) or b(md))(g, h)
        return f

    pred = disjunction()
    if i != len(toks):
        raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}")
    return pred
