"""The subset of Milvus boolean filter expressions `GpuVectorStore` supports: one parser, compiled into Python predicates
(`parse_filter`) or into a postfix program for the row-filter kernel (`compile_filter`)."""
from __future__ import annotations

import operator
import re
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Any, List, Optional, Tuple


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


def like_elements(pattern: str) -> List[Tuple[str, str]]:
    """A `LIKE` pattern as elements: `("%", "")` any run of characters, `("_", "")` exactly one character, `("c", ch)` the
    character `ch` itself.  A backslash makes the next character literal; a trailing lone backslash is a ValueError."""
    out, i = [], 0
    while i < len(pattern):
        ch = pattern[i]
        if ch == "\\":
            if i + 1 == len(pattern):
                raise ValueError(f"GpuVectorStore: LIKE pattern {pattern!r} ends in a lone backslash")
            out.append(("c", pattern[i + 1]))
            i += 2
            continue
        out.append((ch, "") if ch in "%_" else ("c", ch))
        i += 1
    return out


def like_segments(pattern: str) -> int:
    """Non-empty runs of `_` and literal characters between the unescaped `%` of `pattern`: what the device matcher walks
    (VRAG_FILTER_MATCH_MAX_SEGMENTS)."""
    kinds = "".join("%" if kind == "%" else "x" for kind, _ch in like_elements(pattern))
    return len([run for run in kinds.split("%") if run])


@lru_cache(maxsize=256)
def _like_regex(pattern: str):
    return re.compile("".join(".*" if kind == "%" else "." if kind == "_" else re.escape(ch) for kind, ch in like_elements(pattern)),
                      re.S)


def like_match(stored: str, pattern: str) -> bool:
    """`stored LIKE pattern` (Milvus' pattern language): over the whole string, case-sensitive, one character = one code point,
    a newline a character like any other."""
    return _like_regex(pattern).fullmatch(stored) is not None


_LIST_FUNCTIONS = ("json_contains", "json_contains_any", "json_contains_all")


def parse_filter_ast(expr: str):
    """The parser both back ends share: `expr` -> a tree of `("cmp", key, op, want)` (op one of == != < <= > >=, `want` the
    literal's `_typed` key), `("in", key, [want, ...])`, `("like", key, pattern)`, `("has", key, want)` (the list `key` holds an
    element equal to `want`), `("not", a)`, `("and", a, b)`, `("or", a, b)` (`x not in [..]` is `("not", ("in", ..))`;
    `json_contains_any` is nested `("or", ..)` and `json_contains_all` nested `("and", ..)` of `has` nodes).  Raises ValueError
    for anything outside the grammar `parse_filter` states."""
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
            elif w == "LIKE":
                toks.append(("op", "LIKE"))
            elif w.lower() == "like":
                toks.append(("miscased", w))        # a field name where a field may stand, an error where the keyword would
            elif w.lower() in _LIST_FUNCTIONS:
                toks.append(("function", w))        # a function name in front of a `(`, a field name anywhere else
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

    def membership():
        """`json_contains(FIELD, VALUE)` / `json_contains_any(FIELD, [VALUE, ...])` / `json_contains_all(FIELD, [VALUE, ...])`,
        the name taken already."""
        name = toks[i - 1][1]
        if name not in _LIST_FUNCTIONS and name not in [n.upper() for n in _LIST_FUNCTIONS]:
            raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}: the list functions are written json_contains, "
                             f"json_contains_any, json_contains_all or JSON_CONTAINS, JSON_CONTAINS_ANY, JSON_CONTAINS_ALL "
                             f"(got {name!r})")
        name = name.lower()

        def need(kind, value, what):
            if peek() != (kind, value):
                raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}: {name} takes (field, "
                                 f"{'value' if name == 'json_contains' else '[value, ...]'}): expected {what}")
            take()

        def value():
            if peek()[0] != "val":
                raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}: {name} compares with a quoted string, a number or "
                                 f"true / false (a list or an object as an element is not supported)")
            return _typed(take())

        need("op", "(", "'('")
        if peek()[0] in ("miscased", "function"):
            toks[i] = ("field", peek()[1])
        if peek()[0] != "field":
            raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}: {name} takes a field first")
        key = take()
        need("op", ",", "','")
        if name == "json_contains":
            wants = [value()]
        else:
            need("op", "[", "a '[' that opens the list of values")
            if peek() == ("op", "]"):
                raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}: {name} with an empty list")
            wants = [value()]
            while peek() == ("op", ","):
                take()
                wants.append(value())
            need("op", "]", "']'")
        need("op", ")", "')'")
        tree = ("has", key, wants[0])
        for want in wants[1:]:
            tree = ("or" if name == "json_contains_any" else "and", tree, ("has", key, want))
        return tree

    def comparison():
        if peek() == ("op", "("):
            take()
            f = disjunction()
            take("op", ")")
            return f
        if peek() == ("op", "not"):
            take()
            return ("not", comparison())
        if peek()[0] == "function" and i + 1 < len(toks) and toks[i + 1] == ("op", "("):
            take()
            return membership()
        if peek()[0] in ("miscased", "function"):
            toks[i] = ("field", peek()[1])
        key = take("field")
        if peek()[0] == "miscased":
            raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}: the pattern-match keyword is LIKE, in upper case "
                             f"(got {peek()[1]!r})")
        op = take("op")
        if op == "LIKE":
            pattern = take("val")
            if not isinstance(pattern, str):
                raise ValueError(f"GpuVectorStore: LIKE needs a quoted pattern in filter {expr!r}")
            like_elements(pattern)                    # a trailing lone backslash is refused here
            return ("like", key, pattern)
        if op == "not":
            take("op", "in")
            op, negated = "in", True
        else:
            negated = False
        if op in ("==", "!="):
            return ("cmp", key, op, _typed(take("val")))
        if op == "in":
            take("op", "[")
            vals = [_typed(take("val"))]
            while peek() == ("op", ","):
                take()
                vals.append(_typed(take("val")))
            take("op", "]")
            return ("not", ("in", key, vals)) if negated else ("in", key, vals)
        if op in ("<", "<=", ">", ">="):
            want = _typed(take("val"))
            if want[0] == "b":
                raise ValueError(f"GpuVectorStore: ordering comparison with a boolean in filter {expr!r}")
            return ("cmp", key, op, want)
        raise ValueError(f"GpuVectorStore: unsupported operator {op!r} in filter {expr!r}")

    def conjunction():
        f = comparison()
        while peek() in (("op", "and"), ("op", "&&")):
            take()
            f = ("and", f, comparison())
        return f

    def disjunction():
        f = conjunction()
        while peek() in (("op", "or"), ("op", "||")):
            take()
            f = ("or", f, conjunction())
        return f

    tree = disjunction()
    if i != len(toks):
        raise ValueError(f"GpuVectorStore: unsupported filter {expr!r}")
    return tree


_ORDER = {"<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}


def _closure(node):
    """A tree of `parse_filter_ast` as `predicate(metadata: dict) -> bool`."""
    tag = node[0]
    if tag == "not":
        g = _closure(node[1])
        return lambda md: not g(md)
    if tag in ("and", "or"):
        a, b = _closure(node[1]), _closure(node[2])
        if tag == "and":
            return lambda md: a(md) and b(md)
        return lambda md: a(md) or b(md)
    if tag == "in":
        key, vals = node[1], node[2]
        vs = set(vals)
        f = lambda md: _typed(md.get(key)) in vs      # noqa: E731
        f.lookup = (key, vals)
        return f
    if tag == "has":
        key, want = node[1], node[2]

        def has(md):
            have = md.get(key)
            return isinstance(have, (list, tuple)) and any(_typed(e) == want for e in have)
        return has                                    # no `lookup`: the per-key value index holds scalars
    if tag == "like":
        key, matches = node[1], _like_regex(node[2]).fullmatch

        def like(md):
            have = md.get(key)
            return isinstance(have, str) and matches(have) is not None
        return like
    _tag, key, op, want = node
    if op == "!=":
        return lambda md: _typed(md.get(key)) != want
    if op == "==":
        f = lambda md: _typed(md.get(key)) == want   # noqa: E731
        f.lookup = (key, [want])                      # lets the store answer from a per-key value index
        return f
    cmp, (kind, bound) = _ORDER[op], want

    def ordered(md):
        have = _typed(md.get(key))
        return have is not None and have[0] == kind and cmp(have[1], bound)
    return ordered


def parse_filter(expr: str):
    """Compiles the subset of Milvus boolean expressions the store supports into `predicate(metadata: dict) -> bool`:
    `field == value`, `field != value`, `field in [v, ...]`, `field not in [v, ...]`, `field < / <= / > / >= value`,
    `field LIKE "pattern"`, combined with `and` / `&&`, `or` / `||`, `not` and parentheses.  field = `metadata["key"]` (the Local dialect) or a bare `key` (the Cloud
    dialect: index.py:735-739); value = a quoted string, a number (`7`, `-2.5`, `1e3`) or `true` / `false`.
    Comparisons are typed like Milvus' JSON path match: numbers against numeric metadata, strings against text,
    booleans against booleans; a missing key equals nothing (so `!=` holds for it).
    `LIKE` takes a quoted pattern in Milvus' pattern language: `%` matches any run of zero or more characters, `_` exactly one
    character (one code point: `Z_rich` matches `Zürich`), a backslash makes the next character literal (`\\%`, `\\_`, `\\\\`; a
    trailing lone backslash is a ValueError).  The match is over the whole string and case-sensitive, a newline is a character
    like any other, and only a stored string can match -- so `not (title LIKE "x%")` holds for numbers, booleans, None, lists,
    dicts and missing keys, as `not (title == "x")` does.  String literals have no escapes of their own: a pattern that needs
    a `"` is written in `'...'`.  The keyword is the upper-case word `LIKE` only, as the reference writes it; any other casing
    (`like`, `Like`) raises a ValueError that says so, and a metadata key named `LIKE` is written `metadata["LIKE"]`.
    Membership in list-valued metadata stands wherever a comparison may: `json_contains(field, value)`,
    `json_contains_any(field, [value, ...])` (some value is an element) and `json_contains_all(field, [value, ...])` (every
    value is an element).  `json_contains(k, v)` holds iff the stored `k` is a list -- a tuple counts as one: both are a JSON
    array, and a tuple is a list after a save / load -- and some element `e` has `_typed(e) == _typed(v)`: typed like `==`, so
    `2020` finds `2020.0`, `"5"` does not find `5`, `true` does not find `1`; elements that are None, lists or dicts match
    nothing.  A stored value that is no list (a missing key, a scalar, a dict) never passes, so `not json_contains(..)` holds
    for it, as `not (k == v)` does.  A word is a function name only when it is exactly one of the three names in lower case or
    exactly its upper-case form (`JSON_CONTAINS`, ..) and a `(` follows; anywhere else it stays a field name
    (`json_contains == 3` filters on a key of that name), and any other casing in front of a `(` raises a ValueError that names
    the accepted spellings.  An empty `[]`, a list or object literal as a value and a wrong number of arguments raise
    ValueError.  These are this store's semantics, not pinned against Milvus; `array_length`, index access, `is null` /
    `exists` and `TEXT_MATCH` are outside the grammar.
    Anything else raises ValueError -- a filter is never silently ignored."""
    return _closure(parse_filter_ast(expr))


# ---------------------------------------------------------------------------- the device back end
# The same tree as a postfix program over LEAVES for the row-filter kernel (include/vrag_amd.h, vrag_row_filter_eval).  A leaf is
# one comparison of one key and states what it answers for each KIND of stored value -- `_typed`'s kinds, each answer independent
# of the others:
#   other   (None, a list, a dict, a missing key)   a constant: 1 only for `!=`
#   bool                                             one answer for false, one for true
#   number                                           never / always / one IEEE f64 comparison against `bound`
#   string                                           never / always / a Python comparison against `text`, which the store applies
#                                                    once per distinct stored string (store_columns.MetaColumn.string_table) or
#                                                    the match kernel applies to the column's dictionary in HBM (csrc/strmatch.hip)
# `in [..]` is an OR of `==` leaves: a list may mix kinds.  `LIKE` is one leaf that only a string can answer (str_op "like").
# `has` is one `==` leaf pushed with "list_any": the OR, over the elements of the row's list, of what the leaf answers for the
# element (0 for a row that holds no list or an empty one) -- VRAG_FILTER_OP_LIST_ANY, csrc/listfilter.hip.
MAX_COLUMNS, MAX_LEAVES, MAX_OPS, MAX_DEPTH = 16, 64, 256, 32     # VRAG_FILTER_MAX_*
STRING_COMPARE = {"==": operator.eq, "!=": operator.ne, **_ORDER, "like": like_match}


@dataclass(frozen=True)
class FilterLeaf:
    column: int                     # index into FilterProgram.keys
    other: bool
    bools: Tuple[bool, bool]        # (answer for false, answer for true)
    num_op: str                     # "never" | "always" | "==" | "!=" | "<" | "<=" | ">" | ">="
    bound: float
    str_op: str                     # the same choices and "like", against `text`
    text: str


@dataclass
class FilterProgram:
    keys: List[str] = field(default_factory=list)                # referenced metadata keys, in first-use order
    leaves: List[FilterLeaf] = field(default_factory=list)
    ops: List[Tuple[str, int]] = field(default_factory=list)     # ("leaf", i) | ("list_any", i) | ("and", 0) | ("or", 0) | ("not", 0), postfix

    def depth(self) -> int:
        """Deepest the evaluation stack gets."""
        deepest = cur = 0
        for op, _i in self.ops:
            cur += 1 if op in ("leaf", "list_any") else (-1 if op in ("and", "or") else 0)
            deepest = max(deepest, cur)
        return deepest

    def over_limit(self) -> Optional[str]:
        """Why the device cannot run this program (one sentence), or None when it is within every limit."""
        for what, have, most in (("columns", len(self.keys), MAX_COLUMNS), ("leaves", len(self.leaves), MAX_LEAVES),
                                 ("ops", len(self.ops), MAX_OPS), ("stack depth", self.depth(), MAX_DEPTH)):
            if have > most:
                return f"{have} {what} (the device program holds at most {most})"
        return None


def _leaf(column: int, op: str, want) -> FilterLeaf:
    kind, value = want
    differs = op == "!="                                           # the one comparison that holds between different kinds
    rest = "always" if differs else "never"
    return FilterLeaf(
        column=column, other=differs,
        bools=tuple(STRING_COMPARE[op](b, value) for b in (False, True)) if kind == "b" else (differs, differs),
        num_op=op if kind == "n" else rest, bound=value if kind == "n" else 0.0,
        str_op=op if kind == "s" else rest, text=value if kind == "s" else "")


def compile_filter(expr: str) -> FilterProgram:
    """`expr` (the grammar of `parse_filter`, the same ValueErrors) as a `FilterProgram`: evaluated over the kinds and comparison
    keys `_typed` gives the stored values, it answers what `parse_filter(expr)` answers, row for row."""
    prog = FilterProgram()

    def push(key: str, op: str, want) -> None:
        if key not in prog.keys:
            prog.keys.append(key)
        prog.leaves.append(_leaf(prog.keys.index(key), op, want))
        prog.ops.append(("leaf", len(prog.leaves) - 1))

    def emit(node) -> None:
        tag = node[0]
        if tag == "cmp":
            push(node[1], node[2], node[3])
        elif tag == "has":
            push(node[1], "==", node[2])
            prog.ops[-1] = ("list_any", prog.ops[-1][1])
        elif tag == "like":
            if node[1] not in prog.keys:
                prog.keys.append(node[1])
            prog.leaves.append(FilterLeaf(column=prog.keys.index(node[1]), other=False, bools=(False, False), num_op="never",
                                          bound=0.0, str_op="like", text=node[2]))
            prog.ops.append(("leaf", len(prog.leaves) - 1))
        elif tag == "in":
            for n, want in enumerate(node[2]):
                push(node[1], "==", want)
                if n:
                    prog.ops.append(("or", 0))
        elif tag == "not":
            emit(node[1])
            prog.ops.append(("not", 0))
        else:
            emit(node[1])
            emit(node[2])
            prog.ops.append((tag, 0))

    emit(parse_filter_ast(expr))
    return prog
