"""Milvus-style scalar filter expressions over the corpus's columns (`client.search(..., filter='level >= 2 and code like "E11%"')`).

The documented subset of Milvus's boolean expression grammar that the scalar fields of a row need (tools/build_database.py):

    expr      := or_expr
    or_expr   := and_expr (("or" | "||") and_expr)*
    and_expr  := not_expr (("and" | "&&") not_expr)*
    not_expr  := ("not" | "!") not_expr | "(" expr ")" | predicate
    predicate := FIELD ("==" | "!=" | "<" | "<=" | ">" | ">=") LITERAL
               | FIELD ["not"] "in" "[" [LITERAL ("," LITERAL)*] "]"
               | FIELD "like" STRING
               | "TEXT_MATCH" "(" FIELD "," STRING ["," "minimum_should_match" "=" INT] ")"

* FIELD: code, main_code, secondary_code, parent_code, category_path, preferred_zh (strings), level (int), has_complication
  (bool). Strings and bools take `==` and `!=` only; `like` takes strings only.
* LITERAL: a single- or double-quoted string (backslash escapes the next character), an int, true / false in any case.
  Keywords (and, or, not, in, like) are matched in any case too.
* like: "P%" prefix, "%S" suffix, "%X%" infix, no `%` = equality; `_` is an ordinary character.

* TEXT_MATCH (the name and the option keyword in any case): the rows whose text holds at least
  minimum_should_match (default 1, 1 .. 64) of the distinct terms `sparse_text.analyze` makes of STRING. FIELD is the text-indexed
  field (TEXT_FIELDS). Parsing needs no index; evaluating needs a matcher (`Columns.set_text_matcher`). No PHRASE_MATCH.

A syntax error, an unknown field or a type mismatch raises ValueError with the position (0-based, in characters) and the reason.
Nothing is evaluated by `eval`: the expression is parsed into a small tree and the tree is evaluated over whole column arrays.

`compile(expr)` returns the normalised key of an expression (equal for expressions that differ only in spelling: quotes,
case of keywords, `&&` / `and`, spaces, redundant parentheses). `select(expr, columns)` returns the sorted int64 row ids that
match; `Columns` caches its selections per normalised expression (a `Columns` belongs to one generation of the store).
"""
from __future__ import annotations

import re
import threading
from collections import OrderedDict
from functools import lru_cache
from typing import Any, Dict, List, Sequence, Tuple, Union

import numpy as np

STRING_FIELDS = ("code", "main_code", "secondary_code", "parent_code", "category_path", "preferred_zh")
INT_FIELDS = ("level",)
BOOL_FIELDS = ("has_complication",)
FIELDS = STRING_FIELDS + INT_FIELDS + BOOL_FIELDS
# grouping search (Milvus group_by_field): the eight fields, and `category` - an extension: the first element of category_path
# (the three-character category a code belongs to), the code itself where the path is empty
GROUP_FIELDS = FIELDS + ("category",)
MAX_GROUPED_HITS = 128   # include/icd_search.h ICD_MAX_K: top_k * group_size of one query
# keyword match (Milvus TEXT_MATCH): the field that carries the text index (MilvusService.build_sparse_index's default), and the
# bounds of minimum_should_match (include/icd_search.h ICD_SPARSE_MAX_QUERY_TERMS)
TEXT_FIELDS = ("preferred_zh",)
TEXT_MATCH_MAX_TERMS = 64
_CMP = ("==", "!=", "<", "<=", ">", ">=")
_KEYWORDS = ("and", "or", "not", "in", "like", "true", "false")

_TOKEN = re.compile(r"""
    (?P<ws>\s+)
  | (?P<str>"(?:[^"\\]|\\.)*"|'(?:[^'\\]|\\.)*')
  | (?P<int>-?\d+)
  | (?P<op>==|!=|<=|>=|&&|\|\||<|>|!|\(|\)|\[|\]|,)
  | (?P<opt>(?i:minimum_should_match)\s*=(?!=))
  | (?P<name>[A-Za-z_][A-Za-z0-9_]*)
""", re.X | re.S)


def _error(pos: int, reason: str) -> ValueError:
    return ValueError(f"filter expression, position {pos}: {reason}")


def _tokenize(expr: str) -> List[Tuple[str, Any, int]]:
    out, pos = [], 0
    while pos < len(expr):
        m = _TOKEN.match(expr, pos)
        if not m:
            if expr[pos] in "\"'":
                raise _error(pos, "unterminated string")
            raise _error(pos, f"unexpected character {expr[pos]!r}")
        kind = m.lastgroup
        text = m.group(kind)
        if kind == "str":
            out.append(("str", re.sub(r"\\(.)", r"\1", text[1:-1], flags=re.S), pos))
        elif kind == "int":
            out.append(("int", int(text), pos))
        elif kind == "op":
            out.append(("op", text, pos))
        elif kind == "opt":   # TEXT_MATCH's option keyword with its '=' (a lone '=' is no operator of the grammar)
            out.append(("opt", "minimum_should_match=", pos))
        elif kind == "name":
            low = text.lower()
            if low in ("true", "false"):
                out.append(("bool", low == "true", pos))
            elif low in _KEYWORDS:
                out.append(("kw", low, pos))
            else:
                out.append(("name", text, pos))
        pos = m.end()
    out.append(("end", None, len(expr)))
    return out


class _Parser:
    def __init__(self, expr: str):
        self.toks = _tokenize(expr)
        self.i = 0

    def peek(self):
        return self.toks[self.i]

    def take(self):
        t = self.toks[self.i]
        self.i += 1
        return t

    def at(self, kind, *values) -> bool:
        t = self.peek()
        return t[0] == kind and (not values or t[1] in values)

    def parse(self):
        if self.at("end"):
            raise _error(0, "empty expression")
        node = self.or_expr()
        if not self.at("end"):
            t = self.peek()
            raise _error(t[2], f"unexpected {self._show(t)} after a complete expression")
        return node

    def or_expr(self):
        terms = [self.and_expr()]
        while self.at("kw", "or") or self.at("op", "||"):
            self.take()
            terms.append(self.and_expr())
        return terms[0] if len(terms) == 1 else ("or", tuple(terms))

    def and_expr(self):
        terms = [self.not_expr()]
        while self.at("kw", "and") or self.at("op", "&&"):
            self.take()
            terms.append(self.not_expr())
        return terms[0] if len(terms) == 1 else ("and", tuple(terms))

    def not_expr(self):
        if self.at("kw", "not") or self.at("op", "!"):
            self.take()
            return ("not", self.not_expr())
        if self.at("op", "("):
            self.take()
            node = self.or_expr()
            t = self.take()
            if t[:2] != ("op", ")"):
                raise _error(t[2], f"expected ')', found {self._show(t)}")
            return node
        return self.predicate()

    @staticmethod
    def _show(t) -> str:
        return "the end of the expression" if t[0] == "end" else repr(t[1]) if t[0] == "str" else str(t[1]).lower() if t[0] == "bool" else str(t[1])

    def literal(self, field: str):
        t = self.take()
        if t[0] not in ("str", "int", "bool"):
            raise _error(t[2], f"expected a literal, found {self._show(t)}")
        want = "str" if field in STRING_FIELDS else "int" if field in INT_FIELDS else "bool"
        if t[0] != want:
            name = {"str": "string", "int": "int", "bool": "bool"}
            raise _error(t[2], f"type mismatch: {field} is {name[want]}, the literal {self._show(t)} is {name[t[0]]}")
        return t[1]

    def expect_op(self, value: str, where: str):
        t = self.take()
        if t[:2] != ("op", value):
            raise _error(t[2], f"expected '{value}' {where}, found {self._show(t)}")

    def text_match(self):
        """TEXT_MATCH "(" FIELD "," STRING ["," minimum_should_match "=" INT] ")" -> ("text_match", field, sorted distinct terms, m)"""
        from .sparse_text import analyze
        self.expect_op("(", "after TEXT_MATCH")
        t = self.take()
        if t[0] != "name":
            raise _error(t[2], f"TEXT_MATCH takes a field name first, found {self._show(t)}")
        field = t[1]
        if field not in FIELDS:
            raise _error(t[2], f"unknown field {field!r} (fields: {', '.join(FIELDS)})")
        if field not in STRING_FIELDS:
            raise _error(t[2], f"type mismatch: TEXT_MATCH is not defined on {field} (strings only)")
        if field not in TEXT_FIELDS:
            raise _error(t[2], f"TEXT_MATCH: {field} carries no text index (text-indexed: {', '.join(TEXT_FIELDS)})")
        self.expect_op(",", f"after TEXT_MATCH({field}")
        t = self.take()
        if t[0] != "str":
            raise _error(t[2], f"TEXT_MATCH takes a quoted text, found {self._show(t)}")
        terms = tuple(sorted(set(analyze(t[1]))))
        m = 1
        if self.at("op", ","):
            self.take()
            t = self.take()
            if t[0] != "opt":
                raise _error(t[2], f"expected minimum_should_match=, found {self._show(t)}")
            t = self.take()
            if t[0] != "int":
                raise _error(t[2], f"minimum_should_match takes an int, found {self._show(t)}")
            m = t[1]
            if not 1 <= m <= TEXT_MATCH_MAX_TERMS:
                raise _error(t[2], f"minimum_should_match={m}: must lie in 1 .. {TEXT_MATCH_MAX_TERMS}")
        self.expect_op(")", "to close TEXT_MATCH")
        return ("text_match", field, terms, m)

    def predicate(self):
        t = self.take()
        if t[0] != "name":
            raise _error(t[2], f"expected a field name, found {self._show(t)}")
        if t[1].lower() == "text_match" and self.at("op", "("):
            return self.text_match()
        field, fpos = t[1], t[2]
        if field not in FIELDS:
            raise _error(fpos, f"unknown field {field!r} (fields: {', '.join(FIELDS)})")
        op = self.peek()
        if op[0] == "op" and op[1] in _CMP:
            self.take()
            if field not in INT_FIELDS and op[1] not in ("==", "!="):
                raise _error(op[2], f"type mismatch: {op[1]} is not defined on {field} (only == and != are)")
            return ("cmp", field, op[1], self.literal(field))
        negate = False
        if op[:2] == ("kw", "not"):
            self.take()
            negate = True
            op = self.peek()
            if op[:2] != ("kw", "in"):
                raise _error(op[2], f"expected 'in' after '{field} not', found {self._show(op)}")
        if op[:2] == ("kw", "in"):
            self.take()
            t = self.take()
            if t[:2] != ("op", "["):
                raise _error(t[2], f"expected '[' after 'in', found {self._show(t)}")
            values = []
            if self.at("op", "]"):
                self.take()
            else:
                while True:
                    values.append(self.literal(field))
                    t = self.take()
                    if t[:2] == ("op", "]"):
                        break
                    if t[:2] != ("op", ","):
                        raise _error(t[2], f"expected ',' or ']' in the list, found {self._show(t)}")
            # (a canonical list: sorted, without repeats - the normalised key does not depend on how the list was written)
            return ("in", field, negate, tuple(sorted(set(values), key=lambda v: (str(type(v)), v))))
        if op[:2] == ("kw", "like"):
            self.take()
            if field not in STRING_FIELDS:
                raise _error(op[2], f"type mismatch: like is not defined on {field} (strings only)")
            t = self.take()
            if t[0] != "str":
                raise _error(t[2], f"like takes a quoted pattern, found {self._show(t)}")
            pat = t[1]
            if len(pat) >= 2 and pat[0] == "%" and pat[-1] == "%":
                how, text = "infix", pat[1:-1]
            elif pat.startswith("%"):
                how, text = "suffix", pat[1:]
            elif pat.endswith("%"):
                how, text = "prefix", pat[:-1]
            else:
                how, text = "eq", pat
            if "%" in text:
                raise _error(t[2], f"like pattern {pat!r}: only a leading and / or trailing % is supported")
            return ("cmp", field, "==", text) if how == "eq" else ("like", field, how, text)
        raise _error(op[2], f"expected a comparison, 'in', 'not in' or 'like' after {field}, found {self._show(op)}")


def _quote(v) -> str:
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, int):
        return str(v)
    return '"' + v.replace("\\", "\\\\").replace('"', '\\"') + '"'


def _key(node) -> str:
    kind = node[0]
    if kind == "cmp":
        return f"{node[1]} {node[2]} {_quote(node[3])}"
    if kind == "in":
        return f"{node[1]} {'not in' if node[2] else 'in'} [{', '.join(_quote(v) for v in node[3])}]"
    if kind == "like":
        pat = {"prefix": "{}%", "suffix": "%{}", "infix": "%{}%"}[node[2]].format(node[3])
        return f"{node[1]} like {_quote(pat)}"
    if kind == "text_match":   # (the analysed terms hold no quote and no space: the key is an expression again)
        return f"TEXT_MATCH({node[1]}, {_quote(' '.join(node[2]))}, minimum_should_match={node[3]})"
    if kind == "not":
        return f"not ({_key(node[1])})"
    return f" {kind} ".join(f"({_key(t)})" for t in node[1])


@lru_cache(maxsize=512)
def _parse(expr: str):
    if not isinstance(expr, str):
        raise ValueError(f"filter expression must be a string, not {type(expr).__name__}")
    node = _Parser(expr).parse()
    return node, _key(node)


def parse(expr: str):
    """the expression's tree (nested tuples); raises ValueError"""
    return _parse(expr)[0]


def compile(expr: str) -> str:   # noqa: A001 (the name the issue gives the entry point)
    """the normalised key of `expr`; raises ValueError on a syntax error, an unknown field or a type mismatch"""
    return _parse(expr)[1]


def _has_text_match(node) -> bool:
    if node[0] in ("and", "or"):
        return any(_has_text_match(t) for t in node[1])
    if node[0] == "not":
        return _has_text_match(node[1])
    return node[0] == "text_match"


def has_text_match(expr: str) -> bool:
    """whether `expr` holds a TEXT_MATCH predicate anywhere (evaluating it then needs a matcher)"""
    return _has_text_match(_parse(expr)[0])


def text_match_shape(expr: str):
    """The shapes a TEXT_MATCH expression's mask is built on the device for: a lone TEXT_MATCH(...), or a
    top-level conjunction with exactly one TEXT_MATCH among predicates S that hold none. Returns (S, field, terms, m) - S the
    normalised expression of the other conjuncts, None for a lone TEXT_MATCH - or None for every other expression (no
    TEXT_MATCH at all, one under `or` / `not` or in a nested conjunction, two of them): those are evaluated on the host."""
    node = _parse(expr)[0]
    if node[0] == "text_match":
        return None, node[1], node[2], node[3]
    if node[0] != "and":
        return None
    text = [t for t in node[1] if t[0] == "text_match"]
    rest = [t for t in node[1] if t[0] != "text_match"]
    if len(text) != 1 or any(_has_text_match(t) for t in rest):
        return None
    return _key(rest[0] if len(rest) == 1 else ("and", tuple(rest))), text[0][1], text[0][2], text[0][3]


def check_grouping(field, top_k, group_size) -> None:
    """the arguments of a grouping search (group_by_field, limit, group_size); ValueError names the offending limit"""
    if not isinstance(field, str) or field not in GROUP_FIELDS:
        raise ValueError(f"group_by_field={field!r}: not one of {', '.join(GROUP_FIELDS)}")
    if isinstance(group_size, bool) or not isinstance(group_size, (int, np.integer)) or group_size < 1:
        raise ValueError(f"group_size={group_size!r}: must be an integer >= 1")
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 1:
        raise ValueError(f"top_k={top_k!r}: must be an integer >= 1")
    if int(top_k) * int(group_size) > MAX_GROUPED_HITS:
        raise ValueError(f"top_k * group_size = {int(top_k) * int(group_size)} exceeds {MAX_GROUPED_HITS} hits per query "
                         f"(top_k={top_k} groups of group_size={group_size})")


GROUP_SCORERS = ("max", "sum", "avg")   # Milvus's group scorers: what a group of a grouping search ranks by


def check_group_scorer(field, group_scorer) -> None:
    """group_scorer of a call: None (not given: a group ranks by its best row, nothing new runs) or one of GROUP_SCORERS next to
    group_by_field; anything else is a ValueError"""
    if group_scorer is None:
        return
    if not isinstance(group_scorer, str) or group_scorer not in GROUP_SCORERS:
        raise ValueError(f"group_scorer={group_scorer!r}: not one of {', '.join(GROUP_SCORERS)}")
    if field is None:
        raise ValueError("group_scorer needs group_by_field")


class Columns:
    """The eight filter fields of a store's rows as column arrays, built once per generation of the store, with a bounded cache
    of selections keyed by the normalised expression. `generation` is the store's mutation counter when the columns were built."""

    CACHE = 64

    def __init__(self, arrays: Dict[str, np.ndarray], generation: int = 0):
        self.arrays = arrays
        self.generation = generation
        self.n = len(next(iter(arrays.values()))) if arrays else 0
        self._sel: "OrderedDict[str, np.ndarray]" = OrderedDict()
        self._groups: Dict[str, Any] = {}
        self._matchers: Dict[str, Any] = {}
        self._device_cols = None   # (device_columns(),) once built
        self._lock = threading.Lock()

    @classmethod
    def from_records(cls, records: Sequence[Dict[str, Any]], generation: int = 0) -> "Columns":
        arrays: Dict[str, np.ndarray] = {}
        for f in STRING_FIELDS:
            arrays[f] = np.array(["" if r.get(f) is None else str(r.get(f)) for r in records], dtype=str) if len(records) \
                else np.zeros(0, dtype="<U1")
        arrays["level"] = np.fromiter((int(r.get("level", 1)) for r in records), dtype=np.int64, count=len(records))
        arrays["has_complication"] = np.fromiter((bool(r.get("has_complication", False)) for r in records), dtype=bool, count=len(records))
        return cls(arrays, generation)

    def __getitem__(self, field: str) -> np.ndarray:
        return self.arrays[field]

    def group_ids(self, field: str):
        """(ids int32 [n], values): the rows' group under `field` as the rank of its value among the sorted distinct values
        (values[ids[row]] is the row's value). An empty string is a value like any other: the rows without a parent_code form
        one group. Cached per field."""
        check_grouping(field, 1, 1)
        with self._lock:
            hit = self._groups.get(field)
        if hit is not None:
            return hit
        if field == "category":
            path, code = self.arrays["category_path"], self.arrays["code"]
            col = np.array([(p.split(">")[0].strip() or c) for p, c in zip(path.tolist(), code.tolist())], dtype=str) if self.n \
                else np.zeros(0, dtype="<U1")
        else:
            col = self.arrays[field]
        values, ids = np.unique(col, return_inverse=True)
        out = (np.ascontiguousarray(ids.reshape(-1), dtype=np.int32), values)
        out[0].setflags(write=False)
        with self._lock:
            self._groups[field] = out
        return out

    def device_columns(self):
        """int32 [len(DEVICE_COLUMNS), n], C-contiguous: what IcdColumns uploads. A string field goes in as
        group_ids(field) - the rank of the row's value among the sorted distinct values -, level as it is, has_complication as
        0 / 1. None when a level does not fit (INT32_MIN, INT32_MAX): such a store keeps the host route. Cached."""
        with self._lock:
            hit = self._device_cols
        if hit is not None:
            return hit[0]
        level = self.arrays["level"]
        if self.n and (int(level.min()) <= _I32_MIN or int(level.max()) >= _I32_MAX):
            out = None
        else:
            out = np.empty((len(DEVICE_COLUMNS), self.n), np.int32)
            for c, f in enumerate(DEVICE_COLUMNS):
                out[c] = self.group_ids(f)[0] if f in STRING_FIELDS else self.arrays[f].astype(np.int32)
            out.setflags(write=False)
        with self._lock:
            self._device_cols = (out,)
        return out

    def set_text_matcher(self, field: str, fn) -> None:
        """The matcher TEXT_MATCH(field, ...) is evaluated with: fn(terms, m) -> bool[n], terms the analysed distinct terms of
        the predicate's text, m its minimum_should_match (sparse_text.SparseTextIndex.match_rows over the same rows). Selections
        cached under another matcher are dropped."""
        with self._lock:
            if self._matchers.get(field) is fn:
                return
            self._matchers[field] = fn
            for key in [k for k in self._sel if "TEXT_MATCH(" in k]:
                del self._sel[key]

    def select(self, expr: str) -> np.ndarray:
        node, key = _parse(expr)
        with self._lock:
            hit = self._sel.get(key)
            if hit is not None:
                self._sel.move_to_end(key)
                return hit
        rows = np.flatnonzero(_eval(node, self.arrays, self.n, self._matchers)).astype(np.int64)
        rows.setflags(write=False)
        with self._lock:
            self._sel[key] = rows
            while len(self._sel) > self.CACHE:
                self._sel.popitem(last=False)
        return rows


def _eval(node, cols, n: int, matchers=None) -> np.ndarray:
    kind = node[0]
    if kind == "and":
        m = _eval(node[1][0], cols, n, matchers)
        for t in node[1][1:]:
            m = m & _eval(t, cols, n, matchers)
        return m
    if kind == "or":
        m = _eval(node[1][0], cols, n, matchers)
        for t in node[1][1:]:
            m = m | _eval(t, cols, n, matchers)
        return m
    if kind == "not":
        return ~_eval(node[1], cols, n, matchers)
    if kind == "text_match":
        fn = (matchers or {}).get(node[1])
        if fn is None:
            raise ValueError(f"TEXT_MATCH: no sparse index on {node[1]}: call build_sparse_index")
        return np.asarray(fn(node[2], node[3]), dtype=bool).reshape(n)
    col = cols[node[1]]
    if kind == "cmp":
        op, v = node[2], node[3]
        if op == "==":
            return np.asarray(col == v, dtype=bool).reshape(n)
        if op == "!=":
            return np.asarray(col != v, dtype=bool).reshape(n)
        return {"<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}[op](col, v)
    if kind == "in":
        m = np.isin(col, np.array(node[3], dtype=col.dtype)) if node[3] else np.zeros(n, dtype=bool)
        return ~m if node[2] else m
    if kind == "like":
        how, s = node[2], node[3]
        if how == "prefix":
            return np.char.startswith(col, s) if n else np.zeros(0, bool)
        if how == "suffix":
            return np.char.endswith(col, s) if n else np.zeros(0, bool)
        return np.char.find(col, s) >= 0 if n else np.zeros(0, bool)
    raise AssertionError(kind)


def select(expr: str, columns: Union[Columns, Dict[str, np.ndarray]]) -> np.ndarray:
    """sorted int64 row ids whose columns satisfy `expr`. `columns`: a Columns (selections cached per normalised expression) or a
    dict field -> array of equal length (evaluated every time). Raises ValueError on a bad expression."""
    if isinstance(columns, Columns):
        return columns.select(expr)
    node = parse(expr)
    n = len(next(iter(columns.values()))) if columns else 0
    cols = {f: (np.asarray(c) if f not in STRING_FIELDS else np.asarray(c, dtype=str)) for f, c in columns.items()}
    missing = [f for f in _fields_of(node) if f not in cols]
    if missing:
        raise ValueError(f"filter expression needs column(s) {missing} that were not given")
    return np.flatnonzero(_eval(node, cols, n)).astype(np.int64)   # (a TEXT_MATCH needs a Columns with its matcher: ValueError here)


# ---- filter programs for the device (the word layout is include/icd_search.h's) ---------------------------------
DEVICE_COLUMNS = FIELDS   # column c of Columns.device_columns() is field DEVICE_COLUMNS[c]
OP_RANGE, OP_SET, OP_TEXT, OP_AND, OP_OR, OP_NOT = 1, 2, 3, 4, 5, 6
PROGRAM_MAX_OPS, PROGRAM_MAX_LEAVES, PROGRAM_MAX_STACK, PROGRAM_MAX_TEXT, PROGRAM_MAX_SET = 32, 16, 8, 4, 64
_I32_MIN, _I32_MAX = -2 ** 31, 2 ** 31 - 1


class _NoProgram(Exception):
    """the tree does not fit a device program: the host route evaluates it"""


def _u32(v: int) -> int:
    return int(v) & 0xFFFFFFFF


def _clamp(v: int) -> int:
    return min(max(int(v), _I32_MIN), _I32_MAX)


def _prefix_range(values: np.ndarray, prefix: str) -> Tuple[int, int]:
    """[lo, hi) of the sorted distinct `values` that start with `prefix`: contiguous in code-point order, found with two binary
    searches and verified at the range's four borders (anything else: _NoProgram)"""
    if prefix == "":
        return 0, len(values)
    lo = int(np.searchsorted(values, prefix, side="left"))
    last = ord(prefix[-1])
    if last >= 0x10FFFF:
        raise _NoProgram
    hi = int(np.searchsorted(values, prefix[:-1] + chr(last + 1), side="left"))
    ok = lo <= hi and (hi == lo or (str(values[lo]).startswith(prefix) and str(values[hi - 1]).startswith(prefix)))
    ok = ok and (lo == 0 or not str(values[lo - 1]).startswith(prefix)) and (hi == len(values) or not str(values[hi]).startswith(prefix))
    if not ok:
        raise _NoProgram
    return lo, hi


def _leaf(node, columns: "Columns", text_index) -> Tuple[List[int], bool]:
    """(the leaf's words, whether a NOT follows it) of a predicate node"""
    kind = node[0]
    if kind == "text_match":
        tx = (text_index or {}).get(node[1])
        if tx is None:
            raise _NoProgram
        try:
            known, _total = tx.match_terms(node[2])
        except ValueError:
            raise _NoProgram from None
        return [OP_TEXT | len(known) << 8 | int(node[3]) << 16] + [int(t) for t in known], False
    field = node[1]
    col = DEVICE_COLUMNS.index(field)
    if field in STRING_FIELDS:
        values = columns.group_ids(field)[1]
        if kind == "cmp":   # (== or !=: the parser admits nothing else on a string)
            at = int(np.searchsorted(values, node[3], side="left")) if len(values) else 0
            lo, hi = (at, at + 1) if at < len(values) and str(values[at]) == node[3] else (0, 0)
            return [OP_RANGE, col, lo, hi], node[2] == "!="
        if kind == "like" and (node[2] == "prefix" or node[3] == ""):   # (an empty suffix or infix is the empty prefix: every value)
            lo, hi = _prefix_range(values, node[3])
            return [OP_RANGE, col, lo, hi], False
        if kind == "like":
            if not len(values):
                ids = np.zeros(0, np.int64)
            else:
                ids = np.flatnonzero(np.char.endswith(values, node[3]) if node[2] == "suffix" else np.char.find(values, node[3]) >= 0)
        else:   # in / not in
            ids = np.flatnonzero(np.isin(values, np.array(node[3], dtype=values.dtype))) if node[3] and len(values) else np.zeros(0, np.int64)
        if len(ids) > PROGRAM_MAX_SET:
            raise _NoProgram
        return [OP_SET | len(ids) << 8, col] + [int(i) for i in ids], kind == "in" and node[2]
    if kind == "cmp":
        v, op = int(node[3]), node[2]   # (a bool literal is 0 / 1, as its column)
        lo, hi = {"==": (v, v + 1), "!=": (v, v + 1), "<": (_I32_MIN, v), "<=": (_I32_MIN, v + 1), ">": (v + 1, _I32_MAX), ">=": (v, _I32_MAX)}[op]
        # (device_columns() admits no value of INT32_MAX: hi = INT32_MAX is "no upper bound")
        return [OP_RANGE, col, _u32(_clamp(lo)), _u32(_clamp(hi))], op == "!="
    if kind == "in":
        ids = sorted({int(v) for v in node[3] if _I32_MIN <= int(v) <= _I32_MAX})
        if len(ids) > PROGRAM_MAX_SET:
            raise _NoProgram
        return [OP_SET | len(ids) << 8, col] + [_u32(i) for i in ids], bool(node[2])
    raise AssertionError(kind)


def device_program(expr: str, columns: "Columns", text_index=None):
    """`expr` as a postfix program for IcdIndex.filter_masks: uint32 words over the columns of
    `columns.device_columns()`, or None when the tree does not fit - more than 16 leaves or 32 operations, a set above 64 values,
    more than 8 sets on the stack, more than 4 TEXT_MATCHes, a TEXT_MATCH on a field without an entry in `text_index` (a dict
    field -> SparseTextIndex) or with more than 64 known terms, a prefix whose values are not contiguous among the sorted distinct
    values, a column that does not fit int32. None means the host route (`select`). Operands are evaluated in the order written.
    A string predicate becomes an integer predicate on the value's rank among the field's sorted distinct values: == and a prefix
    `like` a rank range, `in` and suffix / infix `like` a rank set, != and `not in` the NOT of those."""
    node = _parse(expr)[0]
    if columns.device_columns() is None:
        return None
    words: List[int] = []
    tally = {"ops": 0, "leaves": 0, "text": 0, "depth": 0}

    def op(word):
        words.append(word)
        tally["ops"] += 1

    def emit(t):
        if t[0] in ("and", "or"):
            emit(t[1][0])
            for u in t[1][1:]:
                emit(u)
                op(OP_AND if t[0] == "and" else OP_OR)
                tally["depth"] -= 1
        elif t[0] == "not":
            emit(t[1])
            op(OP_NOT)
        else:
            leaf, negate = _leaf(t, columns, text_index)
            words.extend(leaf)
            tally["ops"] += 1
            tally["leaves"] += 1
            tally["text"] += t[0] == "text_match"
            tally["depth"] += 1
            if tally["depth"] > PROGRAM_MAX_STACK or tally["leaves"] > PROGRAM_MAX_LEAVES or tally["text"] > PROGRAM_MAX_TEXT:
                raise _NoProgram
            if negate:
                op(OP_NOT)
        if tally["ops"] > PROGRAM_MAX_OPS:
            raise _NoProgram

    try:
        emit(node)
    except _NoProgram:
        return None
    return np.asarray(words, dtype=np.uint32)


def pack_programs(programs: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """(prog_off int64 [nq + 1], prog uint32) of a batch of device programs"""
    off = np.zeros(len(programs) + 1, np.int64)
    np.cumsum([len(p) for p in programs], out=off[1:])
    return off, (np.concatenate(programs).astype(np.uint32) if len(programs) else np.zeros(0, np.uint32))


def _fields_of(node) -> List[str]:
    if node[0] in ("and", "or"):
        return [f for t in node[1] for f in _fields_of(t)]
    if node[0] == "not":
        return _fields_of(node[1])
    return [] if node[0] == "text_match" else [node[1]]
