"""Score expressions -> the postfix score program the device evaluates (include/mlvdb_score.h).

A score is an arithmetic expression over a row's distance to the query and its attributes; ``Index.search_scored`` returns
the rows with the smallest score, exactly, over all live matching rows.  The grammar:

    3, 0.25                                   a number
    "$distance"                               the row's distance in the index's space (l2: the squared distance)
    {"$attr": "likes", "$default": 0}         an int / float / bool attribute's value; ``$default`` (optional) stands in for
                                              an absent value -- without it such a row's score is NaN and the row is dropped
    {"$match": {"tier": "gold"}}              1.0 if the row matches the filter (a ``where`` dict), else 0.0
    {"$add": [a, b, ...]}  {"$mul": [...]}    n-ary, folded left to right: ((a + b) + c) ...
    {"$min": [...]}  {"$max": [...]}          likewise; a NaN operand makes the result NaN
    {"$sub": [a, b]}  {"$div": [a, b]}        binary
    {"$neg": e}  {"$abs": e}                  unary

Every operation is one IEEE-754 binary64 operation; NaN propagates through all of them (``0/0`` drops the row too), ``+-inf``
are ordinary scores.  Three recipes:

    bonus               {"$sub": ["$distance", {"$mul": [0.2, {"$match": {"tier": "gold"}}]}]}
    popularity          {"$div": ["$distance", {"$add": [1, {"$attr": "likes", "$default": 0}]}]}
    linear age penalty  {"$add": ["$distance", {"$mul": [0.3, {"$min": [1, {"$div": [{"$abs": {"$sub": [{"$attr": "year"},
                                                                                                      2024]}}, 10]}]}]}]}

Limits (``ValueError`` before the engine is touched): at most 32 ops, a value stack at most 8 deep, at most 8 ``$match``
filters of together at most 64 filter ops.  ``str``, list, sparse, geo and bits attributes hold no number and are refused by
name in ``$attr``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, List, Mapping, Tuple

import numpy as np

from . import where as where_mod
from .where import Program, float_bits

MAX_OPS = 32    # MLVDB_SCORE_MAX_OPS
MAX_DEPTH = 8   # MLVDB_SCORE_MAX_DEPTH
MAX_CONDS = 8   # MLVDB_SCORE_MAX_CONDS

# op codes (MLVDB_SCORE_*)
CONST, DIST, ATTR, MATCH, ADD, SUB, MUL, DIV, MIN, MAX, NEG, ABS = range(12)
OP_DTYPE = np.dtype([("op", "<i4"), ("attr", "<i4"), ("a", "<i8")])  # mlvdb_score_op

_NARY = {"$add": ADD, "$mul": MUL, "$min": MIN, "$max": MAX}
_BINARY = {"$sub": SUB, "$div": DIV}
_UNARY = {"$neg": NEG, "$abs": ABS}
_NAN_BITS = float_bits(float("nan"))


@dataclass
class ScoreProgram:
    """A compiled score: ``ops`` (structured array in the layout of ``mlvdb_score_op``) and the compiled filters the MATCH
    ops refer to."""

    ops: np.ndarray
    conds: List[Program] = field(default_factory=list)


def _is_number(x: Any) -> bool:
    return not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, np.integer, np.floating))


class _Builder:
    def __init__(self, schema: Mapping[str, str], strings) -> None:
        self.schema = schema
        self.index = {name: i for i, name in enumerate(schema)}
        self.strings = strings
        self.ops: List[Tuple[int, int, int]] = []
        self.conds: List[Program] = []

    def emit(self, op: int, attr: int = 0, a: int = 0) -> None:
        self.ops.append((op, attr, a))

    def node(self, e: Any) -> None:
        if _is_number(e):
            self.emit(CONST, 0, float_bits(float(e)))
            return
        if isinstance(e, str):
            if e != "$distance":
                raise ValueError(f"score: {e!r} is not an expression (the only string is '$distance')")
            self.emit(DIST)
            return
        if not isinstance(e, Mapping):
            raise ValueError(f"score: {e!r} is not an expression (a number, '$distance' or a dict)")
        if "$attr" in e:
            self.attr(e)
            return
        if len(e) != 1:
            raise ValueError(f"score: {dict(e)!r} must hold exactly one operator")
        (op, arg), = e.items()
        if op == "$match":
            if not isinstance(arg, Mapping):
                raise ValueError(f"score: $match takes a filter dict, got {arg!r}")
            try:
                cond = where_mod.compile_where(arg, self.schema, self.strings)
            except ValueError as err:
                raise ValueError(f"score: in {dict(e)!r}: {err}") from None
            self.emit(MATCH, 0, len(self.conds))
            self.conds.append(cond)
        elif op in _NARY:
            if not isinstance(arg, (list, tuple)) or len(arg) < 1:
                raise ValueError(f"score: {op} takes a list of at least one expression, got {arg!r}")
            for i, part in enumerate(arg):
                self.node(part)
                if i:
                    self.emit(_NARY[op])
        elif op in _BINARY:
            if not isinstance(arg, (list, tuple)) or len(arg) != 2:
                raise ValueError(f"score: {op} takes a list of exactly two expressions, got {arg!r}")
            self.node(arg[0])
            self.node(arg[1])
            self.emit(_BINARY[op])
        elif op in _UNARY:
            self.node(arg)
            self.emit(_UNARY[op])
        else:
            raise ValueError(f"score: unknown operator {op!r} in {dict(e)!r}")

    def attr(self, e: Mapping) -> None:
        extra = set(e) - {"$attr", "$default"}
        if extra:
            raise ValueError(f"score: {dict(e)!r}: an $attr operand takes '$attr' and '$default' only")
        name = e["$attr"]
        if name not in self.schema:
            raise ValueError(f"score: {name!r} is not a declared attribute of this index (declared: {sorted(self.schema)})")
        kind = self.schema[name]
        if kind not in ("int", "float", "bool"):
            raise ValueError(f"score: {name!r} is a {kind} attribute: $attr reads int, float and bool attributes only")
        default = _NAN_BITS
        if "$default" in e:
            if not _is_number(e["$default"]):
                raise ValueError(f"score: {dict(e)!r}: $default must be a number")
            default = float_bits(float(e["$default"]))
        self.emit(ATTR, self.index[name], default)

    def program(self) -> ScoreProgram:
        if len(self.ops) > MAX_OPS:
            raise ValueError(f"the score compiles to {len(self.ops)} ops; the device evaluates at most {MAX_OPS}")
        depth = deepest = 0
        for op, _, _ in self.ops:
            depth += 1 if op <= MATCH else -1 if op <= MAX else 0
            deepest = max(deepest, depth)
        if deepest > MAX_DEPTH:
            raise ValueError(f"the score needs a stack {deepest} deep; the device evaluates at most {MAX_DEPTH}")
        if len(self.conds) > MAX_CONDS:
            raise ValueError(f"the score holds {len(self.conds)} $match filters; the device evaluates at most {MAX_CONDS}")
        cond_ops = sum(int(c.ops.size) for c in self.conds)
        if cond_ops > where_mod.MAX_OPS:
            raise ValueError(f"the score's $match filters compile to {cond_ops} ops; the device evaluates at most "
                             f"{where_mod.MAX_OPS} in all")
        return ScoreProgram(np.array(self.ops, dtype=OP_DTYPE), self.conds)


def compile_score(score: Any, schema: Mapping[str, str], strings=None) -> ScoreProgram:
    """Compile ``score`` against ``schema`` (attribute name -> type, in declaration order: attribute i is column i) and the
    namespace's string dictionaries, which the ``$match`` filters are compiled with (``where.compile_where``)."""
    b = _Builder(schema, strings or {})
    b.node(score)
    return b.program()
