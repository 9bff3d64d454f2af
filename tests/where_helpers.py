"""Shared by the metadata-filter tests: a direct Python evaluation of dict filters over metadata dicts (the meaning the
compiler must reproduce), a NumPy evaluation of compiled programs, an oracle engine that runs them, and random data /
filter generators."""
from __future__ import annotations

import math

import numpy as np

from mlvectordb_amd import where as W
from oracle import exact_scan
from oracle.engine import OracleScanEngine

SCHEMA = {"genre": "str", "year": "int", "price": "float", "in_stock": "bool"}
GENRES = ["jazz", "blues", "rock", "pop", "folk", "metal"]


# ---------------------------------------------------------------- the meaning of a dict filter, evaluated directly
def _value(meta, key, kind):
    v = None if meta is None else meta.get(key)
    if v is None or (kind == "float" and isinstance(v, float) and math.isnan(v)):
        return None
    return v


def _field(kind, op, v, lit):
    present = v is not None
    if op == "$eq":
        return present and v == lit
    if op == "$ne":
        return not (present and v == lit)
    if op == "$in":
        return present and any(v == x for x in lit)
    if op == "$nin":
        return not (present and any(v == x for x in lit))
    if op == "$exists":
        return present == bool(lit)
    if not present:
        return False
    return {"$lt": v < lit, "$lte": v <= lit, "$gt": v > lit, "$gte": v >= lit}[op]


def py_match(where, meta, schema=SCHEMA) -> bool:
    for key, val in where.items():
        if key == "$and":
            ok = all(py_match(w, meta, schema) for w in val)
        elif key == "$or":
            ok = any(py_match(w, meta, schema) for w in val)
        elif key == "$not":
            ok = not py_match(val, meta, schema)
        else:
            kind = schema[key]
            v = _value(meta, key, kind)
            if isinstance(val, dict):
                ok = all(_field(kind, op, v, lit) for op, lit in val.items())
            else:
                ok = _field(kind, "$eq", v, val)
        if not ok:
            return False
    return True


# ---------------------------------------------------------------- compiled programs, evaluated with NumPy
def eval_program(program: W.Program, cols: dict, n: int) -> np.ndarray:
    """bool [n]: rows the program matches (attribute columns as the device holds them: int64 / float64 with sentinels)."""
    stack = []
    table = program.set
    for op, attr, a, b in program.ops.tolist():
        if op == W.AND or op == W.OR:
            y, x = stack.pop(), stack.pop()
            stack.append(x & y if op == W.AND else x | y)
            continue
        if op == W.NOT:
            stack.append(~stack.pop())
            continue
        if op == W.TRUE:
            stack.append(np.ones(n, bool))
            continue
        col = cols[attr]
        if col.dtype == np.int64:
            have = col != W.INT64_ABSENT
            if op == W.IN:
                bit = have & np.isin(col, table[a:a + b])
            elif op == W.EXISTS:
                bit = have
            elif op == W.NE:
                bit = ~(have & (col == a))
            else:
                cmp = {W.EQ: np.equal, W.LT: np.less, W.LE: np.less_equal, W.GT: np.greater, W.GE: np.greater_equal}[op]
                bit = have & cmp(col, a)
        else:
            lit = np.array([a], dtype=np.int64).view(np.float64)[0]
            with np.errstate(invalid="ignore"):
                bit = {W.EQ: col == lit, W.NE: ~(col == lit), W.LT: col < lit, W.LE: col <= lit, W.GT: col > lit,
                       W.GE: col >= lit, W.EXISTS: col == col}[op]
        stack.append(bit)
    assert len(stack) == 1
    return stack[0]


class WhereOracleEngine(OracleScanEngine):
    """``OracleScanEngine`` + the attribute columns and ``where`` entries of ``HipScanEngine``, in NumPy."""

    def __init__(self, dim: int, space: str) -> None:
        super().__init__(dim, space)
        self._cols = {}

    def define_attr(self, attr, kind):
        self._cols[attr] = np.full(self._rows.shape[0], np.nan if kind == "float64" else W.INT64_ABSENT,
                                   dtype=np.float64 if kind == "float64" else np.int64)

    def _absent(self, col, n):
        return np.full(n, np.nan if col.dtype == np.float64 else W.INT64_ABSENT, dtype=col.dtype)

    def append(self, rows):
        first = super().append(rows)
        for a, col in self._cols.items():
            self._cols[a] = np.concatenate([col, self._absent(col, self._rows.shape[0] - col.size)])
        return first

    def compact(self):
        old = super().compact()
        self._cols = {a: col[old] for a, col in self._cols.items()}
        return old

    def close(self):
        super().close()
        self._cols = {a: col[:0] for a, col in self._cols.items()}

    def set_attr(self, attr, first, values):
        values = np.asarray(values)
        assert values.dtype == self._cols[attr].dtype and first + values.size <= self._rows.shape[0]
        self._cols[attr][first:first + values.size] = values

    def get_attr(self, attr, first, n, dtype=np.int64):
        return self._cols[attr][first:first + n].astype(dtype)

    def match(self, program) -> np.ndarray:
        return eval_program(program, self._cols, self._rows.shape[0]) & ~self._deleted

    def where_count(self, program):
        return int(self.match(program).sum())

    def where_labels(self, program):
        return np.flatnonzero(self.match(program)).astype(np.int64)

    def search(self, queries, k, mask=None, where=None):
        if where is not None:
            mask = self.match(where).astype(np.uint8)
        return super().search(queries, k, mask)

    def search64(self, queries, k, mask=None, where=None):
        if where is not None:
            mask = self.match(where).astype(np.uint8)
        return super().search64(queries, k, mask)

    def range(self, queries, radius, capacity, truncate=False, where=None):
        if where is None:
            return super().range(queries, radius, capacity, truncate)
        deleted = self._deleted | ~self.match(where)
        hits = exact_scan.range_query(queries, self._rows, radius, self.space, deleted=deleted)
        return [(l[:capacity], d[:capacity]) for l, d in hits] if truncate else hits


# ---------------------------------------------------------------- random data and filters
def random_metadata(rng, n, unseen=("zydeco",)):
    out = []
    for _ in range(n):
        m = {}
        if rng.random() < 0.8:
            m["genre"] = GENRES[rng.integers(len(GENRES))]
        if rng.random() < 0.8:
            m["year"] = int(rng.integers(1950, 2025))
        r = rng.random()
        if r < 0.7:
            m["price"] = float(np.round(rng.uniform(0, 100), 1))
        elif r < 0.8:
            m["price"] = float("nan")
        if rng.random() < 0.8:
            m["in_stock"] = bool(rng.random() < 0.5)
        if rng.random() < 0.05:
            m[["genre", "year", "price", "in_stock"][rng.integers(4)]] = None
        m["other"] = int(rng.integers(10))  # undeclared keys are carried, never indexed
        out.append(m)
    return out


def _literal(rng, key):
    if key == "genre":
        return (GENRES + ["zydeco"])[rng.integers(len(GENRES) + 1)]  # sometimes a string never ingested
    if key == "year":
        return int(rng.integers(1945, 2030))
    if key == "price":
        return [float(np.round(rng.uniform(-5, 105), 1)), int(rng.integers(0, 100))][rng.integers(2)]
    return bool(rng.random() < 0.5)


def random_leaf(rng):
    key = ["genre", "year", "price", "in_stock"][rng.integers(4)]
    ops = ["$eq", "$ne", "$in", "$nin", "$exists"] + ([] if key == "genre" else ["$lt", "$lte", "$gt", "$gte"])
    op = ops[rng.integers(len(ops))]
    if op == "$exists":
        return {key: {"$exists": bool(rng.random() < 0.5)}}
    if op in ("$in", "$nin"):
        return {key: {op: [_literal(rng, key) for _ in range(rng.integers(0, 4))]}}
    if op == "$eq" and rng.random() < 0.5:
        return {key: _literal(rng, key)}
    if key in ("year", "price") and rng.random() < 0.3:  # two operators on one key
        return {key: {"$gte": _literal(rng, key), "$lt": _literal(rng, key)}}
    return {key: {op: _literal(rng, key)}}


def random_filter(rng, depth=0):
    r = rng.random()
    if depth >= 2 or r < 0.45:
        return random_leaf(rng)
    if r < 0.6:
        return {"$not": random_filter(rng, depth + 1)}
    if r < 0.7:
        out = {}
        for _ in range(2):
            out.update(random_leaf(rng))
        return out
    comb = "$and" if r < 0.85 else "$or"
    return {comb: [random_filter(rng, depth + 1) for _ in range(rng.integers(0, 4))]}
