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


class EachOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``search_each`` / ``count_each``: every query searched alone under its own mask."""

    def search_each(self, queries, k, programs, program_of_query, want64=False, return_routes=False):
        nq = queries.shape[0]
        labels = np.empty((nq, k), np.int64)
        dist = np.empty((nq, k), np.float32)
        counts = np.empty(nq, np.int32)
        d64 = np.empty((nq, k))
        for i, p in enumerate(np.asarray(program_of_query).tolist()):
            where = None if p < 0 else programs[p]
            labels[i:i + 1], dist[i:i + 1], counts[i:i + 1], d64[i:i + 1] = self.search64(queries[i:i + 1], k, where=where)
        out = (labels, dist, counts, d64) if want64 else (labels, dist, counts)
        return out + (np.zeros(len(programs), np.int32),) if return_routes else out

    def count_each(self, programs):
        return np.array([self.where_count(p) for p in programs], dtype=np.int64)


class EachRangeOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``range_each``: every query ranged alone under its own mask; every call is counted."""

    each_calls = 0

    def range_each(self, queries, radius, capacity, programs, program_of_query, truncate=False, return_routes=False):
        type(self).each_calls += 1
        out = []
        for i, p in enumerate(np.asarray(program_of_query).tolist()):
            out.append(self.range(queries[i:i + 1], radius, capacity, truncate, where=None if p < 0 else programs[p])[0])
        return (out, np.zeros(len(programs), np.int32)) if return_routes else out


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


# ---------------------------------------------------------------- hostile columns and raw programs
# Value pools for the attribute columns and the literals of raw programs: the sentinels, the extremes of each type, and
# a few small values repeated often so that EQ / IN / LT / LE land on the values the rows hold.
INT64_MAX = np.iinfo(np.int64).max
INT_POOL = np.array([W.INT64_ABSENT, W.INT64_ABSENT + 1, W.INT64_ABSENT + 2, INT64_MAX, INT64_MAX - 1, -1, 0, 1,
                     2, 3, 7, 2, 3, 7, 2, 3], dtype=np.int64)
_F_BASE = [0.0, 1.0, -1.0, 1.5, 5e-324, np.finfo(np.float64).max, -np.finfo(np.float64).max]
with np.errstate(over="ignore"):  # (the neighbour of DBL_MAX above it is inf)
    FLOAT_POOL = np.array(
        [np.nan, -np.nan, np.array([0x7FF0000000000001], np.int64).view(np.float64)[0],  # NaNs: quiet, signed, signalling
         0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, np.finfo(np.float64).tiny]
        + _F_BASE + [np.nextafter(x, np.inf) for x in _F_BASE] + [np.nextafter(x, -np.inf) for x in _F_BASE]
        + [1.0, 1.5, 1.0, 1.5], dtype=np.float64)


def hostile_columns(rng, n, kinds):
    """{attr: column} with ``kinds[attr]`` in ("int64", "float64"), every value drawn from the pools above (INT64_MIN and
    NaN are the absent markers)."""
    return {a: (rng.choice(INT_POOL, n) if kind == "int64" else rng.choice(FLOAT_POOL, n)) for a, kind in kinds.items()}


def set_segments(rng):
    """An int64 table made of sorted ranges -> (table, [(offset, length), ...]): empty ranges, one entry, duplicates
    and a long run of ~500 entries, at offsets inside the one table."""
    parts = [np.sort(rng.choice(INT_POOL, 1)),                                      # one entry
             np.sort(rng.choice(INT_POOL, 6)),                                      # duplicates (a pool of repeats)
             np.sort(np.concatenate([rng.choice(INT_POOL, 8), rng.integers(-1000, 1000, 492)])),  # ~500 entries
             np.sort(rng.integers(-50, 50, int(rng.integers(2, 200))))]
    rng.shuffle(parts)
    ranges, table, at = [], [], 0
    for p in parts:
        ranges.append((at, 0))  # empty, at this offset
        ranges.append((at, p.size))
        table.append(p)
        at += p.size
    ranges.append((at, 0))  # empty, at the very end of the table
    return np.concatenate(table).astype(np.int64), ranges


def random_raw_program(rng, kinds, n_ops, deep=False, p_in=0.2):
    """A valid postfix ``W.Program`` of exactly ``n_ops`` ops over the columns ``kinds`` (attr -> kind), built directly
    (no dict compiler): leaves TRUE / EQ..GE / IN / EXISTS with literals from the value pools, AND / OR / NOT.
    ``deep``: push until the stack is MAX_DEPTH deep (64 ops reach exactly 32).  Its own set table from ``set_segments``."""
    table, ranges = set_segments(rng)
    attrs = list(kinds)
    int_attrs = [a for a in attrs if kinds[a] == "int64"]
    ops, depth, peak = [], 0, 0
    for i in range(n_ops):
        left = n_ops - i  # ops still to emit, this one included
        can_push = depth + 1 <= W.MAX_DEPTH and depth <= left - 1
        can_comb = depth >= 2
        can_not = depth >= 1 and depth - 1 <= left - 1
        if deep and can_push and peak < W.MAX_DEPTH:
            choice = "push"
        else:
            opts = [o for o, ok, w in (("push", can_push, 0.5), ("comb", can_comb, 0.35), ("not", can_not, 0.15)) if ok]
            wts = np.array([{"push": 0.5, "comb": 0.35, "not": 0.15}[o] for o in opts])
            choice = opts[rng.choice(len(opts), p=wts / wts.sum())]
        if choice == "comb":
            ops.append((W.AND if rng.random() < 0.5 else W.OR, 0, 0, 0))
            depth -= 1
        elif choice == "not":
            ops.append((W.NOT, 0, 0, 0))
        else:
            ops.append(_random_leaf_op(rng, kinds, attrs, int_attrs, ranges, p_in))
            depth += 1
            peak = max(peak, depth)
    assert depth == 1, (depth, n_ops)
    return W.Program(np.array(ops, dtype=W.OP_DTYPE), table)


def _random_leaf_op(rng, kinds, attrs, int_attrs, ranges, p_in):
    if int_attrs and rng.random() < p_in:
        a, b = ranges[rng.integers(len(ranges))]
        return (W.IN, int(int_attrs[rng.integers(len(int_attrs))]), a, b)
    r = rng.random()
    if r < 0.04:
        return (W.TRUE, 0, 0, 0)
    attr = int(attrs[rng.integers(len(attrs))])
    if r < 0.12:
        return (W.EXISTS, attr, 0, 0)
    op = (W.EQ, W.NE, W.LT, W.LE, W.GT, W.GE)[rng.integers(6)]
    if kinds[attr] == "int64":
        lit = int(rng.choice(INT_POOL))
    else:
        lit = int(FLOAT_POOL[rng.integers(FLOAT_POOL.size):][:1].view(np.int64)[0])  # the bits as drawn (NaN payloads)
    return (op, attr, lit, 0)


def program_depth(program: W.Program) -> int:
    """The deepest stack the program reaches."""
    d = deepest = 0
    for op in program.ops["op"].tolist():
        d += 1 if op <= W.EXISTS else (-1 if op in (W.AND, W.OR) else 0)
        deepest = max(deepest, d)
    return deepest
