"""Shared by the list-attribute tests (include/mlvdb_list.h): a model engine that keeps every row's list as a Python set
and answers the list entries of ``HipScanEngine`` from those sets, the meaning of the list operators of a dict filter
evaluated directly on metadata dicts, and seeded generators of tagged metadata, dict filters and raw programs.  Nothing
here asks the library for an answer: ``where.ListColumn`` is used as the plain CSR container the engines exchange."""
from __future__ import annotations

from collections import Counter

import numpy as np

from mlvectordb_amd import where as W
from mlvectordb_amd.engine import FacetOverflow
from tests.mutate_helpers import MutateOracleEngine
from tests.where_helpers import _field, eval_program

INT64_MAX = 2 ** 63 - 1
INT64_MIN = -(2 ** 63)
TAG_SCHEMA = {"tags": "str[]", "nums": "int[]", "year": "int", "price": "float"}
TAGS = ["jazz", "live", "1959", "blues", "vinyl", "remaster", "mono", "bootleg"]
COMBINATORS = (W.AND, W.OR, W.NOT)


def csr(lists) -> W.ListColumn:
    """Rows as ``None`` / iterables of ints -> the CSR container (each list sorted, duplicates dropped)."""
    offsets, values, present = [0], [], []
    for row in lists:
        present.append(0 if row is None else 1)
        values.extend(sorted(set(row or ())))
        offsets.append(len(values))
    return W.ListColumn(np.array(offsets, dtype=np.int64), np.array(values, dtype=np.int64), np.array(present, dtype=np.uint8))


def uncsr(col: W.ListColumn):
    """The CSR container -> rows as ``None`` / frozensets."""
    off, vals = col.offsets.tolist(), col.values.tolist()
    return [frozenset(vals[off[i]:off[i + 1]]) if p else None for i, p in enumerate(col.present.tolist())]


# ---------------------------------------------------------------- compiled programs over columns and sets
def eval_list_program(program: W.Program, cols: dict, lists: dict, n: int) -> np.ndarray:
    """bool [n]: ``where_helpers.eval_program`` + the four list ops, read off ``lists[attr]`` (a Python list of ``None`` /
    sets).  Scalar ops and EXISTS go to ``eval_program`` one op at a time (a list column's ``cols`` entry holds the row's
    length, INT64_MIN when it has no list)."""
    stack = []
    table = program.set.tolist()
    for i, (op, attr, a, b) in enumerate(program.ops.tolist()):
        if op == W.AND or op == W.OR:
            y, x = stack.pop(), stack.pop()
            stack.append(x & y if op == W.AND else x | y)
        elif op == W.NOT:
            stack.append(~stack.pop())
        elif op in (W.HAS, W.HAS_ANY, W.HAS_ALL, W.LEN):
            rows = lists[attr]
            want = set(table[a:a + b])
            if op == W.HAS:
                bit = [r is not None and a in r for r in rows]
            elif op == W.HAS_ANY:
                bit = [r is not None and not want.isdisjoint(r) for r in rows]
            elif op == W.HAS_ALL:
                bit = [r is not None and want <= r for r in rows]
            else:
                bit = [r is not None and a <= len(r) <= b for r in rows]
            stack.append(np.array(bit, dtype=bool).reshape(n))
        else:
            stack.append(eval_program(W.Program(program.ops[i:i + 1], program.set), cols, n))
    assert len(stack) == 1
    return stack[0]


class TagsOracleEngine(MutateOracleEngine):
    """The oracle engine + list columns kept as Python sets: ``self._lists[attr][row]`` is ``None`` or a frozenset, and the
    inherited int64 column of a list attribute holds the row's length (INT64_MIN: no list), so that appends, compaction
    and EXISTS keep working on it as they are.  The pool is modelled by its two counters alone."""

    def __init__(self, dim: int, space: str) -> None:
        super().__init__(dim, space)
        self._lists = {}
        self._pool_used = {}

    def define_attr(self, attr, kind):
        if kind != "int64_list":
            return super().define_attr(attr, kind)
        super().define_attr(attr, "int64")
        self._lists[attr] = [None] * self._rows.shape[0]
        self._pool_used[attr] = 0

    def append(self, rows):
        first = super().append(rows)
        for a, rows_ in self._lists.items():
            rows_.extend([None] * (self._rows.shape[0] - len(rows_)))
        return first

    def compact(self):
        old = super().compact()
        for a in self._lists:
            self._lists[a] = [self._lists[a][i] for i in old.tolist()]
            self._pool_used[a] = self.list_stats(a)[1]  # the repack: what the live rows hold, nothing else
        return old

    def _put(self, attr, row, value):
        self._lists[attr][row] = value
        self._cols[attr][row] = W.INT64_ABSENT if value is None else len(value)

    def _refuse_list(self, attr, what):
        if attr in self._lists:
            raise RuntimeError(f"{what} failed (1): a list column")

    def set_attr(self, attr, first, values):
        self._refuse_list(attr, "attr_set")
        return super().set_attr(attr, first, values)

    def get_attr(self, attr, first, n, dtype=np.int64):
        self._refuse_list(attr, "attr_get")
        return super().get_attr(attr, first, n, dtype)

    def set_attr_at(self, attr, labels, values):
        self._refuse_list(attr, "attr_set_at")
        return super().set_attr_at(attr, labels, values)

    def update_where(self, program, assigns):
        for attr, _, _ in assigns:
            self._refuse_list(attr, "attr_update_where")
        return super().update_where(program, assigns)

    def set_attr_list(self, attr, first, col):
        rows = uncsr(col)
        assert first + len(rows) <= self._rows.shape[0]
        for i, r in enumerate(rows):
            self._put(attr, first + i, r)
        self._pool_used[attr] += int(col.values.size)

    def set_attr_list_at(self, attr, labels, col):
        labels = np.asarray(labels, dtype=np.int64).ravel()
        rows = uncsr(col)
        assert len(rows) == labels.size
        if labels.size and (labels.min() < 0 or labels.max() >= self._rows.shape[0] or np.unique(labels).size != labels.size):
            raise RuntimeError("attr_list_set_at failed (1): bad labels")
        wrote = 0
        for lab, r in zip(labels.tolist(), rows):
            if not self._deleted[lab]:
                self._put(attr, lab, r)
                wrote += 1
        self._pool_used[attr] += int(col.values.size)
        return wrote

    def get_attr_list(self, attr, first, n):
        return csr(self._lists[attr][first:first + n])

    def update_where_list(self, program, attr, values):
        hit = self.match(program)  # the lists from before the call
        new = None if values is None else frozenset(int(v) for v in np.asarray(values).ravel().tolist())
        for row in np.flatnonzero(hit).tolist():
            self._put(attr, row, new)
        self._pool_used[attr] += 0 if new is None else len(new)
        return int(hit.sum())

    def list_stats(self, attr):
        live = sum(len(r) for r, dead in zip(self._lists[attr], self._deleted.tolist()) if r is not None and not dead)
        return self._pool_used[attr], live

    def reset_lists(self):
        """What ``mlvdb_index_reset`` leaves of the lists: nothing but the definitions."""
        for a in self._lists:
            self._lists[a] = []
            self._pool_used[a] = 0

    def facet_list_values(self, attr, max_values, where=None):
        mask = self._mask(where)
        counts = Counter()
        absent = 0
        for row in np.flatnonzero(mask).tolist():
            r = self._lists[attr][row]
            counts.update(r or ())
            absent += not r
        if len(counts) > max_values:
            raise FacetOverflow(max_values, len(counts), int(mask.sum()), absent)
        values = sorted(counts)
        return (np.array(values, dtype=np.int64), np.array([counts[v] for v in values], dtype=np.int64), int(mask.sum()),
                absent)

    def match(self, program):
        n = self._rows.shape[0]
        return eval_list_program(program, self._cols, self._lists, n) & ~self._deleted


# ---------------------------------------------------------------- the meaning of a dict filter over list attributes
def _size_ok(n, lit):
    if not isinstance(lit, dict):
        return n == lit
    return all({"$eq": n == x, "$lt": n < x, "$lte": n <= x, "$gt": n > x, "$gte": n >= x}[op] for op, x in lit.items())


def _list_field(op, v, lit):
    """``v``: the row's value as a set, or ``None``."""
    present = v is not None
    if op == "$eq":
        return present and lit in v
    if op == "$ne":
        return not (present and lit in v)
    if op == "$in":
        return present and any(x in v for x in lit)
    if op == "$nin":
        return not (present and any(x in v for x in lit))
    if op == "$all":
        return present and all(x in v for x in lit)
    if op == "$size":
        return present and _size_ok(len(v), lit)
    assert op == "$exists"
    return present == bool(lit)


def py_match(where, meta, schema=TAG_SCHEMA) -> bool:
    """``where_helpers.py_match`` with list attributes: a row's value is the set of its elements (``[]``: the empty set,
    present), ``None`` / a missing key: no value."""
    for key, val in where.items():
        if key == "$and":
            ok = all(py_match(w, meta, schema) for w in val)
        elif key == "$or":
            ok = any(py_match(w, meta, schema) for w in val)
        elif key == "$not":
            ok = not py_match(val, meta, schema)
        else:
            kind = schema[key]
            v = None if meta is None else meta.get(key)
            if kind.endswith("[]"):
                v = None if v is None else set(v)
                ok = all(_list_field(op, v, lit) for op, lit in val.items()) if isinstance(val, dict) else \
                    _list_field("$eq", v, val)
            else:
                if kind == "float" and isinstance(v, float) and v != v:
                    v = None
                ok = all(_field(kind, op, v, lit) for op, lit in val.items()) if isinstance(val, dict) else \
                    _field(kind, "$eq", v, val)
        if not ok:
            return False
    return True


# ---------------------------------------------------------------- random metadata and dict filters
def random_tag_metadata(rng, n):
    out = []
    for _ in range(n):
        m = {}
        r = rng.random()
        if r < 0.75:
            m["tags"] = [TAGS[i] for i in rng.choice(len(TAGS), int(rng.integers(1, 6)), replace=True)]  # duplicates happen
        elif r < 0.85:
            m["tags"] = []
        elif r < 0.9:
            m["tags"] = None
        r = rng.random()
        if r < 0.6:
            m["nums"] = tuple(int(x) for x in rng.integers(0, 12, int(rng.integers(0, 5))))
        if rng.random() < 0.8:
            m["year"] = int(rng.integers(1950, 1970))
        if rng.random() < 0.7:
            m["price"] = float(np.round(rng.uniform(0, 100), 1))
        out.append(m)
    return out


def _tag(rng):
    return (TAGS + ["zydeco"])[rng.integers(len(TAGS) + 1)]  # sometimes a tag never ingested


def random_tag_leaf(rng):
    r = rng.random()
    if r < 0.15:
        return {"year": {"$gte": int(rng.integers(1950, 1970))}}
    if r < 0.25:
        return {"price": {"$lt": float(rng.integers(0, 100))}}
    key = "tags" if rng.random() < 0.7 else "nums"
    lit = (lambda: _tag(rng)) if key == "tags" else (lambda: int(rng.integers(0, 14)))
    op = ["$eq", "bare", "$ne", "$in", "$nin", "$all", "$size", "$size2", "$exists"][rng.integers(9)]
    if op == "bare":
        return {key: lit()}
    if op in ("$eq", "$ne"):
        return {key: {op: lit()}}
    if op in ("$in", "$nin"):
        return {key: {op: [lit() for _ in range(rng.integers(0, 4))]}}
    if op == "$all":
        return {key: {"$all": [lit() for _ in range(rng.integers(1, 4))]}}
    if op == "$size":
        return {key: {"$size": int(rng.integers(0, 5))}}
    if op == "$size2":
        return {key: {"$size": {"$gte": int(rng.integers(0, 3)), "$lt": int(rng.integers(1, 6))}}}
    return {key: {"$exists": bool(rng.random() < 0.5)}}


def random_tag_filter(rng, depth=0):
    r = rng.random()
    if depth >= 2 or r < 0.45:
        return random_tag_leaf(rng)
    if r < 0.6:
        return {"$not": random_tag_filter(rng, depth + 1)}
    comb = "$and" if r < 0.8 else "$or"
    return {comb: [random_tag_filter(rng, depth + 1) for _ in range(rng.integers(1, 4))]}


# ---------------------------------------------------------------- raw programs over a list, an int64 and a float64 column
def random_list_program(rng, list_attr, int_attr, float_attr, elements, n_ops=None):
    """A valid postfix program of list ops over column ``list_attr`` mixed with EQ..GE / EXISTS over an int64 and a float64
    column under AND / OR / NOT, with its own set table.  ``elements``: the values the lists are drawn from (set ranges
    and HAS literals are drawn from them and from values next to them, so that they hit and miss)."""
    elements = np.asarray(elements, dtype=np.int64)
    pool = np.unique(np.concatenate([elements, elements[elements < INT64_MAX] + 1, [0, 1, 2]]))
    table, ops, depth = [], [], 0
    n_ops = int(n_ops or rng.integers(1, 12))
    for i in range(n_ops):
        left = n_ops - i
        opts = [o for o, ok in (("push", depth <= left - 1), ("comb", depth >= 2), ("not", depth >= 1 and depth - 1 <= left - 1))
                if ok]
        choice = opts[rng.integers(len(opts))]
        if choice == "comb":
            ops.append((W.AND if rng.random() < 0.5 else W.OR, 0, 0, 0))
            depth -= 1
            continue
        if choice == "not":
            ops.append((W.NOT, 0, 0, 0))
            continue
        depth += 1
        r = rng.random()
        if r < 0.2:
            ops.append((W.HAS, list_attr, int(rng.choice(pool)), 0))
        elif r < 0.55:
            all_ = r < 0.35
            size = int(rng.integers(1 if all_ else 0, 4))
            vals = np.unique(rng.choice(elements if all_ else pool, size)) if size else np.zeros(0, np.int64)
            ops.append((W.HAS_ALL if all_ else W.HAS_ANY, list_attr, len(table), int(vals.size)))
            table.extend(vals.tolist())
        elif r < 0.7:
            lo = int(rng.integers(-1, 5))
            ops.append((W.LEN, list_attr, lo, lo + int(rng.integers(-1, 300))))
        elif r < 0.75:
            ops.append((W.EXISTS, list_attr, 0, 0))
        elif r < 0.9:
            ops.append(((W.EQ, W.NE, W.LT, W.GE)[rng.integers(4)], int_attr, int(rng.integers(-2, 6)), 0))
        else:
            lit = np.array([rng.uniform(-1, 1)]).view(np.int64)[0]
            ops.append(((W.LT, W.GE, W.EXISTS)[rng.integers(3)], float_attr, int(lit), 0))
    assert depth == 1
    return W.Program(np.array(ops, dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))
