"""Shared by the update / delete-by-filter tests: a NumPy model of the three engine entries of include/mlvdb_mutate.h, a
list-of-dicts model of an ``Index`` that is updated and deleted from by filter, and the seeded call histories both the
NumPy engine and the HIP engine are replayed against."""
from __future__ import annotations

import math

import numpy as np

from mlvectordb_amd import Vector, _native
from mlvectordb_amd import where as W
from oracle import exact_scan
from tests.facet_helpers import FacetOracleEngine
from tests.where_helpers import GENRES, SCHEMA, py_match, random_filter, random_metadata

INT64_MAX = 2 ** 63 - 1
INT64_MIN = -(2 ** 63)


def bits(col: np.ndarray) -> np.ndarray:
    """A column as the int64 words the device holds (NaN payloads and the sign of zero included)."""
    return np.ascontiguousarray(col).view(np.int64)


# ---------------------------------------------------------------- the engine entries, in NumPy
class MutateOracleEngine(FacetOracleEngine):
    """``WhereOracleEngine`` (+ facets) + ``set_attr_at`` / ``update_where`` / ``tombstone_where`` of ``HipScanEngine``."""

    def set_attr_at(self, attr, labels, values):
        labels = np.asarray(labels, dtype=np.int64).ravel()
        values = np.asarray(values).ravel()
        col = self._cols[attr]
        assert values.dtype == col.dtype and values.size == labels.size
        if labels.size and (labels.min() < 0 or labels.max() >= col.size or np.unique(labels).size != labels.size):
            raise RuntimeError("attr_set_at failed (1): bad labels")
        live = ~self._deleted[labels]
        col[labels[live]] = values[live]
        return int(live.sum())

    def update_where(self, program, assigns):
        """(matched, refused); all or nothing.  Sums in Python ints: no wrap-around hides an overflow."""
        hit = self.match(program)  # the values from before the call
        new, refused = {}, np.zeros(hit.size, bool)
        seen = set()
        for attr, op, a in assigns:
            assert attr not in seen and attr in self._cols
            seen.add(attr)
            col = self._cols[attr]
            if op == _native.SET_ASSIGN:
                out = col.copy()
                bits(out)[hit] = a
                new[attr] = out
                continue
            assert op == _native.SET_ADD
            out = col.copy()
            if col.dtype == np.int64:
                rows = np.flatnonzero(hit & (col != W.INT64_ABSENT))
                uniq, inv = np.unique(col[rows], return_inverse=True)
                sums = [int(u) + int(a) for u in uniq.tolist()]
                bad = np.array([not INT64_MIN < s <= INT64_MAX for s in sums], bool)
                stored = np.array([s if not b else 0 for s, b in zip(sums, bad)], dtype=np.int64)
                refused[rows[bad[inv]]] = True
                out[rows[~bad[inv]]] = stored[inv][~bad[inv]]
            else:
                add = np.array([a], dtype=np.int64).view(np.float64)[0]
                assert not math.isnan(add)
                rows = np.flatnonzero(hit & ~np.isnan(col))
                with np.errstate(all="ignore"):
                    sums = col[rows] + add
                bad = np.isnan(sums)
                refused[rows[bad]] = True
                out[rows[~bad]] = sums[~bad]
            new[attr] = out
        matched, n_refused = int(hit.sum()), int(refused.sum())
        if n_refused == 0:
            self._cols.update(new)
        return matched, n_refused

    def tombstone_where(self, program):
        labels = self.where_labels(program)
        assert self.tombstone(labels) == labels.size
        return labels


class UntouchableEngine(MutateOracleEngine):
    """Fails the test when a refused call reaches the engine."""

    armed = False

    def _touched(self, *a, **k):
        if type(self).armed:
            raise AssertionError("a refused call reached the engine")

    def set_attr_at(self, *a, **k):
        self._touched()
        return super().set_attr_at(*a, **k)

    def update_where(self, *a, **k):
        self._touched()
        return super().update_where(*a, **k)

    def tombstone_where(self, *a, **k):
        self._touched()
        return super().tombstone_where(*a, **k)

    def where_labels(self, *a, **k):
        self._touched()
        return super().where_labels(*a, **k)

    def tombstone(self, *a, **k):
        self._touched()
        return super().tombstone(*a, **k)

    def set_attr(self, *a, **k):
        self._touched()
        return super().set_attr(*a, **k)


# ---------------------------------------------------------------- an Index as a list of dicts
def _present(kind, v):
    return v is not None and not (kind == "float" and isinstance(v, float) and math.isnan(v))


class ModelIndex:
    """Rows in insertion order as dicts {"id", "values", "meta", "live"}; ``meta`` holds the declared attributes only.  Every
    filter is evaluated by ``py_match`` and every search by the exact scan over the surviving matching rows."""

    def __init__(self, space: str, schema=SCHEMA) -> None:
        self.space, self.schema, self.rows = space, schema, []

    def add(self, vectors):
        for v in vectors:
            meta = {k: x for k, x in (v.metadata or {}).items() if k in self.schema}
            self.rows.append({"id": v.id, "values": np.asarray(v.values, np.float32), "meta": meta, "live": True})

    def live(self):
        return [r for r in self.rows if r["live"]]

    def matching(self, where):
        return [r for r in self.live() if py_match(where, r["meta"], self.schema)]

    def update_attributes(self, ids, values):
        patches = [values] * len(ids) if isinstance(values, dict) else list(values)
        by_id = {r["id"]: r for r in self.live()}
        touched = set()
        for u, p in zip(ids, patches):
            r = by_id.get(u)
            if r is None or not p:
                continue
            r["meta"] = {**r["meta"], **p}
            touched.add(u)
        return len(touched)

    def update_where(self, where, values):
        """The matched count, or ValueError with nothing changed when an increment cannot be stored."""
        rows = self.matching(where)
        new = []
        for r in rows:
            meta = dict(r["meta"])
            for key, v in values.items():
                if not (isinstance(v, dict) and list(v) == ["$inc"]):
                    meta[key] = v
                    continue
                kind, old = self.schema[key], meta.get(key)
                if not _present(kind, old):
                    continue
                if kind == "int":
                    s = int(old) + int(v["$inc"])
                    if not INT64_MIN < s <= INT64_MAX:
                        raise ValueError("overflow")
                else:
                    s = float(np.float64(old) + np.float64(v["$inc"]))
                    if math.isnan(s):
                        raise ValueError("overflow")
                meta[key] = s
            new.append(meta)
        for r, meta in zip(rows, new):
            r["meta"] = meta
        return len(rows)

    def remove_where(self, where):
        rows = self.matching(where)
        for r in rows:
            r["live"] = False
        return [r["id"] for r in rows]

    def compact(self):
        self.rows = self.live()

    def facets(self, by, where):
        rows = self.matching(where)
        kind = self.schema[by]
        present = [r["meta"][by] for r in rows if _present(kind, r["meta"].get(by))]
        counts = {}
        for v in present:
            counts[v] = counts.get(v, 0) + 1
        return counts, len(rows), len(rows) - len(present)

    def search(self, queries, k, where):
        """Per query the (id, float32 distance) pairs of the k nearest surviving matching rows."""
        if not self.rows:
            return [[] for _ in range(len(queries))]
        keep = np.array([r["live"] and py_match(where, r["meta"], self.schema) for r in self.rows])
        mat = np.stack([r["values"] for r in self.rows])
        labels, dist, counts = exact_scan.knn(queries, mat, k, self.space, deleted=~keep)
        return [[(self.rows[l]["id"], d) for l, d in zip(labels[i, :counts[i]].tolist(), dist[i, :counts[i]].tolist())]
                for i in range(len(queries))]


# ---------------------------------------------------------------- seeded histories over random_metadata rows
def _random_value(rng, key):
    if rng.random() < 0.15:
        return None
    if key == "genre":
        return (GENRES + ["zydeco", "ska"])[rng.integers(len(GENRES) + 2)]  # sometimes a string the dictionary lacks
    if key == "year":
        return int(rng.integers(1940, 2030))
    if key == "price":
        return [float(np.round(rng.uniform(0, 100), 1)), int(rng.integers(0, 100)), float("nan")][rng.integers(3)]
    return bool(rng.random() < 0.5)


def random_patch(rng):
    keys = [k for k in SCHEMA if rng.random() < 0.4] or ["year"]
    return {k: _random_value(rng, k) for k in keys}


def random_assignments(rng):
    out = random_patch(rng)
    r = rng.random()
    if r < 0.3:
        out["year"] = {"$inc": int(rng.integers(-3, 4))}
    elif r < 0.5:
        out["price"] = {"$inc": [float(np.round(rng.uniform(-2, 2), 1)), int(rng.integers(-2, 3))][rng.integers(2)]}
    elif r < 0.65:
        out["year"] = {"$inc": int([INT64_MAX, -INT64_MAX][rng.integers(2)])}  # overflows on every row that holds a year
    return out


def replay_history(index, space: str, seed: int, n_rows: int, d: int, n_ops: int = 40, metric=None):
    """Draw ``n_ops`` operations from update_attributes / update_where / remove_where / add / compact and apply each to
    ``index`` (namespace "ns") and to a ``ModelIndex``; after every one, ``count``, ``query_by_metadata``, ``facets`` and
    ``search_many(where=)`` of the index must equal the model.  Returns how many operations of each kind ran."""
    rng = np.random.default_rng(seed)
    metric = metric or space
    model = ModelIndex(space)
    ran = {}

    def fresh(n):
        return [Vector(values=rng.standard_normal(d).astype(np.float32), metadata=m) for m in random_metadata(rng, n)]

    def add(n):
        vecs = fresh(n)
        index.add(vecs, "ns")
        model.add(vecs)

    def check(tag):
        qs = rng.standard_normal((3, d)).astype(np.float32)
        for j in range(3):
            f = random_filter(rng) if j else {}
            want = model.matching(f)
            assert index.count("ns", f) == len(want), (tag, f)
            assert index.query_by_metadata("ns", f) == [r["id"] for r in want], (tag, f)
            by = ["genre", "year", "in_stock"][rng.integers(3)]
            got = index.facets("ns", by, f)
            counts, matched, absent = model.facets(by, f)
            assert (dict(got["values"]), got["matched"], got["absent"]) == (counts, matched, absent), (tag, f, by)
            k = int(rng.choice([1, 5, 17]))
            hits = index.search_many(qs, k, "ns", metric, where=f)
            want_hits = model.search(qs, k, f)
            assert [[h.vector_id for h in row] for row in hits] == [[u for u, _ in row] for row in want_hits], (tag, f)
            if metric == "l2":  # the score is the distance itself
                got_d = [[h.score for h in row] for row in hits]
                assert np.allclose(sum(got_d, []), [x for row in want_hits for _, x in row], rtol=0, atol=1e-4), (tag, f)

    add(n_rows)
    check("start")
    for step in range(n_ops):
        kind = ["update_attributes", "update_where", "remove_where", "add", "compact"][
            rng.choice(5, p=[0.3, 0.3, 0.2, 0.12, 0.08])]
        ran[kind] = ran.get(kind, 0) + 1
        tag = (seed, step, kind)
        if kind == "update_attributes":
            pool = [r["id"] for r in model.rows]
            m = int(rng.integers(1, 12))
            ids = [pool[i] for i in rng.integers(0, len(pool), m)] if pool else []  # dead ids and repeats included
            ids += [Vector(values=[0.0]).id] if rng.random() < 0.3 else []  # an id nobody knows
            values = random_patch(rng) if rng.random() < 0.5 else [random_patch(rng) for _ in ids]
            assert index.update_attributes(ids, values, "ns") == model.update_attributes(ids, values), tag
        elif kind == "update_where":
            f, values = random_filter(rng), random_assignments(rng)
            try:
                want = model.update_where(f, values)
            except ValueError:
                before = index.count("ns", {})
                try:
                    index.update_where("ns", f, values)
                except ValueError as e:
                    assert "overflow" in str(e), tag
                else:
                    raise AssertionError(f"{tag}: an overflowing $inc was accepted")
                assert index.count("ns", {}) == before
                ran["refused"] = ran.get("refused", 0) + 1
            else:
                assert index.update_where("ns", f, values) == want, (tag, f, values)
        elif kind == "remove_where":
            f = random_filter(rng) if rng.random() < 0.8 else {"year": {"$lt": 1956}}
            if len(model.matching(f)) > 0.4 * max(1, len(model.live())):
                f = {"$and": [f, {"year": {"$lt": 1965}}]}  # keep rows to work on
            want = model.remove_where(f)
            if rng.random() < 0.5:
                assert index.remove_where("ns", f, return_ids=True) == want, (tag, f)
            else:
                assert index.remove_where("ns", f) == len(want), (tag, f)
        elif kind == "add":
            add(int(rng.integers(1, 30)))
        else:
            assert index.compact("ns")
            model.compact()
        check(tag)
    return ran
