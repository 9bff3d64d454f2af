"""Scan engines: what an ``Index`` namespace delegates its arithmetic to.

``HipScanEngine`` is the product backend -- a ctypes handle onto one ``mlvdb_index`` in
HBM (include/mlvdb_hip.h).  It takes the role hnswlib.Index plays in the reference
(src/mlvectordb/implementations/index.py:36-38,65,80,111).  There is deliberately no
CPU engine in this package: tests inject the oracle's engine through ``Index(engine_factory=...)``.
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Sequence
from typing import List, Protocol, Tuple

import numpy as np

from . import _native


class ScanEngine(Protocol):
    """One namespace's corpus: dense labels 0..total-1 in insertion order."""

    dim: int
    space: str

    def append(self, rows: np.ndarray) -> int: ...

    def tombstone(self, labels: np.ndarray) -> int: ...

    def counts(self) -> Tuple[int, int]: ...

    def compact(self) -> np.ndarray: ...

    def get_rows(self, first: int, n: int) -> np.ndarray: ...

    def get_rows_at(self, labels: np.ndarray) -> np.ndarray: ...

    def pair_distances(self, queries: np.ndarray, labels: np.ndarray) -> Tuple[np.ndarray, np.ndarray]: ...

    def search(self, queries: np.ndarray, k: int, mask: np.ndarray | None = None
               ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]: ...

    def range(self, queries: np.ndarray, radius: float, capacity: int, truncate: bool = False
              ) -> List[Tuple[np.ndarray, np.ndarray]]: ...

    def close(self) -> None: ...


class RangeHits(Sequence):
    """The answer of a range call: ``hits[i]`` is ``(labels int64[n_i], distances float32[n_i])`` of query i, nearest first --
    views of the packed arrays ``labels`` / ``dist`` between ``offsets[i]`` and ``offsets[i + 1]`` (what the C ABI's packed
    entry returns; nothing is copied per query)."""

    __slots__ = ("labels", "dist", "offsets", "_off")

    def __init__(self, labels: np.ndarray, dist: np.ndarray, offsets: np.ndarray) -> None:
        self.labels, self.dist, self.offsets = labels, dist, offsets
        self._off = offsets.tolist()

    def __len__(self) -> int:
        return len(self._off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("query index out of range")
        a, b = self._off[i], self._off[i + 1]
        return self.labels[a:b], self.dist[a:b]


def stitch_range_hits(parts, nq: int) -> RangeHits:
    """The packed answers of several calls, each over a subset of a batch's queries -- ``parts`` = [(query indices,
    labels, dist, offsets), ...], every query of the batch in exactly one part -- as one ``RangeHits`` in query order."""
    if len(parts) == 1 and np.array_equal(parts[0][0], np.arange(nq)):
        return RangeHits(*parts[0][1:])
    lens = np.zeros(nq, dtype=np.int64)
    for idx, _, _, off in parts:
        lens[idx] = np.diff(off)
    offsets = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    labels = np.empty(int(offsets[-1]), dtype=np.int64)
    dist = np.empty(int(offsets[-1]), dtype=np.float32)
    for idx, lab, dst, off in parts:
        for j, i in enumerate(idx.tolist()):
            a, b = int(off[j]), int(off[j + 1])
            labels[offsets[i]:offsets[i] + b - a] = lab[a:b]
            dist[offsets[i]:offsets[i] + b - a] = dst[a:b]
    return RangeHits(labels, dist, offsets)


class FacetOverflow(RuntimeError):
    """A value-facet call met more than ``max_values`` distinct values (``MLVDB_ERR_OVERFLOW``).  ``matched`` and ``absent``
    are still exact; ``n_values`` is some number above ``max_values``."""

    def __init__(self, max_values: int, n_values: int, matched: int, absent: int) -> None:
        super().__init__(f"facet_values: more than max_values={max_values} distinct values")
        self.max_values, self.n_values, self.matched, self.absent = max_values, n_values, matched, absent


class StatsOverflow(RuntimeError):
    """An ``attr_stats`` call met more than ``max_groups`` distinct values of ``by`` (``MLVDB_ERR_OVERFLOW``).  ``matched`` and
    ``by_absent`` are still exact; ``n_groups`` is some number above ``max_groups``."""

    def __init__(self, max_groups: int, n_groups: int, matched: int, by_absent: int) -> None:
        super().__init__(f"attr_stats: more than max_groups={max_groups} distinct values of by")
        self.max_groups, self.n_groups, self.matched, self.by_absent = max_groups, n_groups, matched, by_absent


class JoinOverflow(RuntimeError):
    """A self-join met a row with more than ``max_per_row`` partners, so its pair list is truncated and does not determine
    the connected components (``duplicate_groups``).  ``most`` is the largest exact partner count."""

    def __init__(self, max_per_row: int, most: int) -> None:
        super().__init__(f"duplicate_groups: a row has {most} partners within the radius, more than max_per_row={max_per_row}")
        self.max_per_row, self.most = max_per_row, most


class MaxSimOverflow(RuntimeError):
    """A late-interaction call met more than ``max_groups`` documents among the rows it counts (``MLVDB_ERR_OVERFLOW``)."""

    def __init__(self, max_groups: int) -> None:
        super().__init__(f"search_maxsim: more than max_groups={max_groups} documents")
        self.max_groups = max_groups


def _opt(a):
    """The data pointer of an optional array: ``None`` stays ``None`` (NULL: the entry skips that output or input)."""
    return None if a is None else a.ctypes.data


def _nonempty(a):
    """The data pointer of an array that may be empty: NULL then (NumPy's pointer of an empty array points nowhere)."""
    return a.ctypes.data if a.size else None


class HipScanEngine:
    """Exhaustive fp32 corpus scan on one MI355X, through the C ABI."""

    def __init__(self, dim: int, space: str, device: int = 0, capacity_hint: int = 0,
                 strategy: str = "auto") -> None:
        if space not in _native.SPACE_CODES:
            # hnswlib raises RuntimeError("Space name must be one of l2, ip, or cosine.")
            raise RuntimeError(f"space must be one of l2, ip, cosine (got {space!r})")
        self._lib = _native.load()
        self.dim = int(dim)
        self.space = space
        self.device = int(device)
        handle = C.c_void_p()
        rc = self._lib.mlvdb_index_create(self.device, self.dim, _native.SPACE_CODES[space],
                                          int(capacity_hint), C.byref(handle))
        if rc != _native.OK:
            msg = self._lib.mlvdb_last_global_error().decode(errors="replace")
            raise RuntimeError(f"mlvdb_index_create failed ({rc}): {msg}")
        self._h = handle
        self._attr_kinds = {}  # column -> "int64" / "float64", as defined through this object
        if strategy != "auto":
            self.set_strategy(strategy)

    # -- helpers -------------------------------------------------------------------
    def _check(self, rc: int, what: str, allow=()) -> int:
        if rc != _native.OK and rc not in allow:
            msg = self._lib.mlvdb_last_error(self._h).decode(errors="replace")
            raise RuntimeError(f"{what} failed ({rc}): {msg}")
        return rc

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def _queries(self, queries) -> np.ndarray:
        """``queries`` as the contiguous float32 [nq, dim] array the entries read (itself when it already is one)."""
        queries = np.ascontiguousarray(queries, dtype=np.float32)
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise RuntimeError(f"Wrong dimensionality of the vectors: got {queries.shape}, index dim {self.dim}")
        return queries

    @staticmethod
    def _knn_outputs(shape, want64: bool):
        """The outputs of a kNN-shaped entry: labels int64 and distances float32 of ``shape`` = (nq, k, ...), counts int32
        [nq] (zeros), float64 distances of ``shape`` with ``want64`` (else ``None``)."""
        return (np.empty(shape, dtype=np.int64), np.empty(shape, dtype=np.float32), np.zeros(shape[0], dtype=np.int32),
                np.empty(shape, dtype=np.float64) if want64 else None)

    @staticmethod
    def _tally():
        """The ``n, matched, absent`` out-parameters of the aggregating entries."""
        return C.c_int64(0), C.c_int64(0), C.c_int64(0)

    @staticmethod
    def _first(n, arrays, *totals) -> tuple:
        """What an aggregating entry returns: the first ``n`` of each output buffer (copies: the buffers are sized for the
        most the call may return), then the totals as ints."""
        return tuple(a[: n.value].copy() for a in arrays) + tuple(int(t.value) for t in totals)

    def set_strategy(self, strategy: str) -> None:
        self._check(self._lib.mlvdb_index_set_strategy(self._h, _native.STRATEGY_CODES[strategy]), "set_strategy")

    def set_tuning(self, **knobs: int) -> None:
        """Tuning state of the handle (``mlvdb_index_set_tuning``): ``set_tuning(SCAN_NQT=16, I8=0)``.  The MLVDB_* environment
        variables are only read when the handle is created; this is how a live handle is switched (tools/scan_ab.py)."""
        for key, value in knobs.items():
            self._check(self._lib.mlvdb_index_set_tuning(self._h, f"{key}={int(value)}".encode()), f"set_tuning({key})")

    def get_tuning(self, key: str) -> int:
        out = C.c_int32(0)
        self._check(self._lib.mlvdb_index_get_tuning(self._h, key.encode(), C.byref(out)), f"get_tuning({key})")
        return int(out.value)

    def set_profiling(self, enabled: bool) -> None:
        self._check(self._lib.mlvdb_index_set_profiling(self._h, int(bool(enabled))), "set_profiling")

    def last_stats(self) -> dict:
        st = _native.Stats()
        self._check(self._lib.mlvdb_index_last_stats(self._h, C.byref(st)), "last_stats")
        return {name: getattr(st, name) for name, _ in _native.Stats._fields_}

    # -- ScanEngine ----------------------------------------------------------------
    def append(self, rows: np.ndarray) -> int:
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise RuntimeError(f"Wrong dimensionality of the vectors: got {rows.shape}, index dim {self.dim}")
        first = C.c_int64(-1)
        self._check(self._lib.mlvdb_index_append(self._h, rows.ctypes.data, rows.shape[0], C.byref(first)), "append")
        return int(first.value)

    def append_device(self, device_ptr: int, n: int) -> int:
        first = C.c_int64(-1)
        self._check(self._lib.mlvdb_index_append_device(self._h, C.c_void_p(device_ptr), int(n), C.byref(first)),
                    "append_device")
        return int(first.value)

    def tombstone(self, labels: np.ndarray) -> int:
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        changed = C.c_int64(0)
        self._check(self._lib.mlvdb_index_tombstone(self._h, labels.ctypes.data, labels.size, C.byref(changed)),
                    "tombstone")
        return int(changed.value)

    def counts(self) -> Tuple[int, int]:
        total, deleted = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.mlvdb_index_counts(self._h, C.byref(total), C.byref(deleted)), "counts")
        return int(total.value), int(deleted.value)

    def compact(self) -> np.ndarray:
        """Drop the tombstoned rows on the device; returns old_labels with old_labels[new] = old."""
        total, deleted = self.counts()
        old = np.empty(max(total - deleted, 1), dtype=np.int64)
        live = C.c_int64(0)
        self._check(self._lib.mlvdb_index_compact(self._h, old.ctypes.data_as(C.c_void_p), old.size, C.byref(live)),
                    "mlvdb_index_compact")
        return old[: live.value]

    def reset(self, space: str | None = None) -> None:
        code = -1 if space is None else _native.SPACE_CODES[space]
        self._check(self._lib.mlvdb_index_reset(self._h, code), "reset")
        if space is not None:
            self.space = space

    def get_rows(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dim), dtype=np.float32)
        self._check(self._lib.mlvdb_index_get_rows(self._h, int(first), int(n), out.ctypes.data), "get_rows")
        return out

    def get_rows_at(self, labels: np.ndarray) -> np.ndarray:
        labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        out = np.empty((labels.size, self.dim), dtype=np.float32)
        self._check(self._lib.mlvdb_index_get_rows_at(self._h, labels.ctypes.data, labels.size, out.ctypes.data),
                    "get_rows_at")
        return out

    def pair_distances(self, queries: np.ndarray, labels: np.ndarray):
        """Exact distances of the pairs (queries[q], row labels[q, j]) in this index's space, by the kernels' own fp64
        summation (``mlvdb_pair_distances``): (float64 [nq, m], float32 [nq, m]); label -1 gives +inf."""
        queries = self._queries(queries)
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        if labels.ndim != 2 or labels.shape[0] != queries.shape[0]:
            raise RuntimeError(f"labels must be [nq, m]; got {labels.shape} for {queries.shape[0]} queries")
        d64 = np.empty(labels.shape, dtype=np.float64)
        d32 = np.empty(labels.shape, dtype=np.float32)
        self._check(self._lib.mlvdb_pair_distances(self._h, queries.ctypes.data, queries.shape[0], labels.ctypes.data,
                                                   labels.shape[1], d64.ctypes.data, d32.ctypes.data), "pair_distances")
        return d64, d32

    # -- metadata filters (include/mlvdb_where.h) ------------------------------------
    def define_attr(self, attr: int, kind: str) -> None:
        """Column ``attr`` (0..15) of type "int64" (absent = INT64_MIN), "float64" (absent = NaN), "int64_list" (a set of
        int64 per row, include/mlvdb_list.h), "sparse" (a sparse vector per row, include/mlvdb_sparse.h), "bits" (a bit code
        per row, include/mlvdb_bits.h) or "geo" (a packed
        location per row, stored as int64 with INT64_MIN absent, include/mlvdb_geo.h), every row absent."""
        code = _native.LIST_ATTR_CODES[kind] if kind in _native.LIST_ATTR_CODES else _native.ATTR_CODES[kind]
        self._check(self._lib.mlvdb_attr_define(self._h, int(attr), code), "attr_define")
        self._attr_kinds[int(attr)] = kind

    def set_attr(self, attr: int, first: int, values: np.ndarray) -> None:
        """Values of rows first..first+len(values)-1 (int64 or float64 by the column's type)."""
        values = np.ascontiguousarray(values)
        if values.dtype not in (np.int64, np.float64):
            raise RuntimeError(f"attribute values must be int64 or float64, got {values.dtype}")
        self._check(self._lib.mlvdb_attr_set(self._h, int(attr), int(first), values.size, values.ctypes.data), "attr_set")

    def get_attr(self, attr: int, first: int, n: int, dtype=np.int64) -> np.ndarray:
        out = np.empty(int(n), dtype=dtype)
        self._check(self._lib.mlvdb_attr_get(self._h, int(attr), int(first), int(n), out.ctypes.data), "attr_get")
        return out

    @staticmethod
    def _where(program):
        """(mlvdb_where, the arrays it points into: kept alive by the caller for the call)."""
        ops = np.ascontiguousarray(program.ops)
        table = np.ascontiguousarray(program.set, dtype=np.int64)
        w = _native.Where(ops.ctypes.data, int(ops.size), _nonempty(table), int(table.size))
        return w, (ops, table)

    @classmethod
    def _where_arg(cls, program):
        """An optional compiled filter as (the ``const mlvdb_where*`` argument: ``None`` without one, what the caller keeps
        alive for the call)."""
        if program is None:
            return None, None
        w, keep = cls._where(program)
        return C.byref(w), (w, keep)

    def where_count(self, program) -> int:
        """Live rows the compiled filter (``where.Program``) matches, counted on the device."""
        w, keep = self._where(program)
        n = C.c_int64(0)
        self._check(self._lib.mlvdb_where_count(self._h, C.byref(w), C.byref(n)), "where_count")
        return int(n.value)

    def where_labels(self, program) -> np.ndarray:
        """Ascending labels of the live rows the compiled filter matches."""
        w, keep = self._where(program)
        total, deleted = self.counts()
        out = np.empty(max(total - deleted, 1), dtype=np.int64)
        n = C.c_int64(0)
        self._check(self._lib.mlvdb_where_labels(self._h, C.byref(w), out.ctypes.data, out.size, C.byref(n)), "where_labels")
        return out[: n.value]

    # -- attribute updates and filtered deletes (include/mlvdb_mutate.h) ----------------
    def set_attr_at(self, attr: int, labels: np.ndarray, values: np.ndarray) -> int:
        """``values[j]`` -> row ``labels[j]`` of column ``attr`` (distinct labels in [0, total); tombstoned rows are
        skipped); returns the rows written.  The sentinels clear a value, as in ``set_attr``."""
        labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        values = np.ascontiguousarray(values).ravel()
        if values.dtype not in (np.int64, np.float64):
            raise RuntimeError(f"attribute values must be int64 or float64, got {values.dtype}")
        if values.size != labels.size:
            raise RuntimeError(f"{labels.size} labels but {values.size} values")
        n = C.c_int64(0)
        self._check(self._lib.mlvdb_attr_set_at(self._h, int(attr), labels.ctypes.data, labels.size, values.ctypes.data,
                                                C.byref(n)), "attr_set_at")
        return int(n.value)

    def update_where(self, program, assigns) -> Tuple[int, int]:
        """Apply ``assigns`` -- (attr, op, a) triples, op ``_native.SET_ASSIGN`` / ``SET_ADD``, ``a`` the int64 the column
        takes (float64 column: the bits of the double) -- to every live row the compiled filter matches, all or nothing:
        (matched, refused), and nothing changed when ``refused`` (rows whose sum cannot be stored) is not 0."""
        w, keep = self._where(program)
        sets = np.array([(int(attr), int(op), int(a)) for attr, op, a in assigns], dtype=_native.ASSIGN_DTYPE)
        matched, refused = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.mlvdb_attr_update_where(self._h, C.byref(w), sets.ctypes.data, int(sets.size),
                                                      C.byref(matched), C.byref(refused)), "attr_update_where")
        return int(matched.value), int(refused.value)

    def tombstone_where(self, program) -> np.ndarray:
        """Tombstone every live row the compiled filter matches; their labels, ascending."""
        w, keep = self._where(program)
        total, deleted = self.counts()
        out = np.empty(max(total - deleted, 1), dtype=np.int64)
        n = C.c_int64(0)
        self._check(self._lib.mlvdb_tombstone_where(self._h, C.byref(w), out.ctypes.data, out.size, C.byref(n)),
                    "tombstone_where")
        if n.value > out.size:  # (cannot happen: the buffer holds every live row)
            raise RuntimeError(f"tombstone_where: {n.value} matches for {out.size} live rows")
        return out[: n.value]

    # -- list columns (include/mlvdb_list.h) -------------------------------------------
    @staticmethod
    def _csr(col):
        """A ``where.ListColumn`` as the contiguous arrays the C entries take (kept alive by the caller for the call)."""
        offsets = np.ascontiguousarray(col.offsets, dtype=np.int64)
        values = np.ascontiguousarray(col.values, dtype=np.int64)
        present = np.ascontiguousarray(col.present, dtype=np.uint8)
        if offsets.size != present.size + 1:
            raise RuntimeError(f"{present.size} rows but {offsets.size} offsets")
        return offsets, values, present

    def set_attr_list(self, attr: int, first: int, col) -> None:
        """The lists of rows first..first+len(col)-1 of list column ``attr`` (``col``: a ``where.ListColumn``)."""
        offsets, values, present = self._csr(col)
        self._check(self._lib.mlvdb_attr_list_set(self._h, int(attr), int(first), present.size, offsets.ctypes.data,
                                                  _nonempty(values), present.ctypes.data), "attr_list_set")

    def set_attr_list_at(self, attr: int, labels: np.ndarray, col) -> int:
        """List i of ``col`` -> row ``labels[i]`` (distinct labels in [0, total); tombstoned rows are skipped); returns the
        rows written."""
        labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        offsets, values, present = self._csr(col)
        if present.size != labels.size:
            raise RuntimeError(f"{labels.size} labels but {present.size} lists")
        n = C.c_int64(0)
        self._check(self._lib.mlvdb_attr_list_set_at(self._h, int(attr), labels.ctypes.data, labels.size, offsets.ctypes.data,
                                                     _nonempty(values), present.ctypes.data, C.byref(n)), "attr_list_set_at")
        return int(n.value)

    def get_attr_list(self, attr: int, first: int, n: int):
        """The lists of rows first..first+n-1 as a ``where.ListColumn`` (tombstoned rows keep what they hold)."""
        from .where import ListColumn

        n = int(n)
        offsets = np.zeros(n + 1, dtype=np.int64)
        present = np.zeros(n, dtype=np.uint8)
        values = np.empty(0, dtype=np.int64)
        needed = C.c_int64(0)
        for _ in range(2):  # the first call sizes the values, the second reads them
            self._check(self._lib.mlvdb_attr_list_get(self._h, int(attr), int(first), n, offsets.ctypes.data, _nonempty(values),
                                                      present.ctypes.data, values.size, C.byref(needed)), "attr_list_get")
            if needed.value <= values.size:
                break
            values = np.empty(needed.value, dtype=np.int64)
        return ListColumn(offsets, values[: needed.value], present)

    def update_where_list(self, program, attr: int, values) -> int:
        """Every live row the compiled filter matches gets the list ``values`` (sorted unique int64), or loses its list
        (``None``); returns the matched count."""
        w, keep = self._where(program)
        arr = np.zeros(0, dtype=np.int64) if values is None else np.ascontiguousarray(values, dtype=np.int64).ravel()
        matched = C.c_int64(0)
        self._check(self._lib.mlvdb_attr_list_update_where(self._h, C.byref(w), int(attr), _nonempty(arr), int(arr.size),
                                                           1 if values is None else 0, C.byref(matched)),
                    "attr_list_update_where")
        return int(matched.value)

    def list_stats(self, attr: int) -> Tuple[int, int]:
        """(values allocated in the attribute's pool, summed list lengths of the live rows): equal right after ``compact``."""
        used, live = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.mlvdb_attr_list_stats(self._h, int(attr), C.byref(used), C.byref(live)), "attr_list_stats")
        return int(used.value), int(live.value)

    def facet_list_values(self, attr: int, max_values: int, where=None):
        """``facet_values`` of a list column: counts[v] = live matching rows whose list holds values[v]; ``absent`` = the
        matching rows with no list or an empty one (a row counts under each of its values, so the counts do not sum to
        ``matched - absent``)."""
        return self._facet("facet_list_values", attr, max_values, where)

    # -- sparse vector columns (include/mlvdb_sparse.h) ----------------------------------
    @staticmethod
    def _sparse_csr(col):
        """A ``where.SparseColumn`` as the contiguous arrays the C entries take (kept alive by the caller for the call)."""
        offsets, terms, weights = HipScanEngine._sparse_arrays(col)
        present = np.ascontiguousarray(col.present, dtype=np.uint8)
        if offsets.size != present.size + 1 or terms.size != weights.size:
            raise RuntimeError(f"{present.size} rows but {offsets.size} offsets, {terms.size} terms and {weights.size} weights")
        return offsets, terms, weights, present

    @staticmethod
    def _sparse_arrays(col):
        """``_sparse_csr`` without ``present`` and without its size check: the form of a batch of sparse queries, whose
        entries check the sizes against their own query count."""
        return (np.ascontiguousarray(col.offsets, dtype=np.int64), np.ascontiguousarray(col.terms, dtype=np.int32),
                np.ascontiguousarray(col.weights, dtype=np.float32))

    def set_attr_sparse(self, attr: int, first: int, col) -> None:
        """The vectors of rows first..first+len(col)-1 of sparse column ``attr`` (``col``: a ``where.SparseColumn``)."""
        offsets, terms, weights, present = self._sparse_csr(col)
        self._check(self._lib.mlvdb_sparse_set(self._h, int(attr), int(first), present.size, offsets.ctypes.data,
                                               _nonempty(terms), _nonempty(weights), present.ctypes.data), "sparse_set")

    def set_attr_sparse_at(self, attr: int, labels: np.ndarray, col) -> int:
        """Vector i of ``col`` -> row ``labels[i]`` (distinct labels in [0, total); tombstoned rows are skipped); returns the
        rows written."""
        labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        offsets, terms, weights, present = self._sparse_csr(col)
        if present.size != labels.size:
            raise RuntimeError(f"{labels.size} labels but {present.size} vectors")
        n = C.c_int64(0)
        self._check(self._lib.mlvdb_sparse_set_at(self._h, int(attr), labels.ctypes.data, labels.size, offsets.ctypes.data,
                                                  _nonempty(terms), _nonempty(weights), present.ctypes.data, C.byref(n)),
                    "sparse_set_at")
        return int(n.value)

    def get_attr_sparse(self, attr: int, first: int, n: int):
        """The vectors of rows first..first+n-1 as a ``where.SparseColumn`` (tombstoned rows keep what they hold)."""
        from .where import SparseColumn

        n = int(n)
        offsets = np.zeros(n + 1, dtype=np.int64)
        present = np.zeros(n, dtype=np.uint8)
        terms = np.empty(0, dtype=np.int32)
        weights = np.empty(0, dtype=np.float32)
        needed = C.c_int64(0)
        for _ in range(2):  # the first call sizes the entries, the second reads them
            self._check(self._lib.mlvdb_sparse_get(self._h, int(attr), int(first), n, offsets.ctypes.data, _nonempty(terms),
                                                   _nonempty(weights), present.ctypes.data, terms.size, C.byref(needed)),
                        "sparse_get")
            if needed.value <= terms.size:
                break
            terms = np.empty(needed.value, dtype=np.int32)
            weights = np.empty(needed.value, dtype=np.float32)
        return SparseColumn(offsets, terms[: needed.value], weights[: needed.value], present)

    def search_batch_sparse(self, attr: int, queries, k: int, where=None):
        """Exact lexical kNN (``mlvdb_search_batch_sparse``): ``queries`` is a ``where.SparseColumn`` (its ``present`` is
        ignored: every query is one, an empty one ranks by label), ``where`` a compiled filter or ``None``.  Returns
        (labels int64 [nq, k] padded -1, scores float32 [nq, k] padded -inf, counts int32 [nq], scores float64 [nq, k]):
        the rows with a vector ranked by (inner product descending, label ascending)."""
        offsets, terms, weights = self._sparse_arrays(queries)
        nq, k = offsets.size - 1, int(k)
        if nq < 0 or terms.size != weights.size:
            raise RuntimeError(f"{offsets.size} offsets, {terms.size} terms and {weights.size} weights")
        labels, score, counts, score64 = self._knn_outputs((nq, max(k, 0)), True)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_sparse(
            self._h, int(attr), offsets.ctypes.data, _nonempty(terms), _nonempty(weights), nq, k, w, labels.ctypes.data,
            score.ctypes.data, counts.ctypes.data, score64.ctypes.data), "search_batch_sparse")
        return labels, score, counts, score64

    # -- binary vector columns (include/mlvdb_bits.h) -------------------------------------
    @staticmethod
    def _bits_codes(col):
        """A ``where.BitsColumn`` as the contiguous arrays the C entries take (kept alive by the caller for the call)."""
        words = np.ascontiguousarray(col.words, dtype=np.uint64)
        present = np.ascontiguousarray(col.present, dtype=np.uint8)
        if words.ndim != 2 or words.shape[0] != present.size:
            raise RuntimeError(f"{present.size} rows but codes of shape {words.shape}")
        return words, present

    def bits_set(self, attr: int, first: int, col) -> None:
        """The codes of rows first..first+len(col)-1 of bits column ``attr`` (``col``: a ``where.BitsColumn``)."""
        words, present = self._bits_codes(col)
        self._check(self._lib.mlvdb_bits_set(self._h, int(attr), int(first), present.size, words.shape[1], _nonempty(words),
                                             present.ctypes.data), "bits_set")

    def bits_set_at(self, attr: int, labels: np.ndarray, col) -> int:
        """Code i of ``col`` -> row ``labels[i]`` (distinct labels in [0, total); tombstoned rows are skipped); returns the
        rows written."""
        labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        words, present = self._bits_codes(col)
        if present.size != labels.size:
            raise RuntimeError(f"{labels.size} labels but {present.size} codes")
        n = C.c_int64(0)
        self._check(self._lib.mlvdb_bits_set_at(self._h, int(attr), labels.ctypes.data, labels.size, words.shape[1],
                                                _nonempty(words), present.ctypes.data, C.byref(n)), "bits_set_at")
        return int(n.value)

    def bits_get(self, attr: int, first: int, n: int):
        """The codes of rows first..first+n-1: (widths int32 [n] in words, 0 = absent; the present rows' words uint64, back to
        back in row order).  Tombstoned rows keep what they hold."""
        n = int(n)
        widths = np.zeros(n, dtype=np.int32)
        codes = np.empty(0, dtype=np.uint64)
        needed = C.c_int64(0)
        for _ in range(2):  # the first call sizes the codes, the second reads them
            self._check(self._lib.mlvdb_bits_get(self._h, int(attr), int(first), n, _nonempty(widths), _nonempty(codes),
                                                 codes.size, C.byref(needed)), "bits_get")
            if needed.value <= codes.size:
                break
            codes = np.empty(needed.value, dtype=np.uint64)
        return widths, codes[: needed.value]

    def search_bits(self, attr: int, queries: np.ndarray, k: int, metric: str = "hamming", where=None):
        """Exact kNN over bit codes (``mlvdb_search_batch_bits``): ``queries`` uint64 [nq, words], ``metric`` "hamming" or
        "jaccard", ``where`` a compiled filter or ``None``.  Returns (labels int64 [nq, k] padded -1, distances float32
        [nq, k] padded +inf, counts int32 [nq], distances float64 [nq, k]): the live rows with a code of ``words`` words
        ranked by (distance ascending, label ascending)."""
        queries = np.ascontiguousarray(queries, dtype=np.uint64)
        if queries.ndim != 2:
            raise RuntimeError(f"queries must be [nq, words]; got shape {queries.shape}")
        if metric not in _native.BITS_METRIC_CODES:
            raise RuntimeError(f"unknown bits metric {metric!r} (one of {sorted(_native.BITS_METRIC_CODES)})")
        nq, k = queries.shape[0], int(k)
        labels, dist, counts, dist64 = self._knn_outputs((nq, max(k, 0)), True)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_bits(
            self._h, int(attr), _nonempty(queries), nq, queries.shape[1], _native.BITS_METRIC_CODES[metric], k, w,
            labels.ctypes.data, dist.ctypes.data, counts.ctypes.data, dist64.ctypes.data), "search_batch_bits")
        return labels, dist, counts, dist64

    # -- hybrid search (include/mlvdb_hybrid.h) -------------------------------------------
    def search_hybrid(self, queries: np.ndarray, attr: int, sparse_queries, k: int, fetch_dense: int, fetch_sparse: int,
                      method: str = "rrf", weights=(1.0, 1.0), rrf_k: float = 60.0, where=None, components: bool = False):
        """Dense and sparse kNN fused on the device (``mlvdb_search_batch_hybrid``): ``queries`` [nq, dim], ``sparse_queries``
        a ``where.SparseColumn`` of ``nq`` vectors over sparse column ``attr`` (an empty one gets the sparse search's
        label-ordered zero-score list: a caller without a sparse query wants ``search``), ``method`` one of "rrf", "linear",
        "relative", ``weights`` = (w_dense, w_sparse), ``where`` a compiled filter or ``None`` (it restricts both legs).
        Returns (labels int64 [nq, k] padded -1, fused float64 [nq, k] padded -inf, counts int32 [nq]) and, with
        ``components``, (dist64, sparse64, rank_dense, rank_sparse) behind them: each hit's completed components and its
        position in the two candidate lists (-1: not in that list)."""
        queries = self._queries(queries)
        if method not in _native.FUSE_CODES:
            raise RuntimeError(f"unknown fusion method {method!r} (one of {sorted(_native.FUSE_CODES)})")
        offsets, terms, wts = self._sparse_arrays(sparse_queries)
        nq, k = queries.shape[0], int(k)
        if offsets.size != nq + 1 or terms.size != wts.size:
            raise RuntimeError(f"{nq} dense queries but {offsets.size} offsets, {terms.size} terms and {wts.size} weights")
        shape = (nq, max(k, 0))
        labels = np.empty(shape, dtype=np.int64)
        fused = np.empty(shape, dtype=np.float64)
        counts = np.zeros(nq, dtype=np.int32)
        d64 = np.empty(shape, dtype=np.float64) if components else None
        s64 = np.empty(shape, dtype=np.float64) if components else None
        rd = np.empty(shape, dtype=np.int32) if components else None
        rs = np.empty(shape, dtype=np.int32) if components else None
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_hybrid(
            self._h, queries.ctypes.data, int(attr), offsets.ctypes.data, _nonempty(terms), _nonempty(wts), nq, k,
            int(fetch_dense), int(fetch_sparse), _native.FUSE_CODES[method], float(weights[0]), float(weights[1]),
            float(rrf_k), w, labels.ctypes.data, fused.ctypes.data, counts.ctypes.data, _opt(d64), _opt(s64), _opt(rd),
            _opt(rs)), "search_batch_hybrid")
        return (labels, fused, counts, d64, s64, rd, rs) if components else (labels, fused, counts)

    # -- per-query filters (include/mlvdb_where_each.h) -------------------------------
    @staticmethod
    def _where_array(programs):
        """(mlvdb_where[len(programs)], the arrays they point into: kept alive by the caller for the call)."""
        arr = (_native.Where * max(len(programs), 1))()
        keep = []
        for j, prog in enumerate(programs):
            w, k = HipScanEngine._where(prog)
            arr[j] = w
            keep.append(k)
        return arr, keep

    def count_each(self, programs) -> np.ndarray:
        """Live rows each compiled filter of ``programs`` matches (int64 array), all counted in one pass per native call."""
        from .where import chunk_programs

        out = np.zeros(len(programs), dtype=np.int64)
        start = 0
        for _, chunk, _ in chunk_programs(list(programs), np.zeros(0, np.int32)):
            arr, keep = self._where_array(chunk)
            part = np.zeros(max(len(chunk), 1), dtype=np.int64)
            self._check(self._lib.mlvdb_where_count_each(self._h, arr, len(chunk), part.ctypes.data), "where_count_each")
            out[start:start + len(chunk)] = part[:len(chunk)]
            start += len(chunk)
        return out

    def search_each(self, queries: np.ndarray, k: int, programs, program_of_query, want64: bool = False,
                    return_routes: bool = False):
        """kNN with a filter per query: query i searches the rows ``programs[program_of_query[i]]`` matches (-1: all
        rows).  Returns what ``search`` (``want64=False``) or ``search64`` returns, each query's row bit-identical to a call
        for it alone; ``return_routes=True`` appends an int32 array with each program's route (``_native.ROUTE_*``).
        One native call per chunk of at most 64 programs / 1024 ops (``where.chunk_programs``)."""
        from .where import chunk_programs

        queries = self._queries(queries)
        of = np.ascontiguousarray(program_of_query, dtype=np.int32)
        nq = queries.shape[0]
        if of.shape != (nq,):
            raise RuntimeError(f"program_of_query: {of.shape}, expected ({nq},)")
        labels, dist, counts, d64 = self._knn_outputs((nq, k), want64)
        routes = np.zeros(len(programs), dtype=np.int32)
        start = 0
        for idx, chunk, local in chunk_programs(list(programs), of):
            n = idx.size
            q = np.ascontiguousarray(queries[idx])
            lab, dst, cnt, l64 = self._knn_outputs((n, k), want64)
            rts = np.zeros(max(len(chunk), 1), dtype=np.int32)
            arr, keep = self._where_array(chunk)
            self._check(self._lib.mlvdb_search_batch_where_each(
                self._h, q.ctypes.data, n, int(k), arr, len(chunk), local.ctypes.data, lab.ctypes.data, dst.ctypes.data,
                cnt.ctypes.data, _opt(l64), rts.ctypes.data), "search_batch_where_each")
            labels[idx], dist[idx], counts[idx] = lab, dst, cnt
            if want64:
                d64[idx] = l64
            routes[start:start + len(chunk)] = rts[:len(chunk)]
            start += len(chunk)
        out = (labels, dist, counts, d64) if want64 else (labels, dist, counts)
        return out + (routes,) if return_routes else out

    # -- distinct-by-attribute kNN (include/mlvdb_distinct.h) ---------------------------
    def search_distinct(self, queries: np.ndarray, k: int, attr: int, max_groups: int = 0, where=None,
                        want64: bool = False):
        """The nearest row of each of the ``k`` nearest groups, a group being one present value of int64 column ``attr``
        (rows with an absent value are in no group).  ``max_groups``: an upper bound on the number of distinct present
        values (0 = unknown), which only lets a query stop early; ``where`` (optional, a compiled ``where.Program``)
        restricts the rows first.  Returns (labels int64 [nq, k], dist float32, counts int32, groups int64 [nq, k]) or,
        with ``want64``, (labels, dist, counts, dist64, groups); padding is label -1 / +inf / group INT64_MIN."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        labels, dist, counts, d64 = self._knn_outputs((nq, k), want64)
        groups = np.empty((nq, k), dtype=np.int64)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_distinct(
            self._h, queries.ctypes.data, nq, int(k), int(attr), int(max_groups), w, labels.ctypes.data, dist.ctypes.data,
            counts.ctypes.data, _opt(d64), groups.ctypes.data), "search_batch_distinct")
        return (labels, dist, counts, d64, groups) if want64 else (labels, dist, counts, groups)

    # -- scored kNN (include/mlvdb_score.h) -----------------------------------------------
    def search_scored(self, queries: np.ndarray, k: int, program, where=None, want64: bool = False):
        """The ``k`` (<= 64) rows with the smallest score per query, the score being the compiled ``score.ScoreProgram``
        evaluated on the device for every live row -- of those the optional compiled ``where.Program`` matches -- in fp64:
        the exact top k by (score, label), rows whose score is NaN dropped.  Returns (labels int64 [nq, k], scores float64
        [nq, k], counts int32) or, with ``want64``, (labels, scores, counts, dist64: the rows' fp64 distances); padding is
        label -1 / +inf, and ``counts`` tells it from a real +inf score."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        labels, _, counts, d64 = self._knn_outputs((nq, k), want64)
        scores = np.empty((nq, k), dtype=np.float64)
        ops = np.ascontiguousarray(program.ops)
        conds, keep_conds = self._where_array(program.conds)
        sc = _native.Score(ops.ctypes.data, int(ops.size), conds, len(program.conds))
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_scored(
            self._h, queries.ctypes.data, nq, int(k), C.byref(sc), w, labels.ctypes.data, scores.ctypes.data,
            counts.ctypes.data, _opt(d64)), "search_batch_scored")
        return (labels, scores, counts, d64) if want64 else (labels, scores, counts)

    # -- grouped kNN (include/mlvdb_grouped.h) --------------------------------------------
    def search_grouped(self, queries: np.ndarray, k: int, group_size: int, attr: int, max_groups: int = 0, where=None,
                       want64: bool = False):
        """The ``group_size`` (<= 64) nearest rows of each of the ``k`` nearest groups of int64 column ``attr``: the groups
        and their ranking are those of ``search_distinct`` with the same arguments, slot ``[i, j, 0]`` is its ``[i, j]``.
        Returns (labels int64 [nq, k, group_size], dist float32, counts int32 [nq]: groups returned, group_counts int32
        [nq, k]: rows returned per group, groups int64 [nq, k]) or, with ``want64``, (labels, dist, counts, group_counts,
        dist64, groups); padding is label -1 / +inf / group count 0 / group INT64_MIN."""
        queries = self._queries(queries)
        nq, k, g = queries.shape[0], int(k), int(group_size)
        shape = (nq, max(k, 0), max(g, 0))
        labels, dist, counts, d64 = self._knn_outputs(shape, want64)
        group_counts = np.empty(shape[:2], dtype=np.int32)
        groups = np.empty(shape[:2], dtype=np.int64)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_grouped(
            self._h, queries.ctypes.data, nq, k, g, int(attr), int(max_groups), w, labels.ctypes.data, dist.ctypes.data,
            counts.ctypes.data, group_counts.ctypes.data, _opt(d64), groups.ctypes.data), "search_batch_grouped")
        return ((labels, dist, counts, group_counts, d64, groups) if want64
                else (labels, dist, counts, group_counts, groups))

    # -- diversified kNN (include/mlvdb_mmr.h) --------------------------------------------
    def search_mmr(self, queries: np.ndarray, k: int, fetch_k: int, lam: float, where=None, want64: bool = False):
        """Greedy maximal-marginal-relevance selection of ``k`` (<= 64) hits among the ``fetch_k`` (<= 1024) nearest rows
        of each query -- those the optional compiled ``where.Program`` matches -- on the device: the first pick is the
        nearest row, each further pick minimises ``lam * d(query, i) - (1 - lam) * min over the picks s of d(s, i)``, ties
        to the better-ranked candidate.  Returns (labels int64 [nq, k], dist float32, counts int32, dist64 float64 or
        ``None`` without ``want64``, rank int32 [nq, k]: the pick's position among the candidates, objective float64
        [nq, k]), all in pick order; padding is label -1 / +inf / rank -1 / objective +inf."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        labels, dist, counts, d64 = self._knn_outputs((nq, k), want64)
        rank = np.empty((nq, k), dtype=np.int32)
        objective = np.empty((nq, k), dtype=np.float64)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_mmr(
            self._h, queries.ctypes.data, nq, int(k), int(fetch_k), float(lam), w, labels.ctypes.data, dist.ctypes.data,
            counts.ctypes.data, _opt(d64), rank.ctypes.data, objective.ctypes.data), "search_batch_mmr")
        return labels, dist, counts, d64, rank, objective

    # -- search by stored examples (include/mlvdb_like.h) -----------------------------------
    def search_like(self, labels: np.ndarray, weights: np.ndarray, offsets: np.ndarray, k: int, *, base=None,
                    exclude: bool = True, where=None, want64: bool = False, want_queries: bool = False):
        """kNN with queries built on the device from stored rows: query ``i`` is ``base[i]`` (when given) plus
        ``weights[j]`` times the stored row ``labels[j]`` -- the unit vector of that row on a cosine index -- over
        ``j = offsets[i] .. offsets[i + 1] - 1`` (<= 64 per query), summed in fp64 and rounded to fp32 once.  With ``exclude``
        the examples of a query are taken out of its hits on the device (the inner search fetches ``k`` + the most distinct
        examples of a query, <= 1024); ``where`` (a compiled ``where.Program``) restricts the rows searched, not the
        examples.  Returns (labels int64 [nq, k], dist float32, counts int32, dist64 float64 or ``None`` without
        ``want64``, queries float32 [nq, dim] or ``None`` without ``want_queries``); padding is label -1 / +inf."""
        ex_labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        ex_weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        ex_offsets = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
        if ex_offsets.size < 1 or ex_labels.size != ex_weights.size:
            raise RuntimeError(f"search_like: {ex_labels.size} labels, {ex_weights.size} weights, {ex_offsets.size} offsets")
        nq = ex_offsets.size - 1
        if nq > 0 and ex_offsets[-1] > ex_labels.size:
            raise RuntimeError(f"search_like: the offsets end at {int(ex_offsets[-1])}, there are {ex_labels.size} examples")
        if base is not None:
            base = np.ascontiguousarray(base, dtype=np.float32)
            if base.shape != (nq, self.dim):
                raise RuntimeError(f"Wrong dimensionality of the vectors: got {base.shape}, index dim {self.dim}, {nq} queries")
        k = int(k)
        out_labels, dist, counts, d64 = self._knn_outputs((nq, max(k, 0)), want64)
        queries = np.empty((nq, self.dim), dtype=np.float32) if want_queries else None
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_like(
            self._h, ex_labels.ctypes.data, ex_weights.ctypes.data, ex_offsets.ctypes.data, _opt(base), nq, k,
            1 if exclude else 0, w, out_labels.ctypes.data, dist.ctypes.data, counts.ctypes.data, _opt(d64), _opt(queries)),
            "search_batch_like")
        return out_labels, dist, counts, d64, queries

    # -- similarity join (include/mlvdb_join.h) ---------------------------------------------
    def join_within(self, labels: np.ndarray, mode: int, radius: float, capacity: int, where=None, truncate: bool = False):
        """The stored rows within ``radius`` of the stored rows ``labels`` (strictly ascending; tombstoned ones allowed), the
        queries gathered on the device: per left row what ``range(get_rows_at(labels), radius, ..., where=where)`` returns
        for it, bit for bit, without the row itself (``_native.JOIN_OTHERS``) or without every label <= its own
        (``_native.JOIN_LATER``: every unordered pair once).  Returns (``RangeHits``, exact counts int64 [n]); ``capacity``
        and ``truncate`` as in ``range``, the most per row being ``_native.JOIN_MAX_CAPACITY``.  The first call leaves room
        for 16 partners per row on average (near-duplicates are few); when the hits need more, the call is repeated with
        the sizes the first one reported."""
        left = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        n = int(left.size)
        w, keep = self._where_arg(where)

        def call(capacity, total, out_labels, dist, offsets, counts):
            return self._lib.mlvdb_join_within(self._h, _nonempty(left), n, int(mode), float(radius), capacity, total, w,
                                               out_labels.ctypes.data, dist.ctypes.data, offsets.ctypes.data,
                                               _nonempty(counts))

        out_labels, dist, offsets, counts = self._range_packed_counts(call, n, capacity, truncate, _native.JOIN_MAX_CAPACITY,
                                                                      16, "join_within")
        return RangeHits(out_labels, dist, offsets), counts

    # -- recommend / discover (include/mlvdb_examples.h) ------------------------------------
    def search_examples(self, mode: int, labels: np.ndarray, vectors, roles: np.ndarray, offsets: np.ndarray, k: int, *,
                        exclude: bool = True, where=None):
        """The ``k`` (<= 64) best rows per query against its bag of examples, each example judged on its own: query ``i``
        owns the examples ``offsets[i] .. offsets[i + 1] - 1`` (1..64); example ``j`` is the stored row ``labels[j]`` (read
        on the device) or, with ``labels[j] == -1``, row ``j`` of ``vectors`` (float32 ``[examples, dim]``, ``None`` without
        one); ``roles[j]`` is ``_native.EXAMPLE_POS / NEG / TARGET`` as ``mode`` (``_native.EXAMPLES_BEST / DISCOVER /
        CONTEXT``) allows.  Rows are ranked by (tier, value, label) as the header defines them; with ``exclude`` a query's
        stored examples never come back; ``where`` (a compiled ``where.Program``) restricts the rows, not the examples.
        Returns (labels int64 [nq, k] padded -1, tiers int32 padded INT32_MAX, values float64 padded +inf, counts int32)."""
        ex_labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        ex_roles = np.ascontiguousarray(roles, dtype=np.int32).ravel()
        ex_offsets = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
        if ex_offsets.size < 1 or ex_labels.size != ex_roles.size:
            raise RuntimeError(f"search_examples: {ex_labels.size} labels, {ex_roles.size} roles, {ex_offsets.size} offsets")
        nq = ex_offsets.size - 1
        if nq > 0 and ex_offsets[-1] > ex_labels.size:
            raise RuntimeError(f"search_examples: the offsets end at {int(ex_offsets[-1])}, there are {ex_labels.size} examples")
        if vectors is not None:
            vectors = np.ascontiguousarray(vectors, dtype=np.float32)
            if vectors.shape != (ex_labels.size, self.dim):
                raise RuntimeError(f"Wrong dimensionality of the vectors: got {vectors.shape}, index dim {self.dim}, "
                                   f"{ex_labels.size} examples")
        k = int(k)
        shape = (nq, max(k, 0))
        out_labels = np.empty(shape, dtype=np.int64)
        tiers = np.empty(shape, dtype=np.int32)
        values = np.empty(shape, dtype=np.float64)
        counts = np.zeros(nq, dtype=np.int32)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_search_batch_examples(
            self._h, int(mode), _nonempty(ex_labels), _opt(vectors), _nonempty(ex_roles), ex_offsets.ctypes.data, nq, k,
            1 if exclude else 0, w, out_labels.ctypes.data, tiers.ctypes.data, values.ctypes.data, counts.ctypes.data),
            "search_batch_examples")
        return out_labels, tiers, values, counts

    # -- clustering (include/mlvdb_cluster.h) ------------------------------------------------
    def _centroids(self, labels, vectors, what: str):
        """The centroid arguments of the two entries: (labels int64 [m] or ``None``, vectors float32 [m, dim] or ``None``,
        m).  Centroid ``j`` is the stored row ``labels[j]`` or, with ``labels[j] == -1`` (or no labels at all), row ``j`` of
        ``vectors``."""
        if labels is None and vectors is None:
            raise RuntimeError(f"{what}: neither centroid labels nor centroid vectors")
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.int64).ravel()
        if vectors is not None:
            vectors = np.ascontiguousarray(vectors, dtype=np.float32)
            if vectors.ndim != 2 or vectors.shape[1] != self.dim or (labels is not None and vectors.shape[0] != labels.size):
                raise RuntimeError(f"Wrong dimensionality of the vectors: got {vectors.shape}, index dim {self.dim}"
                                   + ("" if labels is None else f", {labels.size} centroids"))
        return labels, vectors, int(labels.size if labels is not None else vectors.shape[0])

    def assign_nearest(self, labels, vectors=None, *, where=None, assign_attr: int = -1):
        """Every candidate row (live, matching ``where``) to its nearest centroid: the lowest ``j`` with the smallest
        ``pair_distances`` value, bit for bit; a row every distance of which is NaN or +inf stays unassigned.  With
        ``assign_attr`` >= 0 that int64 column receives ``j`` (absent for an unassigned row); no other row is touched, and
        the filter is evaluated before anything is written.  Returns (sizes int64 [m], costs float64 [m] -- the members'
        best distances in the header's blocked order --, candidates)."""
        labels, vectors, m = self._centroids(labels, vectors, "assign_nearest")
        sizes = np.zeros(max(m, 1), dtype=np.int64)
        costs = np.zeros(max(m, 1), dtype=np.float64)
        matched = C.c_int64(0)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_assign_nearest(self._h, _opt(labels), _opt(vectors), m, w, int(assign_attr),
                                                   sizes.ctypes.data, costs.ctypes.data, C.byref(matched)), "assign_nearest")
        return sizes[:m], costs[:m], int(matched.value)

    def kmeans(self, labels, vectors=None, *, max_iterations: int = 25, where=None, assign_attr: int = -1):
        """Lloyd's algorithm over the candidate rows from the given centroids (l2 and cosine): per iteration the assignment
        of ``assign_nearest`` and, per cluster, the mean of its members in the order ``include/mlvdb_cluster.h`` states
        (cosine: of the normalised members); a cluster without members keeps its centroid.  Stops after the first iteration
        >= 2 that moves no row, or at ``max_iterations``.  Returns (centroids float32 [m, dim], sizes int64 [m], costs
        float64 [m], iterations, converged, candidates); ``assign_attr`` holds the last assignment."""
        labels, vectors, m = self._centroids(labels, vectors, "kmeans")
        centroids = np.zeros((max(m, 1), self.dim), dtype=np.float32)
        sizes = np.zeros(max(m, 1), dtype=np.int64)
        costs = np.zeros(max(m, 1), dtype=np.float64)
        iterations, converged, matched = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_kmeans(self._h, _opt(labels), _opt(vectors), m, int(max_iterations), w, int(assign_attr),
                                           centroids.ctypes.data, sizes.ctypes.data, costs.ctypes.data, C.byref(iterations),
                                           C.byref(converged), C.byref(matched)), "kmeans")
        return centroids[:m], sizes[:m], costs[:m], int(iterations.value), bool(converged.value), int(matched.value)

    # -- late-interaction search (include/mlvdb_maxsim.h) -----------------------------------
    def search_maxsim(self, tokens: np.ndarray, offsets: np.ndarray, k: int, attr: int, where=None,
                      want_matches: bool = False):
        """Documents (the present values of int64 column ``attr``) ranked by the summed distance of each query token to the
        document's best row: query ``i`` is the token rows ``tokens[offsets[i]:offsets[i + 1]]`` (1..128 of them), a
        document's score the fp64 sum over them, in order, of the smallest distance to a live row of the document (one the
        compiled ``where.Program`` matches, when given); ascending by (score, group code), ``k`` <= 64.  Returns (groups
        int64 [nq, k], score float32, counts int32, score64 float64, match_labels int64 [total tokens, k] or ``None``,
        match_dist64 float64 [total tokens, k] or ``None``): row ``(offsets[i] + t, j)`` of the last two is the best row of
        query ``i``'s ``j``-th document for its token ``t`` and that pair's distance.  Padding is group INT64_MIN / +inf /
        label -1.  More than 2**20 documents raise ``MaxSimOverflow``."""
        tokens = self._queries(tokens)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
        if offsets.size < 1 or (offsets.size > 1 and offsets[-1] > tokens.shape[0]):
            raise RuntimeError(f"search_maxsim: {offsets.size} offsets ending at {int(offsets[-1]) if offsets.size else 0}, "
                               f"{tokens.shape[0]} tokens")
        nq, k = offsets.size - 1, int(k)
        ntok = int(offsets[-1]) if nq > 0 else 0
        groups, score, counts, score64 = self._knn_outputs((nq, max(k, 0)), True)
        match_labels = np.empty((ntok, max(k, 0)), dtype=np.int64) if want_matches else None
        match_d64 = np.empty((ntok, max(k, 0)), dtype=np.float64) if want_matches else None
        w, keep = self._where_arg(where)
        rc = self._check(self._lib.mlvdb_search_batch_maxsim(
            self._h, tokens.ctypes.data, offsets.ctypes.data, nq, k, int(attr), w, groups.ctypes.data, score.ctypes.data,
            counts.ctypes.data, score64.ctypes.data, _opt(match_labels), _opt(match_d64)), "search_batch_maxsim",
            allow=(_native.ERR_OVERFLOW,))
        if rc == _native.ERR_OVERFLOW:
            raise MaxSimOverflow(_native.MAXSIM_MAX_GROUPS)
        return groups, score, counts, score64, match_labels, match_d64

    # -- facet counts and histograms (include/mlvdb_facet.h) ---------------------------
    def facet_values(self, attr: int, max_values: int, where=None):
        """The distinct present values of int64 column ``attr`` among the live rows (those the compiled ``where.Program``
        matches, when one is given) and how many rows hold each: (values int64 ascending, counts int64, matched, absent)
        with ``counts.sum() + absent == matched``.  More than ``max_values`` distinct values raise ``FacetOverflow``."""
        return self._facet("facet_values", attr, max_values, where)

    def _facet(self, entry: str, attr: int, max_values: int, where):
        """``mlvdb_facet_values`` or ``mlvdb_facet_list_values``: the two take and return the same."""
        max_values = int(max_values)
        values = np.empty(max(0, min(max_values, _native.FACET_MAX_VALUES)), dtype=np.int64)
        counts = np.empty(values.size, dtype=np.int64)
        n, matched, absent = self._tally()
        w, keep = self._where_arg(where)
        rc = self._check(getattr(self._lib, "mlvdb_" + entry)(
            self._h, int(attr), w, max_values, values.ctypes.data, counts.ctypes.data, C.byref(n), C.byref(matched),
            C.byref(absent)), entry, allow=(_native.ERR_OVERFLOW,))
        if rc == _native.ERR_OVERFLOW:
            raise FacetOverflow(max_values, int(n.value), int(matched.value), int(absent.value))
        return self._first(n, (values, counts), matched, absent)

    def facet_bins(self, attr: int, edges: np.ndarray, where=None):
        """Histogram of column ``attr`` over the strictly ascending ``edges`` (an int64 array for an int64 column, float64
        for a float64 one): (counts int64 [len(edges) + 1], matched, absent), ``counts[i]`` = the live matching rows whose
        present value has ``i`` edges at or below it (``np.searchsorted(edges, v, side="right")``)."""
        edges = np.ascontiguousarray(edges)
        if edges.ndim != 1 or edges.dtype not in (np.int64, np.float64):
            raise RuntimeError(f"edges must be a 1-d int64 or float64 array, got {edges.dtype} {edges.shape}")
        kind = self._attr_kinds.get(int(attr))
        if kind is not None and kind != edges.dtype.name:
            raise RuntimeError(f"attribute {attr} is an {kind} column, the edges are {edges.dtype.name}")
        counts = np.zeros(edges.size + 1, dtype=np.int64)
        matched, absent = C.c_int64(0), C.c_int64(0)
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_facet_bins(self._h, int(attr), w, edges.ctypes.data, int(edges.size), counts.ctypes.data,
                                               C.byref(matched), C.byref(absent)), "facet_bins")
        return counts, int(matched.value), int(absent.value)

    # -- attribute statistics (include/mlvdb_stats.h) ------------------------------------
    def attr_stats(self, attr: int, by: Optional[int] = None, max_groups: int = 1, where=None):
        """Rows, count, min, max and sum of scalar column ``attr`` among the live rows (those the compiled ``where.Program``
        matches, when one is given), per distinct present value of int64 column ``by`` or, with ``by=None``, as one group
        under key 0: (keys int64 ascending, rows int64, count int64, min, max -- int64 or float64 by the column's type,
        unspecified where count is 0 --, sum_hi int64, sum_lo uint64, matched, by_absent) with ``rows.sum() + by_absent ==
        matched``.  ``sum_hi:sum_lo`` is a signed 128-bit integer: the exact sum of an int64 column, the fixed-point sum
        of a float64 one (``stats.int128`` / ``stats.float_sum``).  More than ``max_groups`` groups raise ``StatsOverflow``."""
        max_groups = int(max_groups)
        size = max(1, min(max_groups, _native.FACET_MAX_VALUES))
        kind = self._attr_kinds.get(int(attr), "int64")
        keys, rows, count, hi = (np.zeros(size, dtype=np.int64) for _ in range(4))
        lo = np.zeros(size, dtype=np.uint64)
        mn, mx = (np.zeros(size, dtype=np.float64 if kind == "float64" else np.int64) for _ in range(2))
        n, matched, absent = self._tally()
        w, keep = self._where_arg(where)
        rc = self._check(self._lib.mlvdb_attr_stats(
            self._h, int(attr), -1 if by is None else int(by), w, max_groups, keys.ctypes.data, rows.ctypes.data,
            count.ctypes.data, mn.ctypes.data, mx.ctypes.data, hi.ctypes.data, lo.ctypes.data, C.byref(n), C.byref(matched),
            C.byref(absent)), "attr_stats", allow=(_native.ERR_OVERFLOW,))
        if rc == _native.ERR_OVERFLOW:
            raise StatsOverflow(max_groups, int(n.value), int(matched.value), int(absent.value))
        return self._first(n, (keys, rows, count, mn, mx, hi, lo), matched, absent)

    # -- ordered metadata queries (include/mlvdb_order.h) -------------------------------
    def where_ordered(self, attr: int, limit: int, where=None, descending: bool = False, offset: int = 0):
        """Ranks ``[offset, offset + limit)`` of the live rows (those the compiled ``where.Program`` matches, when one is
        given) that hold a value of column ``attr``, by that value -- ascending, or descending -- and rows of equal value by
        ascending label: (labels int64 [n_out], values int64 or float64 [n_out] by the column's type, matched, absent).
        ``offset + limit <= _native.ORDER_MAX_ROWS``; the ranking is done on the device, only the window comes back."""
        limit, offset = int(limit), int(offset)
        kind = self._attr_kinds.get(int(attr), "int64")
        size = max(0, min(limit, _native.ORDER_MAX_ROWS))
        labels = np.empty(size, dtype=np.int64)
        values = np.empty(size, dtype=np.float64 if kind == "float64" else np.int64)
        n, matched, absent = self._tally()
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_where_ordered(
            self._h, int(attr), 1 if descending else 0, w, offset, limit, labels.ctypes.data, values.ctypes.data, C.byref(n),
            C.byref(matched), C.byref(absent)), "where_ordered")
        return self._first(n, (labels, values), matched, absent)

    # -- nearest by distance on a geo column (include/mlvdb_geo.h) ----------------------
    def geo_nearest(self, attr: int, center: int, limit: int, where=None, offset: int = 0):
        """Ranks ``[offset, offset + limit)`` of the live rows (those the compiled ``where.Program`` matches, when one is
        given) that hold a point in geo column ``attr``, by great-circle distance from the packed point ``center`` and rows
        at equal distance by ascending label: (labels int64 [n_out], points int64 [n_out] as stored, metres float64 [n_out],
        matched, absent).  ``offset + limit <= _native.ORDER_MAX_ROWS``; a maximum distance is a ``$geo_radius`` in ``where``."""
        limit, offset = int(limit), int(offset)
        size = max(0, min(limit, _native.ORDER_MAX_ROWS))
        labels = np.empty(size, dtype=np.int64)
        points = np.empty(size, dtype=np.int64)
        dist = np.empty(size, dtype=np.float64)
        n, matched, absent = self._tally()
        w, keep = self._where_arg(where)
        self._check(self._lib.mlvdb_geo_nearest(
            self._h, int(attr), int(center), w, offset, limit, labels.ctypes.data, points.ctypes.data, dist.ctypes.data,
            C.byref(n), C.byref(matched), C.byref(absent)), "geo_nearest")
        return self._first(n, (labels, points, dist), matched, absent)

    def search64(self, queries: np.ndarray, k: int, mask: np.ndarray | None = None, where=None):
        """kNN; ``mask`` (optional, one byte per row, non-zero = allowed) restricts the search to those rows, ``where``
        (optional, a compiled ``where.Program``) to the rows it matches, evaluated on the device.
        Returns (labels int64, dist float32, counts int32, dist64 float64): the last is what a merge over several
        engines (row shards) has to rank on."""
        return self._search(queries, k, mask, True, where)

    def search(self, queries: np.ndarray, k: int, mask: np.ndarray | None = None, where=None):
        """kNN -> (labels int64 [nq, k], dist float32 [nq, k], counts int32 [nq]); ``mask`` / ``where`` as in ``search64``."""
        return self._search(queries, k, mask, False, where)

    def _search(self, queries: np.ndarray, k: int, mask, want64: bool, where=None):
        queries = self._queries(queries)
        nq = queries.shape[0]
        labels, dist, counts, d64 = self._knn_outputs((nq, k), want64)
        if where is not None:
            if mask is not None:
                raise RuntimeError("search: give a row mask or a where program, not both")
            w, keep = self._where(where)
            self._check(self._lib.mlvdb_search_batch_where(self._h, queries.ctypes.data, nq, int(k), C.byref(w),
                                                           labels.ctypes.data, dist.ctypes.data, counts.ctypes.data, _opt(d64)),
                        "search_batch_where")
            return (labels, dist, counts, d64) if want64 else (labels, dist, counts)
        if mask is not None:
            mask = np.ascontiguousarray(mask, dtype=np.uint8)
            if mask.shape != (self.counts()[0],):
                raise RuntimeError(f"row mask has shape {mask.shape}, the index holds {self.counts()[0]} rows")
        self._check(self._lib.mlvdb_search_batch_ex(self._h, queries.ctypes.data, nq, int(k), _opt(mask), labels.ctypes.data,
                                                    dist.ctypes.data, counts.ctypes.data, _opt(d64)), "search_batch")
        return (labels, dist, counts, d64) if want64 else (labels, dist, counts)

    def search_device(self, q_ptr: int, nq: int, k: int, labels_ptr: int, dist_ptr: int, counts_ptr: int,
                      dist64_ptr: int = 0, stream: int = 0) -> None:
        """Device-pointer search; results are complete when ``stream`` is.

        ``dist64_ptr`` (optional) receives the unrounded fp64 distances, which is what a
        multi-shard merge must rank on.
        """
        self._check(self._lib.mlvdb_search_batch_device(
            self._h, C.c_void_p(q_ptr), int(nq), int(k), C.c_void_p(labels_ptr), C.c_void_p(dist_ptr),
            C.c_void_p(counts_ptr), C.c_void_p(dist64_ptr or None), C.c_void_p(stream or None)), "search_batch_device")

    def range(self, queries: np.ndarray, radius: float, capacity: int, truncate: bool = False, where=None):
        """Per query (labels, fp32 distances) of the live rows within ``radius``, nearest first: a ``RangeHits`` sequence
        (``hits[i]`` -> the two arrays of query i, views of the call's packed outputs).

        ``truncate=False``: ``capacity`` is an initial size; the call is repeated once with the exact largest count,
        so every hit comes back (up to MLVDB_MAX_TOPK_PAGED = 16384 per query, the most one call can rank: beyond
        that the nearest 16384 are returned).  ``truncate=True``: at most ``capacity`` hits per query, the nearest.
        Through ``mlvdb_range_batch_packed``: hit counts differ by orders of magnitude between queries, the packed arrays
        hold the hits and nothing else (a first call with room for 256 hits per query on average; when the hits need
        more, the call is repeated with the size the first one reported).  ``where`` (optional, a compiled ``where.Program``)
        restricts the hits to the rows it matches (``mlvdb_range_batch_packed_where``)."""
        queries = self._queries(queries)
        nq = queries.shape[0]
        w, keep = self._where_arg(where)

        def call(capacity, total, labels, dist, offsets, counts):
            if w is None:
                return self._lib.mlvdb_range_batch_packed(self._h, queries.ctypes.data, nq, float(radius), capacity, total,
                                                          labels.ctypes.data, dist.ctypes.data, offsets.ctypes.data,
                                                          counts.ctypes.data)
            return self._lib.mlvdb_range_batch_packed_where(self._h, queries.ctypes.data, nq, float(radius), capacity, total,
                                                            w, labels.ctypes.data, dist.ctypes.data, offsets.ctypes.data,
                                                            counts.ctypes.data)

        return RangeHits(*self._range_packed(call, nq, capacity, truncate))

    def _range_packed(self, call, nq: int, capacity: int, truncate: bool):
        """The protocol of the packed range entries: a first guess of ``total_capacity`` (room for 256 hits per query on
        average) and one repeat with the sizes the first call reported.  ``call(capacity, total, labels, dist, offsets,
        counts)`` -> status.  Returns (labels, dist, offsets)."""
        return self._range_packed_counts(call, nq, capacity, truncate)[:3]

    def _range_packed_counts(self, call, nq: int, capacity: int, truncate: bool, cap_max: int = _native.MAX_TOPK_PAGED,
                             per_query: int = 256, what: str = "range_batch_packed"):
        """``_range_packed`` with the exact counts behind its answer: (labels, dist, offsets, counts).  ``cap_max``: the most
        hits per query the entry ranks; ``per_query``: the hits per query the first guess leaves room for on average."""
        capacity = max(1, min(int(capacity), cap_max))
        total = min(nq * capacity, max(65_536, per_query * nq))
        while True:
            labels = np.empty(total, dtype=np.int64)
            dist = np.empty(total, dtype=np.float32)
            offsets = np.zeros(nq + 1, dtype=np.int64)
            counts = np.zeros(nq, dtype=np.int64)
            rc = self._check(call(capacity, total, labels, dist, offsets, counts), what, allow=(_native.ERR_OVERFLOW,))
            if rc == _native.OK:
                break
            need_cap = capacity if truncate else min(max(int(counts.max(initial=0)), capacity), cap_max)
            need_total = int(np.minimum(counts, need_cap).sum())
            if need_cap == capacity and need_total <= total:
                break  # per-query truncation was asked for (or the engine's limit reached): the outputs hold the nearest
            capacity, total = need_cap, max(need_total, 1)
        return labels, dist, offsets, counts

    def range_each(self, queries: np.ndarray, radius: float, capacity: int, programs, program_of_query,
                   truncate: bool = False, return_routes: bool = False):
        """Range search with a filter per query: query i's hits are the rows ``programs[program_of_query[i]]`` matches (-1:
        all rows) within ``radius``.  Returns what ``range`` returns (``RangeHits``), each query's hits bit-identical to a
        ``range(..., where=program)`` call for it alone; ``return_routes=True`` -> (hits, int32 array with each program's
        route, ``_native.ROUTE_*``).  One native call per chunk of at most 64 programs / 1024 ops
        (``where.chunk_programs``), each with ``range``'s protocol for ``total_capacity``; the chunks' answers are
        stitched in query order."""
        from .where import chunk_programs

        queries = self._queries(queries)
        of = np.ascontiguousarray(program_of_query, dtype=np.int32)
        nq = queries.shape[0]
        if of.shape != (nq,):
            raise RuntimeError(f"program_of_query: {of.shape}, expected ({nq},)")
        routes = np.zeros(len(programs), dtype=np.int32)
        parts = []
        start = 0
        for idx, chunk, local in chunk_programs(list(programs), of):
            q = np.ascontiguousarray(queries[idx])
            rts = np.zeros(max(len(chunk), 1), dtype=np.int32)
            arr, keep = self._where_array(chunk)

            def call(capacity, total, labels, dist, offsets, counts):
                return self._lib.mlvdb_range_batch_packed_where_each(
                    self._h, q.ctypes.data, idx.size, float(radius), capacity, total, arr, len(chunk), local.ctypes.data,
                    labels.ctypes.data, dist.ctypes.data, offsets.ctypes.data, counts.ctypes.data, rts.ctypes.data)

            parts.append((idx,) + self._range_packed(call, idx.size, capacity, truncate))
            routes[start:start + len(chunk)] = rts[:len(chunk)]
            start += len(chunk)
        hits = stitch_range_hits(parts, nq)
        return (hits, routes) if return_routes else hits

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.mlvdb_index_destroy(self._h)
            self._h = None

    def __del__(self) -> None:  # best effort; HBM is released with the handle
        try:
            self.close()
        except Exception:
            pass
