"""Shared by the similarity-join tests (include/mlvdb_join.h): the rule restated in NumPy over the exact-scan oracle, the
preconditions every case asserts on the oracle alone, and an oracle engine with ``join_within``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from mlvectordb_amd import _native
from mlvectordb_amd.engine import RangeHits
from mlvectordb_amd.index import Index
from oracle import exact_scan
from tests.where_helpers import WhereOracleEngine

OTHERS, LATER = _native.JOIN_OTHERS, _native.JOIN_LATER


def strip(labels, dist, a: int, mode: int):
    """One ranked range answer by the rule: the entry ``a`` removed (OTHERS) or every entry with label <= ``a`` (LATER)."""
    keep = labels > a if mode == LATER else labels != a
    return labels[keep], dist[keep]


def join_model(rows, left, radius: float, space: str, mode: int, deleted=None, matching=None):
    """The NumPy model: ``range_query(rows[left], rows, radius, space)`` over the live rows ``matching`` admits (a boolean
    mask; None: all), stripped by the rule.  Returns (per left row (labels int64, dist float32), exact counts int64)."""
    rows = np.asarray(rows, dtype=np.float32)
    left = np.asarray(left, dtype=np.int64)
    hidden = np.zeros(rows.shape[0], dtype=bool) if deleted is None else np.asarray(deleted, dtype=bool).copy()
    if matching is not None:
        hidden |= ~np.asarray(matching, dtype=bool)
    if left.size == 0:
        return [], np.zeros(0, np.int64)
    hits = exact_scan.range_query(rows[left], rows, radius, space, deleted=hidden)
    out = [strip(l, d, int(a), mode) for (l, d), a in zip(hits, left)]
    return out, np.array([len(l) for l, _ in out], dtype=np.int64)


def cut(want, capacity: int):
    return [(l[:capacity], d[:capacity]) for l, d in want]


def offsets_of(want) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([len(l) for l, _ in want])]).astype(np.int64)


def assert_clear_of_radius(rows, left, radius: float, space: str, on_radius: bool = False):
    """Precondition, on the oracle alone: no distance of a left row lies within 1e-9 relative of the radius -- unless the
    case means rows to sit exactly on it (``on_radius``), which then must be there bit for bit."""
    r = float(np.float32(radius))
    d = exact_scan.exact_distances(np.asarray(rows, np.float32)[np.asarray(left, np.int64)], rows, space)
    near = np.abs(d - r) <= 1e-9 * max(abs(r), np.finfo(np.float64).tiny)
    exactly = d == r
    if on_radius:
        assert exactly.any(), "precondition: no oracle distance sits exactly on the radius"
    assert not (near & ~exactly).any() and (on_radius or not exactly.any()), \
        f"precondition: {int((near & ~exactly).sum())} oracle distances within 1e-9 relative of the radius {r!r}"


def assert_ties(rows, groups, space: str):
    """Precondition: the rows of each planted group of identical rows are bit-equal, so every distance to them ties."""
    rows = np.asarray(rows, np.float32)
    for g in groups:
        assert all(np.array_equal(rows[g[0]].view(np.uint32), rows[x].view(np.uint32)) for x in g), f"group {g[:3]}.. differs"
        d = exact_scan.exact_distances(rows[g[:1]], rows[list(g)], space)[0]
        assert (d == d[0]).all(), f"precondition: the distances to the identical rows {g[:3]}.. do not tie bit for bit"


def assert_join_matches(got, got_counts, want, want_counts, tag: str, exact_bits: bool = True):
    """``got`` (a ``RangeHits`` or a list of (labels, dist)) against the model: labels, counts, offsets and -- the float32
    distance being the oracle's float64 rounded once -- the float32 bits."""
    assert len(got) == len(want), f"{tag}: {len(got)} left rows answered, {len(want)} asked"
    assert np.array_equal(np.asarray(got_counts), want_counts), \
        f"{tag}: counts differ at {np.flatnonzero(np.asarray(got_counts) != want_counts)[:5]}"
    if isinstance(got, RangeHits):
        assert np.array_equal(got.offsets, offsets_of(want)), f"{tag}: offsets differ"
    for i, ((gl, gd), (wl, wd)) in enumerate(zip(got, want)):
        assert np.array_equal(gl, wl), f"{tag}: left row {i}: labels {gl[:6]} ({len(gl)}), the model has {wl[:6]} ({len(wl)})"
        if exact_bits:
            bad = np.flatnonzero(gd != wd)
            assert bad.size == 0, (f"{tag}: left row {i}: distance of label {wl[bad[0]]} is {gd[bad[0]]!r}, the oracle's "
                                   f"float64 rounded once is {wd[bad[0]]!r}")


def native_join(eng, left, mode: int, radius: float, capacity: int, total: int, where=None):
    """One mlvdb_join_within call -> (status, hits per left row or None, counts, offsets, raw label / dist arrays);
    total = 0: a counting call (NULL hit arrays).  The outputs start from sentinels, so what a call leaves untouched shows."""
    left = np.ascontiguousarray(left, dtype=np.int64)
    n = left.size
    lab = np.full(max(total, 1), -9, dtype=np.int64)
    dist = np.full(max(total, 1), -9.0, dtype=np.float32)
    off = np.full(n + 1, -1, dtype=np.int64)
    cnt = np.full(max(n, 1), -1, dtype=np.int64)
    w, keep = eng._where_arg(where)
    rc = eng._lib.mlvdb_join_within(eng.handle, left.ctypes.data if n else None, n, mode, C.c_float(radius), capacity, total, w,
                                    lab.ctypes.data if total else None, dist.ctypes.data if total else None,
                                    off.ctypes.data, cnt.ctypes.data)
    hits = None
    if total and rc in (_native.OK, _native.ERR_OVERFLOW) and off[-1] >= 0 and off[-1] <= total:
        hits = [(lab[off[i]:off[i + 1]], dist[off[i]:off[i + 1]]) for i in range(n)]
    return rc, hits, cnt[:n], off, lab, dist


class JoinOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``join_within`` as ``HipScanEngine`` declares it; ``calls`` counts the engine's work."""

    def __init__(self, dim: int, space: str) -> None:
        super().__init__(dim, space)
        self.calls = 0

    def join_within(self, labels, mode, radius, capacity, where=None, truncate=False):
        self.calls += 1
        left = np.asarray(labels, dtype=np.int64)
        assert mode in (OTHERS, LATER) and 1 <= capacity <= _native.JOIN_MAX_CAPACITY
        assert (np.diff(left) > 0).all() and ((left >= 0) & (left < self._rows.shape[0])).all()
        matching = None if where is None else self.match(where) | self._deleted  # (match() leaves the tombstoned out itself)
        want, counts = join_model(self._rows, left, radius, self.space, mode, deleted=self._deleted, matching=matching)
        if truncate:
            want = cut(want, capacity)
        lab = np.concatenate([l for l, _ in want]) if want else np.zeros(0, np.int64)
        dist = np.concatenate([d for _, d in want]) if want else np.zeros(0, np.float32)
        return RangeHits(lab.astype(np.int64), dist.astype(np.float32), offsets_of(want)), counts

    def where_labels(self, program):
        self.calls += 1
        return super().where_labels(program)


def oracle_index(attributes=None, space="l2", **kw) -> Index:
    return Index(space=space, engine_factory=JoinOracleEngine, attributes=attributes, **kw)
