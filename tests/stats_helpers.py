"""Shared by the attribute-statistics tests (include/mlvdb_stats.h): the model of the entry in NumPy and Python integers --
exact sums, totalOrder min / max and the header's fixed-point rule written out --, an oracle engine that answers
``attr_stats`` without a GPU, and the constants of the kernels."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from mlvectordb_amd.engine import StatsOverflow
from tests import facet_helpers as F
from tests.where_helpers import SCHEMA, py_match
from tests.facet_helpers import ABSENT, INT64_MAX, MAX_VALUES, GRID_ROWS, colliding_keys, facet_hash, global_slots  # noqa: F401

# csrc/internal.h: the per-block table of the statistics kernels; the probe bound and the peel rounds are the facet kernels'
LDS_SLOTS = 1024   # kStatsLdsSlots
LDS_SLOTS_ONE = 64  # kStatsLdsSlotsOne: the block table of an ungrouped call
LDS_PROBES = F.LDS_PROBES  # kFacetLdsProbes
PEEL_ROUNDS = 8    # kFacetPeelRounds
SCALE = 61         # a term is rint(v * 2**(SCALE - E))


# ---------------------------------------------------------------- the model
def total_order(col: np.ndarray) -> np.ndarray:
    """uint64 keys whose integer order is IEEE totalOrder of the doubles in ``col`` (-0.0 below +0.0)."""
    bits = np.ascontiguousarray(col, dtype=np.float64).view(np.uint64)
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, ~bits, bits | np.uint64(1 << 63))


def exact_sum(ints: np.ndarray) -> int:
    """The sum of an int64 array as a Python int: the high and low halves summed apart, so nothing wraps."""
    return (int((ints >> 32).sum()) << 32) + int((ints & 0xFFFFFFFF).sum())


def fixed_sum(values: np.ndarray):
    """The fixed-point sum S of the present (non-NaN) float64 ``values`` of one group, and E (None when S is 0 by rule)."""
    finite = values[np.isfinite(values)]
    if finite.size < values.size or finite.size == 0:
        return 0, None  # an infinity in the group (or no value at all)
    m = float(np.abs(finite).max())
    if m == 0.0:
        return 0, None
    E = math.frexp(m)[1] - 1  # floor(log2 m), subnormals included
    assert math.ldexp(1.0, E) <= m and (E == 1023 or m < math.ldexp(1.0, E + 1))
    terms = np.rint(np.ldexp(finite, SCALE - E)).astype(np.int64)  # the scaling is exact, rint rounds half to even
    return exact_sum(terms), E


def final_sum(S: int, E, lo: float, hi: float) -> float:
    """The double a float group's sum comes back as: one rounding of S * 2**(E - 61), through a Fraction."""
    if lo == -math.inf or hi == math.inf:
        return math.nan if (lo == -math.inf and hi == math.inf) else (-math.inf if lo == -math.inf else math.inf)
    if E is None:
        return 0.0
    try:
        return float(Fraction(S) * Fraction(2) ** (E - SCALE))
    except OverflowError:
        return math.copysign(math.inf, S)


def float_sum_model(values) -> float:
    """The returned sum of a group holding the doubles ``values``."""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return 0.0
    S, E = fixed_sum(v)
    order = total_order(v)
    return final_sum(S, E, float(v[order.argmin()]), float(v[order.argmax()]))


def stats_oracle(col: np.ndarray, by_col, mask: np.ndarray):
    """(keys ascending, rows, count, min, max, sums -- Python ints: exact or fixed-point --, matched, by_absent) of ``col``
    over the rows of ``mask`` (live and matching) grouped by int64 ``by_col``, or as one group under key 0 (``by_col is
    None``: that group exists even when nothing matches).  min / max of a group without values are 0."""
    f64 = col.dtype == np.float64
    present = F.present_of(col)
    if by_col is None:
        keys, member, by_absent = np.zeros(1, np.int64), [mask], 0
    else:
        has = mask & (by_col != ABSENT)
        keys = np.unique(by_col[has]).astype(np.int64)
        member = [has & (by_col == k) for k in keys.tolist()] if keys.size <= 64 else None
        by_absent = int((mask & ~has).sum())
        if member is None:  # many groups: one sort instead of one mask per key
            idx = np.flatnonzero(has)
            idx = idx[np.argsort(by_col[idx], kind="stable")]
            cuts = np.flatnonzero(np.diff(by_col[idx])) + 1
            member = np.split(idx, cuts)
    rows, count, sums = [], [], []
    mn, mx = np.zeros(keys.size, col.dtype), np.zeros(keys.size, col.dtype)
    for g, rows_of in enumerate(member):
        sel = col[rows_of]
        vals = sel[present[rows_of]]
        rows.append(int(sel.size))
        count.append(int(vals.size))
        if vals.size:
            order = total_order(vals) if f64 else vals
            mn[g], mx[g] = vals[order.argmin()], vals[order.argmax()]
        sums.append(fixed_sum(vals)[0] if f64 else exact_sum(vals))
    return keys, np.array(rows, np.int64), np.array(count, np.int64), mn, mx, sums, int(mask.sum()), by_absent


def split_sums(sums):
    """Python ints -> (hi int64, lo uint64) arrays, two's complement in 128 bits."""
    hi = np.array([s >> 64 for s in sums], dtype=np.int64)
    lo = np.array([s & (2 ** 64 - 1) for s in sums], dtype=np.uint64)
    return hi, lo


class StatsOracleEngine(F.FacetOracleEngine):
    """``FacetOracleEngine`` + ``attr_stats`` of ``HipScanEngine``, from the model."""

    def attr_stats(self, attr, by=None, max_groups=1, where=None):
        keys, rows, count, mn, mx, sums, matched, by_absent = stats_oracle(
            self._cols[attr], None if by is None else self._cols[by], self._mask(where))
        if keys.size > max_groups:
            raise StatsOverflow(max_groups, int(keys.size), matched, by_absent)
        return (keys, rows, count, mn, mx) + split_sums(sums) + (matched, by_absent)


# ---------------------------------------------------------------- the answer of Index.stats, from metadata dicts
def metadata_stats(metas, attr, where, by=None, schema=SCHEMA):
    """``Index.stats`` in plain Python over the metadata dicts of the live rows: exact integer sums, the modelled float sum."""
    kind = schema[attr]
    rows = [m for m in metas if where is None or py_match(where, m, schema)]

    def summary(ms):
        xs = [m.get(attr) for m in ms]
        xs = [x for x in xs if x is not None and x == x]
        if not xs:
            return {"count": 0, "min": None, "max": None, "sum": 0, "mean": None}
        total = float_sum_model(xs) if kind == "float" else sum(int(x) for x in xs)
        return {"count": len(xs), "min": min(xs), "max": max(xs), "sum": total, "mean": total / len(xs)}

    if by is None:
        s = summary(rows)
        return {"matched": len(rows), "absent": len(rows) - s["count"], **s}
    keys = sorted({m[by] for m in rows if m.get(by) is not None})
    groups = [(k, [m for m in rows if m.get(by) is not None and m[by] == k]) for k in keys]
    return {"groups": [(k, {"rows": len(ms), **summary(ms)}) for k, ms in groups], "matched": len(rows),
            "by_absent": sum(1 for m in rows if m.get(by) is None)}
