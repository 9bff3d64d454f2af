"""Shared by the facet tests (include/mlvdb_facet.h): the NumPy oracle of both entries, an oracle engine that answers them
without a GPU, and the kernels' hash mirrored so that tests can build keys that share a probe chain."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import where as W
from mlvectordb_amd.engine import FacetOverflow
from tests.where_helpers import WhereOracleEngine

ABSENT = W.INT64_ABSENT
INT64_MAX = np.iinfo(np.int64).max
MAX_VALUES = 1 << 20  # MLVDB_FACET_MAX_VALUES
MAX_EDGES = 4096      # MLVDB_FACET_MAX_EDGES
# csrc/internal.h: the per-block table of facet_values_kernel and the launch shape it shares with where_eval_kernel
LDS_SLOTS = 4096
LDS_PROBES = 8
GRID_ROWS = 4096 * 256  # rows one pass of the grid covers: beyond, threads take a second row


# ---------------------------------------------------------------- the hash (csrc/internal.h: facet_hash)
def facet_hash(v) -> np.ndarray:
    """uint64: x = v * 0x9E3779B97F4A7C15 mod 2^64; x ^ (x >> 32).  A key's first slot is ``facet_hash(v) & (slots - 1)``."""
    with np.errstate(over="ignore"):
        x = np.asarray(v, dtype=np.int64).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    return x ^ (x >> np.uint64(32))


def global_slots(max_values: int) -> int:
    """Slots of the global table of a call: the power of two >= max(64, 2 max_values)."""
    slots = 64
    while slots < 2 * max_values:
        slots *= 2
    return slots


def colliding_keys(slots: int, n: int, slot: int = 5, start: int = 1) -> np.ndarray:
    """The first ``n`` integers >= ``start`` whose first slot in a table of ``slots`` is ``slot``: one probe chain."""
    out, lo = [], start
    while len(out) < n:
        cand = np.arange(lo, lo + 65536, dtype=np.int64)
        out.extend(cand[(facet_hash(cand) & np.uint64(slots - 1)) == np.uint64(slot)].tolist())
        lo += 65536
    return np.array(out[:n], dtype=np.int64)


# ---------------------------------------------------------------- the oracle
def present_of(col: np.ndarray) -> np.ndarray:
    return ~np.isnan(col) if col.dtype == np.float64 else col != ABSENT


def values_oracle(col: np.ndarray, mask: np.ndarray):
    """(values ascending, counts, matched, absent) of int64 ``col`` over the rows of ``mask`` (live and matching)."""
    present = present_of(col)
    values, counts = np.unique(col[mask & present], return_counts=True)
    return values.astype(np.int64), counts.astype(np.int64), int(mask.sum()), int((mask & ~present).sum())


def bins_oracle(col: np.ndarray, edges: np.ndarray, mask: np.ndarray):
    """(counts [len(edges) + 1], matched, absent): np.searchsorted(edges, v, side="right") of the present values."""
    present = present_of(col)
    v = col[mask & present]
    counts = np.bincount(np.searchsorted(edges, v, side="right"), minlength=edges.size + 1).astype(np.int64)
    return counts, int(mask.sum()), int((mask & ~present).sum())


class FacetOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + the two facet entries of ``HipScanEngine``, in NumPy."""

    def _mask(self, where):
        return ~self._deleted if where is None else self.match(where)

    def facet_values(self, attr, max_values, where=None):
        values, counts, matched, absent = values_oracle(self._cols[attr], self._mask(where))
        if values.size > max_values:
            raise FacetOverflow(max_values, int(values.size), matched, absent)
        return values, counts, matched, absent

    def facet_bins(self, attr, edges, where=None):
        edges = np.asarray(edges)
        assert edges.dtype == self._cols[attr].dtype
        return bins_oracle(self._cols[attr], edges, self._mask(where))
