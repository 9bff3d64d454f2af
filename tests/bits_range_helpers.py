"""The model of range search over bit codes (include/mlvdb_bits_range.h): integer distances from ``np.unpackbits`` sums, one
fp64 division for Jaccard (``bits_helpers.distances``), hits ranked by ``np.lexsort`` on (label, distance).  Nothing here asks
the library for an answer: ``engine.RangeHits`` is used as the plain container the engines return."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd.engine import RangeHits
from tests.bits_helpers import METRICS, BitsOracleEngine, distances

MAX_HITS = 16384  # MLVDB_BITS_RANGE_MAX_HITS


def range_bits(model, attr, queries, radius, metric="hamming", capacity=MAX_HITS, where=None):
    """(labels int64, dist64 float64, offsets int64 [nq + 1], counts int64 [nq]) of the packed answer: a query with more
    than ``capacity`` hits has its exact count and an empty segment."""
    assert metric in METRICS and 1 <= capacity <= MAX_HITS and radius == radius
    queries = np.asarray(queries, dtype=np.uint64)
    nq, words = queries.shape
    idx = np.flatnonzero(model.candidates(attr, where, words))
    codes = np.array([model.bits_rows(attr)[i] for i in idx.tolist()], dtype=np.uint64).reshape(idx.size, words)
    dist = distances(queries, codes, metric) if idx.size and nq else np.zeros((nq, idx.size))
    labels, d64, counts = [], [], np.zeros(nq, dtype=np.int64)
    offsets = np.zeros(nq + 1, dtype=np.int64)
    for q in range(nq):
        hit = np.flatnonzero(dist[q] <= radius)
        counts[q] = hit.size
        if hit.size <= capacity:
            order = hit[np.lexsort((idx[hit], dist[q, hit]))]
            labels.append(idx[order])
            d64.append(dist[q, order])
        offsets[q + 1] = offsets[q] + (hit.size if hit.size <= capacity else 0)
    cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    return cat(labels, np.int64), cat(d64, np.float64), offsets, counts


class BitsRangeOracleEngine(BitsOracleEngine):
    """``BitsOracleEngine`` + ``range_bits`` with the signature and the returns of ``HipScanEngine.range_bits``."""

    def range_bits(self, attr, queries, radius, metric="hamming", capacity=MAX_HITS, where=None, count_only=False):
        assert attr in self._bits
        labels, d64, offsets, counts = range_bits(self, attr, queries, radius, metric, capacity, where)
        return counts if count_only else (RangeHits(labels, d64.astype(np.float32), offsets), d64, counts)
