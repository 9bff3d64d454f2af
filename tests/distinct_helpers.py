"""Shared by the distinct-kNN tests (include/mlvdb_distinct.h): the NumPy oracle, a brute-force restatement of it, an oracle
engine with ``search_distinct``, and the launch geometry of the grouped scan (so a test can state which blocks and waves
hold a group's rows)."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import where as W
from mlvectordb_amd.index import Index
from oracle import exact_scan
from tests.where_helpers import WhereOracleEngine

ABSENT = W.INT64_ABSENT


def distinct_knn(dist: np.ndarray, groups: np.ndarray, allowed: np.ndarray, k: int):
    """The k nearest groups per query from a float64 distance matrix ``dist`` [nq, n]: over the rows that are ``allowed``
    (live, matching) and hold a present value, rank by (distance, label), take the first row of each group, then the first
    k.  Returns (labels int64 [nq, k], dist64 [nq, k], counts int32 [nq], groups int64 [nq, k]), padded -1 / inf / ABSENT."""
    nq = dist.shape[0]
    idx = np.flatnonzero(np.asarray(allowed, bool) & (groups != ABSENT))
    labels = np.full((nq, k), -1, np.int64)
    d64 = np.full((nq, k), np.inf)
    grp = np.full((nq, k), ABSENT, np.int64)
    counts = np.zeros(nq, np.int32)
    for i in range(nq):
        order = idx[np.lexsort((idx, dist[i, idx]))]
        _, first = np.unique(groups[order], return_index=True)
        keep = order[np.sort(first)][:k]
        counts[i] = keep.size
        labels[i, :keep.size], d64[i, :keep.size], grp[i, :keep.size] = keep, dist[i, keep], groups[keep]
    return labels, d64, counts, grp


def distinct_knn_brute(dist: np.ndarray, groups: np.ndarray, allowed: np.ndarray, k: int):
    """The same answer by the definition itself: the best (distance, label) row of every group, the groups ranked by it."""
    out = []
    for i in range(dist.shape[0]):
        best = {}
        for row in range(groups.size):
            g = int(groups[row])
            if not allowed[row] or g == ABSENT:
                continue
            key = (float(dist[i, row]), row)
            if g not in best or key < best[g]:
                best[g] = key
        out.append(sorted((d, row, g) for g, (d, row) in best.items())[:k])
    return out


class DistinctOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``search_distinct`` as ``HipScanEngine`` declares it."""

    def search_distinct(self, queries, k, attr, max_groups=0, where=None, want64=False):
        col = self._cols[attr]
        assert col.dtype == np.int64
        allowed = ~self._deleted if where is None else self.match(where)
        dist = exact_scan.exact_distances(queries, self._rows, self.space)
        labels, d64, counts, grp = distinct_knn(dist, col, allowed, k)
        if max_groups:
            assert counts.max(initial=0) <= max_groups
        d32 = d64.astype(np.float32)
        return (labels, d32, counts, d64, grp) if want64 else (labels, d32, counts, grp)


def oracle_index(attributes, space="l2", **kw) -> Index:
    return Index(space=space, engine_factory=DistinctOracleEngine, attributes=attributes, **kw)


# ---------------------------------------------------------------- launch geometry of the grouped exact scan
def scan_geometry(n: int, dim: int, nq_sel: int):
    """(queries per tile, panels per wave step, waves per block, blocks along the corpus) the grouped scan takes for ``n`` rows
    and ``nq_sel`` selected queries: plan_exact's rule (kernels_exact.hip) over internal.h's kExactTiles, which plan_distinct keeps."""
    ld = (dim + 15) // 16 * 16
    qt = 8 if nq_sel >= 8 else 4 if nq_sel >= 4 else 2 if nq_sel >= 2 else 1
    while qt > 1 and qt * ld * 8 > 64 * 1024:
        qt >>= 1
    nw = 16 if qt <= 2 else 8
    pw = 4 if qt == 4 else 2
    nqtiles = -(-nq_sel // qt)
    ntasks = -(-(-(-n // 16)) // pw)
    nblk = max(1, min(-(-ntasks // nw), max(8, min(256, 1024 // nqtiles))))
    return qt, pw, nw, nblk


def block_and_wave(rows: np.ndarray, geometry):
    """(block, wave) that scans each of ``rows``: task t = rows [t * pw * 16, (t + 1) * pw * 16) goes to slot
    t mod (nblk * nw), block = slot // nw, wave = slot mod nw."""
    _, pw, nw, nblk = geometry
    slot = (np.asarray(rows) // (pw * 16)) % (nblk * nw)
    return slot // nw, slot % nw


def group_spans_blocks_and_waves(groups: np.ndarray, live: np.ndarray, geometry) -> bool:
    """Does some group have live rows in at least two blocks, and some group live rows in two waves of one block?"""
    rows = np.flatnonzero(live & (groups != ABSENT))
    blk, wav = block_and_wave(rows, geometry)
    g = groups[rows]
    two_blocks = two_waves = False
    for code in np.unique(g)[:2000]:
        sel = g == code
        two_blocks = two_blocks or np.unique(blk[sel]).size >= 2
        pairs = np.unique(np.stack([blk[sel], wav[sel]], axis=1), axis=0)
        two_waves = two_waves or (pairs.shape[0] > np.unique(pairs[:, 0]).size)
        if two_blocks and two_waves:
            return True
    return False
