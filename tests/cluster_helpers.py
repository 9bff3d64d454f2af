"""Shared by the clustering tests (include/mlvdb_cluster.h): the header's rule and its blocked sums written in NumPy -- one
ufunc per step on float64 arrays, so every step is one rounded IEEE binary64 operation --, Lloyd's loop around them, and an
oracle engine with ``assign_nearest`` / ``kmeans``."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import _native as N
from mlvectordb_amd import where as W
from oracle import exact_scan
from tests.where_helpers import WhereOracleEngine

SEGMENT = N.CLUSTER_SEGMENT
UNASSIGNED = -1
NO_CANDIDATE = -2


def model_assign(D, live):
    """The rule over a distance matrix.  ``D`` float64 [m, n]: the distance of centroid j to row x; ``live`` bool [n]: the
    candidates.  For j ascending a centroid wins when ``D[j] < best`` (from +inf): ties go to the lower j, a NaN and +inf
    never win.  Returns (assign int64 [n]: j, ``UNASSIGNED``, or ``NO_CANDIDATE`` outside ``live``; best float64 [n])."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[1]
    best = np.full(n, np.inf)
    assign = np.full(n, UNASSIGNED, np.int64)
    with np.errstate(all="ignore"):
        for j in range(D.shape[0]):
            win = D[j] < best
            best = np.where(win, D[j], best)
            assign[win] = j
    assign[~np.asarray(live, bool)] = NO_CANDIDATE
    return assign, best


def _running(values):
    """The left-to-right fp64 sum along axis 0 starting from +0.0 (``np.add.accumulate`` adds one row at a time)."""
    values = np.asarray(values, dtype=np.float64)
    zero = np.zeros((1,) + values.shape[1:])
    return np.add.accumulate(np.concatenate([zero, values], axis=0), axis=0)[-1]


def blocked_sum(values):
    """The header's blocked sum along axis 0: segments of ``SEGMENT`` members, each summed left to right from +0.0, the
    segment sums summed left to right from +0.0."""
    values = np.asarray(values, dtype=np.float64)
    parts = [_running(values[a:a + SEGMENT]) for a in range(0, values.shape[0], SEGMENT)]
    return _running(np.stack(parts)) if parts else np.zeros(values.shape[1:])


def row_weights(rows):
    """w(x) = 1 / (sqrt(nx) + 1e-30) per row, nx in the scans' order: with the columns zero-padded to a multiple of 16,
    s_g = the squares of columns 16 kb + 4 g + i summed over kb then i from +0.0, nx = (s_0 + s_1) + (s_2 + s_3).  The square
    of a float32 is exact in float64."""
    rows = np.asarray(rows, dtype=np.float32)
    n, d = rows.shape
    ld = (d + 15) // 16 * 16
    x = np.zeros((n, ld))
    x[:, :d] = rows
    sq = np.multiply(x, x).reshape(n, ld // 16, 4, 4)  # [row, kb, g, i]
    s = [_running(sq[:, :, g, :].reshape(n, -1).T) for g in range(4)]
    nx = np.add(np.add(s[0], s[1]), np.add(s[2], s[3]))
    return np.divide(1.0, np.add(np.sqrt(nx), 1e-30))


def model_means(rows, assign, m, space, prev):
    """The centroids after one update: per cluster the blocked sum of its members' addends in ascending label order --
    ``(double)x`` for l2, ``(double)x * w(x)`` for cosine --, divided by the count in float64, rounded once to float32; a
    cluster without members keeps ``prev[j]``.  ``rows`` float32 [n, d] by label, ``assign`` [n] as ``model_assign`` returns."""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.array(prev, dtype=np.float32, copy=True)
    w = row_weights(rows) if space == "cosine" else None
    for j in range(m):
        mem = np.flatnonzero(np.asarray(assign) == j)
        if mem.size == 0:
            continue
        addend = rows[mem].astype(np.float64)
        if w is not None:
            addend = np.multiply(addend, w[mem][:, None])
        out[j] = np.divide(blocked_sum(addend), np.float64(mem.size)).astype(np.float32)
    return out


def model_sizes_costs(assign, best, m):
    """(sizes int64 [m], costs float64 [m]): the members of every cluster and the blocked sum of their best distances."""
    sizes = np.array([(np.asarray(assign) == j).sum() for j in range(m)], dtype=np.int64)
    costs = np.array([blocked_sum(best[np.flatnonzero(np.asarray(assign) == j)]) for j in range(m)], dtype=np.float64)
    return sizes, costs


def model_kmeans(distances, rows, live, c0, space, max_iterations):
    """Lloyd's loop as the header states it.  ``distances(C)`` -> float64 [m, n] for centroids ``C`` float32 [m, d] (the
    device's own ``pair_distances`` in the replay tests, the oracle's elsewhere).  Returns (centroids, sizes, costs,
    iterations, converged, assign) of the last iteration."""
    c = np.array(c0, dtype=np.float32, copy=True)
    m = c.shape[0]
    prev = None
    for t in range(1, max_iterations + 1):
        assign, best = model_assign(distances(c), live)
        c = model_means(rows, assign, m, space, c)
        converged = t >= 2 and np.array_equal(assign, prev)
        prev = assign
        if converged or t == max_iterations:
            break
    sizes, costs = model_sizes_costs(assign, best, m)
    return c, sizes, costs, t, converged, assign


def centroid_vectors(rows, labels, vectors):
    """float32 [m, dim]: every centroid as a vector -- the stored row or the raw one."""
    if labels is None:
        return np.array(vectors, dtype=np.float32, copy=True)
    labels = np.asarray(labels, np.int64)
    out = np.array(vectors, dtype=np.float32, copy=True) if vectors is not None else np.zeros((labels.size, rows.shape[1]), np.float32)
    out[labels >= 0] = rows[labels[labels >= 0]]
    return out


class ClusterOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``assign_nearest`` / ``kmeans`` as ``HipScanEngine`` declares them:
    ``exact_scan.exact_distances`` for the distances, the model above for the rest."""

    def _distances(self, c):
        return exact_scan.exact_distances(np.asarray(c, np.float32), self._rows, self.space)

    def _candidates(self, where):
        return ~self._deleted if where is None else self.match(where)

    def _write(self, attr, assign):
        if attr < 0:
            return
        assert self._cols[attr].dtype == np.int64
        cand = assign != NO_CANDIDATE
        self._cols[attr][cand] = np.where(assign[cand] >= 0, assign[cand], W.INT64_ABSENT)

    def _check(self, labels, vectors):
        c = centroid_vectors(self._rows, labels, vectors)
        assert 1 <= c.shape[0] <= N.CLUSTER_MAX and c.shape[1] == self.dim and np.isfinite(c).all()
        if labels is not None:
            labels = np.asarray(labels)
            assert ((labels >= -1) & (labels < self._rows.shape[0])).all()
        return c

    def assign_nearest(self, labels, vectors=None, *, where=None, assign_attr=-1):
        c = self._check(labels, vectors)
        live = self._candidates(where)
        assign, best = model_assign(self._distances(c) if self._rows.shape[0] else np.zeros((c.shape[0], 0)), live)
        self._write(assign_attr, assign)
        sizes, costs = model_sizes_costs(assign, best, c.shape[0])
        return sizes, costs, int(live.sum())

    def kmeans(self, labels, vectors=None, *, max_iterations=25, where=None, assign_attr=-1):
        assert self.space != "ip" and 1 <= max_iterations <= N.CLUSTER_MAX_ITERATIONS
        c0 = self._check(labels, vectors)
        live = self._candidates(where)
        dist = self._distances if self._rows.shape[0] else (lambda c: np.zeros((c.shape[0], 0)))
        c, sizes, costs, t, converged, assign = model_kmeans(dist, self._rows, live, c0, self.space, max_iterations)
        self._write(assign_attr, assign)
        return c, sizes, costs, t, bool(converged), int(live.sum())
