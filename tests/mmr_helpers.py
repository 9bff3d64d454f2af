"""Shared by the diversified-kNN tests (include/mlvdb_mmr.h): the greedy selection in NumPy fp64, a brute-force restatement
of it, and an oracle engine with ``search_mmr``."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd.index import Index
from oracle import exact_scan
from tests.where_helpers import WhereOracleEngine

D64_BOUND = 1e-10  # what a device fp64 distance may differ from the oracle's by where the oracle's picks are asked for
GAP_MIN = 1e-9  # an fp64 sum of <= 208 exact products errs by <= 208 * 2^-53 * sum|terms| ~ 5e-11 at these shapes; an objective
                # inherits at most one such error from each of its two distances: 1e-9 leaves a tenfold margin


def mmr_select(dq, P, k: int, lam: float, step_gaps=None):
    """The greedy of mlvdb_mmr.h over one candidate list.  ``dq`` [m]: float64 distances to the query in rank order.
    ``P``: the float64 matrix P[s][i] = D(s, i), or a callable ``P(s)`` giving row s (only the picked rows are ever asked
    for).  The first pick is position 0; each further pick is the unpicked position minimising
    ``lam * dq[i] - (1.0 - lam) * mind[i]`` -- two rounded products, one rounded subtraction -- the first minimum in
    position order (a stable argmin).  Returns (picks int32 [min(k, m)], objectives float64, the smallest gap between the
    best and the runner-up objective over all steps that had a runner-up; inf when none had).  ``step_gaps``: a list that
    receives that gap of every step that had a runner-up."""
    dq = np.asarray(dq, dtype=np.float64)
    m = dq.size
    n = min(int(k), m)
    lam = float(lam)
    oml = 1.0 - lam
    row = P if callable(P) else (lambda s: P[s])
    rel = lam * dq
    mind = np.full(m, np.inf)
    free = np.ones(m, bool)
    picks = np.zeros(n, np.int32)
    objs = np.zeros(n, np.float64)
    gap = np.inf
    for t in range(n):
        if t == 0:
            s, o = 0, rel[0]
        else:
            cand = np.flatnonzero(free)
            oc = rel[cand] - oml * mind[cand]
            j = int(np.argmin(oc))  # the first minimum: the lower position
            s, o = int(cand[j]), oc[j]
            if cand.size > 1:
                step = float(np.partition(oc, 1)[1] - o)
                gap = min(gap, step)
                if step_gaps is not None:
                    step_gaps.append(step)
        picks[t], objs[t] = s, o
        free[s] = False
        if t + 1 < n:
            mind = np.minimum(mind, np.asarray(row(s), dtype=np.float64))
    return picks, objs, gap


def mmr_select_brute(dq, P, k: int, lam: float):
    """The same answer by the definition itself, position by position in Python floats (IEEE doubles)."""
    m = len(dq)
    oml = 1.0 - float(lam)
    picks, objs = [], []
    for t in range(min(k, m)):
        if t == 0:
            best = (float(lam) * float(dq[0]), 0)
        else:
            best = None
            for i in range(m):
                if i in picks:
                    continue
                mind = min(float(P[s][i]) for s in picks)
                key = (float(lam) * float(dq[i]) - oml * mind, i)
                if best is None or key < best:
                    best = key
        objs.append(best[0])
        picks.append(best[1])
    return picks, objs


def pad_mmr(nq: int, k: int):
    return (np.full((nq, k), -1, np.int64), np.full((nq, k), np.inf, np.float32), np.zeros(nq, np.int32),
            np.full((nq, k), np.inf), np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf))


def mmr_from_candidates(cl, cd32, cc, cd64, pair_rows, k: int, lam: float):
    """``search_mmr``'s six outputs from candidate lists (labels / float32 / counts / float64 of a search at fetch_k) and
    ``pair_rows(q, cands) -> P`` (matrix or callable).  Also returns the smallest objective gap of each query."""
    nq = cl.shape[0]
    labels, dist, counts, d64, rank, obj = pad_mmr(nq, k)
    gaps = np.full(nq, np.inf)
    for i in range(nq):
        m = int(cc[i])
        if m == 0:
            continue
        picks, objs, gaps[i] = mmr_select(cd64[i, :m], pair_rows(i, cl[i, :m]), k, lam)
        n = picks.size
        counts[i] = n
        labels[i, :n], dist[i, :n], d64[i, :n] = cl[i, picks], cd32[i, picks], cd64[i, picks]
        rank[i, :n], obj[i, :n] = picks, objs
    return (labels, dist, counts, d64, rank, obj), gaps


class MmrOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``search_mmr`` as ``HipScanEngine`` declares it."""

    def search_mmr(self, queries, k, fetch_k, lam, where=None, want64=False):
        assert 1 <= k <= 64 and k <= fetch_k <= 1024 and 0.0 <= lam <= 1.0
        cl, cd32, cc, cd64 = self.search64(queries, fetch_k, where=where)

        def pair_rows(_, cands):
            return exact_scan.exact_distances(self._rows[cands], self._rows[cands], self.space)

        out, _ = mmr_from_candidates(cl, cd32, cc, cd64, pair_rows, k, lam)
        return out if want64 else out[:3] + (None,) + out[4:]


def oracle_index(attributes=None, space="l2", **kw) -> Index:
    return Index(space=space, engine_factory=MmrOracleEngine, attributes=attributes, **kw)
