"""Shared by the recommend / discover tests (include/mlvdb_examples.h): the header's reduction over a bag of examples written
in NumPy -- one ufunc per step on float64 arrays, so every step is one rounded IEEE binary64 operation -- the ranking by
(tier, value, label) as a stable sort, seeded bags, and an oracle engine with ``search_examples``."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import _native as N
from oracle import exact_scan
from tests.where_helpers import WhereOracleEngine

BEST, DISCOVER, CONTEXT = N.EXAMPLES_BEST, N.EXAMPLES_DISCOVER, N.EXAMPLES_CONTEXT
POS, NEG, TARGET = N.EXAMPLE_POS, N.EXAMPLE_NEG, N.EXAMPLE_TARGET
NO_TIER = np.iinfo(np.int32).max


def bag_keys(mode: int, D, roles):
    """(tier int32 [n], value float64 [n]) of every row for one query.  ``D`` float64 [m, n]: the distance of example j to
    row x; ``roles`` [m].  A minimum over no example is +inf, one over a NaN is NaN (``np.minimum`` propagates it)."""
    D = np.asarray(D, dtype=np.float64)
    roles = np.asarray(roles)
    n = D.shape[1]
    inf = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        if mode == BEST:
            pos, neg = D[roles == POS], D[roles == NEG]
            p = np.minimum.reduce(pos, axis=0) if pos.shape[0] else inf
            m = np.minimum.reduce(neg, axis=0) if neg.shape[0] else inf
            liked = (p < m) | (neg.shape[0] == 0) if pos.shape[0] else np.zeros(n, bool)
            return np.where(liked, 0, 1).astype(np.int32), np.where(liked, p, np.negative(m))
        head = 1 if mode == DISCOVER else 0
        assert (D.shape[0] - head) % 2 == 0 and (head == 0 or roles[0] == TARGET)
        tier = np.zeros(n, np.int32)
        s = np.zeros(n)
        for i in range(head, D.shape[0], 2):
            assert roles[i] == POS and roles[i + 1] == NEG
            dp, dn = D[i], D[i + 1]
            tier += ~(dp < dn)
            s = np.add(s, np.where(dp > dn, np.subtract(dp, dn), 0.0))
        return (tier, D[0].copy()) if mode == DISCOVER else (np.zeros(n, np.int32), s)


def tiered_topk(tier, value, k: int, candidates):
    """The ranking of one query: the min(k, candidates) rows of ``candidates`` (bool [n]) whose value is no NaN, by a stable
    sort on (tier, value) -- so -0.0 == +0.0 and ties keep label order.  Returns (labels int64 [k] padded -1, tiers int32
    padded INT32_MAX, values float64 padded +inf, count)."""
    idx = np.flatnonzero(np.asarray(candidates, bool) & ~np.isnan(value))
    pick = idx[np.lexsort((value[idx], tier[idx]))][:k]
    labels = np.full(k, -1, np.int64)
    tiers = np.full(k, NO_TIER, np.int32)
    values = np.full(k, np.inf)
    labels[:pick.size], tiers[:pick.size], values[:pick.size] = pick, tier[pick], value[pick]
    return labels, tiers, values, pick.size


def model_search(mode, D_of_example, ex_labels, roles, offsets, k, live, exclude=True):
    """The whole call: ``D_of_example`` float64 [examples, n], ``live`` bool [n] (live and matching the filter)."""
    nq = len(offsets) - 1
    out = (np.full((nq, k), -1, np.int64), np.full((nq, k), NO_TIER, np.int32), np.full((nq, k), np.inf),
           np.zeros(nq, np.int32))
    for q in range(nq):
        a, b = int(offsets[q]), int(offsets[q + 1])
        tier, value = bag_keys(mode, D_of_example[a:b], roles[a:b])
        cand = np.asarray(live, bool).copy()
        if exclude:
            own = np.asarray(ex_labels[a:b])
            cand[own[own >= 0]] = False
        out[0][q], out[1][q], out[2][q], out[3][q] = tiered_topk(tier, value, k, cand)
    return out


def random_bags(rng, mode, sizes, n_rows, dim, raw_share=0.3, repeat_share=0.2, pool=None):
    """Seeded bags of the given sizes: (labels int64, vectors float32 [examples, dim], roles int32, offsets int64).  Stored
    and raw examples mixed, labels repeated inside a bag; ``pool``: the labels stored examples are drawn from (default: all
    rows).  DISCOVER / CONTEXT sizes count the target; an impossible size is rounded down to the nearest possible one."""
    labels, roles, offsets = [], [], [0]
    pool = np.arange(n_rows) if pool is None else np.asarray(pool)
    for m in sizes:
        if mode == DISCOVER:
            m = m if m % 2 == 1 else m - 1
            r = [TARGET] + [POS, NEG] * ((m - 1) // 2)
        elif mode == CONTEXT:
            m = max(2, m - m % 2)
            r = [POS, NEG] * (m // 2)
        else:
            r = rng.choice([POS, NEG], m, p=[0.6, 0.4]).tolist()
        lab = rng.choice(pool, m).tolist() if pool.size else [-1] * m
        for j in range(1, m):
            if rng.random() < repeat_share:
                lab[j] = lab[int(rng.integers(j))]
        lab = [-1 if rng.random() < raw_share else x for x in lab]
        labels += lab
        roles += r
        offsets.append(len(labels))
    labels = np.asarray(labels, np.int64)
    vectors = rng.standard_normal((labels.size, dim)).astype(np.float32)
    return labels, vectors, np.asarray(roles, np.int32), np.asarray(offsets, np.int64)


def example_vectors(rows, labels, vectors):
    """float32 [examples, dim]: every example as a vector -- the stored row or the raw one."""
    out = np.array(vectors, dtype=np.float32, copy=True) if vectors is not None else np.zeros((len(labels), rows.shape[1]), np.float32)
    stored = np.asarray(labels) >= 0
    out[stored] = rows[np.asarray(labels)[stored]]
    return out


class ExamplesOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``search_examples`` as ``HipScanEngine`` declares it: ``exact_scan.exact_distances`` for the
    distances, the model above for the rest."""

    def search_examples(self, mode, labels, vectors, roles, offsets, k, *, exclude=True, where=None):
        assert 1 <= k <= 64
        labels = np.asarray(labels, np.int64)
        assert ((labels >= -1) & (labels < self._rows.shape[0])).all()
        ex = example_vectors(self._rows, labels, vectors)
        D = exact_scan.exact_distances(ex, self._rows, self.space) if labels.size else np.zeros((0, self._rows.shape[0]))
        live = ~self._deleted if where is None else self.match(where)
        return model_search(mode, D, labels, np.asarray(roles), np.asarray(offsets), k, live, exclude)
