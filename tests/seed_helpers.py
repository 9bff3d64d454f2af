"""Shared by the seeding tests: include/mlvdb_seed.h's sum tree, descent and greedy k-means++ steps in NumPy -- one ufunc or
one Python float operation per step, so every step is one rounded IEEE binary64 operation -- and a model engine."""
import numpy as np

from mlvectordb_amd import _native as N
from tests.cluster_helpers import ClusterOracleEngine


def tree(w):
    """The levels of T(w), level 0 first: ``w`` padded with +0.0 to P leaves, every level the pairwise sums of the one below."""
    P = N.SEED_BLOCK
    while P < len(w):
        P *= 2
    levels = [np.concatenate([np.asarray(w, np.float64), np.zeros(P - len(w))])]
    while levels[-1].size > 1:
        levels.append(np.add(levels[-1][0::2], levels[-1][1::2]))
    return levels


def draw(levels, u):
    """draw(T, u) = descend(T, u * root): the label reached."""
    r = np.float64(u) * levels[-1][0]
    i = 0
    for level in reversed(levels[:-1]):
        a, b = level[2 * i], level[2 * i + 1]
        if b == 0:
            i = 2 * i
        elif a == 0:
            i = 2 * i + 1
        elif r < a:
            i = 2 * i
        else:
            r, i = r - a, 2 * i + 1
    return i


def model_seed(distance, live, m, u):
    """The header's steps.  ``distance(s)`` -> float64 [n]: d(s, x) for every label x; ``live`` bool [n]: the candidates;
    ``u`` float64 [m, trials].  Returns (labels int64 [m] in pick order, potentials float64 [m], candidates)."""
    live, u = np.asarray(live, bool), np.asarray(u, np.float64)

    def clamped(s):
        d = np.asarray(distance(s), np.float64)
        with np.errstate(invalid="ignore"):
            return np.where(live & (d > 0), d, 0.0)

    ones = tree(live.astype(np.float64))
    labels = [draw(ones, u[0, 0])]
    best = clamped(labels[0])
    B = tree(best)
    potentials = [B[-1][0]]
    for j in range(1, m):
        source, won = B if B[-1][0] > 0 else ones, None
        for t in range(u.shape[1]):
            s = draw(source, u[j, t])
            c = clamped(s)
            p = np.where(c < best, c, best)
            T = tree(p)
            if won is None or T[-1][0] < won[0][-1][0]:
                won = (T, s, p)
        B, s, best = won
        labels.append(s)
        potentials.append(B[-1][0])
    return np.array(labels, np.int64), np.array(potentials, np.float64), int(live.sum())


def seed_u(seed, k, trials):
    """The random numbers ``Index`` hands the engine."""
    return np.random.default_rng(seed).random((k, N.SEED_MAX_TRIALS))[:, :trials]


class SeedOracleEngine(ClusterOracleEngine):
    """``ClusterOracleEngine`` + ``kmeans_seed``; ``started``: the labels every ``kmeans`` call was started from."""

    started = ()

    def kmeans_seed(self, m, u, *, where=None):
        live = self._candidates(where)
        assert self.space != "ip" and 1 <= m <= live.sum() and len(u) == m and ((u >= 0) & (u < 1)).all()
        return model_seed(lambda s: self._distances(self._rows[s:s + 1])[0], live, m, u)

    def kmeans(self, labels, vectors=None, **kw):
        self.started += (np.asarray(labels).tolist(),)
        return super().kmeans(labels, vectors, **kw)
