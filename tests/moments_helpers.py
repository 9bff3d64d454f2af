"""The NumPy model of include/mlvdb_moments.h: slab sums over the candidate rows in ascending label, folded slab by slab."""
import numpy as np

SLAB = 4096  # MLVDB_MOMENTS_SLAB


def model_moments(rows: np.ndarray, cand=None):
    """(count, sums float64 [dim], gram float64 [dim, dim]) of ``rows`` float32 [n, dim] where ``cand`` bool [n] is set."""
    n, dim = rows.shape
    cand = np.ones(n, bool) if cand is None else np.asarray(cand, bool)
    sums, gram = np.zeros(dim), np.zeros((dim, dim))
    for first in range(0, n, SLAB):
        slab_sums, slab_gram = np.zeros(dim), np.zeros((dim, dim))
        for r in first + np.flatnonzero(cand[first:first + SLAB]):
            x = rows[r].astype(np.float64)
            slab_sums += x
            slab_gram += np.outer(x, x)  # (a product of two fp32 values is exact in fp64)
        sums += slab_sums
        gram += slab_gram
    return int(cand.sum()), sums, gram
