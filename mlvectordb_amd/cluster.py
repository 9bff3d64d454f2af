"""Clustering of the stored rows (include/mlvdb_cluster.h): what ``Index.cluster`` returns."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

METRICS = ("l2", "cosine")            # the metrics k-means takes: the ones a mean minimises
ASSIGN_METRICS = ("l2", "cosine", "ip")  # ... and the ones the nearest-centroid assignment takes


def left_to_right(costs) -> float:
    """The sum of ``costs`` left to right in float64 from +0.0: how ``inertia`` is defined."""
    total = 0.0
    for c in np.asarray(costs, dtype=np.float64).tolist():
        total = total + c
    return total


@dataclass
class ClusterResult:
    """``centroids`` float32 [k, dim]; ``sizes`` int64 [k]: the members of every cluster; ``costs`` float64 [k]: the sum of
    the members' distances to their centroid, in the index's own distance (squared for "l2", ``1 - cosine`` for "cosine")
    and in the order the header states; ``inertia``: ``costs`` summed left to right; ``iterations`` run; ``converged``: the
    last one moved no row, so the centroids are the means of exactly the clusters returned."""

    centroids: np.ndarray
    sizes: np.ndarray
    costs: np.ndarray
    inertia: float
    iterations: int
    converged: bool

    @classmethod
    def of(cls, centroids, sizes, costs, iterations, converged) -> "ClusterResult":
        return cls(centroids, sizes, costs, left_to_right(costs), int(iterations), bool(converged))
