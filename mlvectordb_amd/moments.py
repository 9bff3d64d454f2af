"""Principal axes from the row moments (include/mlvdb_moments.h): what ``Index.pca`` returns, and the host step behind it."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class PcaResult:
    """``components`` float32 [m, dim]: unit rows, the principal axes by descending variance, each signed so that its entry
    of largest magnitude is positive; ``explained_variance`` float64 [m]: the variance along each; ``explained_variance_ratio``:
    its share of the total; ``mean`` float64 [dim] (zeros with ``center=False``); ``thresholds`` float64 [m]:
    ``components @ mean``, so that ``components[j] . x > thresholds[j]`` is the sign of the centred projection; ``count``:
    the rows the moments were taken over."""

    components: np.ndarray
    explained_variance: np.ndarray
    explained_variance_ratio: np.ndarray
    mean: np.ndarray
    thresholds: np.ndarray
    count: int

    def transform(self, vectors) -> np.ndarray:
        """The coordinates of ``vectors`` [n, dim] along the components, float64 [n, m], on the host."""
        return np.asarray(vectors, dtype=np.float64) @ self.components.astype(np.float64).T - self.thresholds


def pca_from_moments(count: int, sums, gram, n_components: int, center: bool = True) -> PcaResult:
    """PCA from the raw moments of ``count`` rows: ``sums`` [dim] and ``gram`` = ``X.T @ X`` [dim, dim], float64.

    ``mean = sums / count``; ``cov = (gram - count * mean mean^T) / (count - 1)``, or ``gram / count`` with
    ``center=False``; ``np.linalg.eigh`` of it, eigenvalues descending.  The decomposition of a dim x dim matrix is O(dim^3)
    whatever the row count, so it stays on the host.  Raw moments lose digits when the mean dwarfs the spread: the
    subtraction cancels about ``2 * log10(|mean| / spread)`` of float64's sixteen."""
    sums, gram = np.asarray(sums, dtype=np.float64), np.asarray(gram, dtype=np.float64)
    dim, count = sums.shape[0], int(count)
    if gram.shape != (dim, dim):
        raise ValueError(f"pca: gram must be [{dim}, {dim}] (got shape {gram.shape})")
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or not 1 <= n_components <= dim:
        raise ValueError(f"pca: n_components must be an int in [1, {dim}] (got {n_components!r})")
    if count < (2 if center else 1):
        raise ValueError(f"pca: {'a centred PCA needs two rows' if center else 'PCA needs a row'} at the least (got {count})")
    if center:
        mean = sums / count
        cov = (gram - count * np.outer(mean, mean)) / (count - 1)
    else:
        mean = np.zeros(dim)
        cov = gram / count
    values, vectors = np.linalg.eigh(cov)  # ascending
    order = np.argsort(values)[::-1][:int(n_components)]
    axes = vectors[:, order].T
    axes = axes * np.sign(axes[np.arange(axes.shape[0]), np.abs(axes).argmax(axis=1)])[:, None]
    components = (axes / np.linalg.norm(axes, axis=1, keepdims=True)).astype(np.float32)
    variance = np.maximum(values[order], 0.0)
    total = max(float(np.trace(cov)), np.finfo(np.float64).tiny)
    return PcaResult(components, variance, variance / total, mean, components.astype(np.float64) @ mean, count)
