"""The NumPy model of include/mlvdb_transform.h: the projection of tests/project_helpers.py, one fp64 subtract, one rounding."""
import numpy as np

from tests.project_helpers import proj


def model_transform(rows: np.ndarray, matrix: np.ndarray, shift=None) -> np.ndarray:
    """float32 [n, out_dim] of ``rows`` float32 [n, dim] (the candidates in ascending label)."""
    shift = np.zeros(matrix.shape[0]) if shift is None else np.asarray(shift, dtype=np.float64)
    with np.errstate(over="ignore"):
        return (proj(np.asarray(matrix, np.float32), rows) - shift[None, :]).astype(np.float32)
