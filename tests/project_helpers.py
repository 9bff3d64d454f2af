"""The NumPy model of include/mlvdb_project.h: the projection in the header's summation order, the bits, the packing."""
import numpy as np


def proj(planes: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """proj(planes[j], rows[i]) as float64 [n, nbits]: four slice sums per pair, columns ascending inside a slice (one
    rounded add each; a product of two fp32 values is exact in fp64), then (S0 + S1) + (S2 + S3)."""
    (n, dim), ld = rows.shape, (rows.shape[1] + 15) // 16 * 16
    X, P = np.zeros((n, ld)), np.zeros((planes.shape[0], ld))
    X[:, :dim], P[:, :dim] = rows, planes
    S = np.zeros((n, planes.shape[0], 4))
    for group in range(0, ld, 16):
        for j in range(4):
            cols = group + 4 * np.arange(4) + j  # the j-th column of each of the four slices
            S += X[:, None, cols] * P[None, :, cols]
    return (S[..., 0] + S[..., 1]) + (S[..., 2] + S[..., 3])


def pack(bits: np.ndarray) -> np.ndarray:
    """bool [n, nbits] -> uint64 [n, nbits / 64]: bit b is bit b & 63 of word b >> 6."""
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").astype(np.uint64)


def model_codes(rows: np.ndarray, planes, nbits: int, thresholds=None) -> np.ndarray:
    """The codes of ``rows`` float32 [n, dim]; ``planes`` float32 [nbits, dim], or ``None`` for sign mode."""
    thr = np.zeros(nbits) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    if planes is not None:
        return pack(proj(np.asarray(planes, np.float32), rows) > thr[None, :])
    bits = np.zeros((rows.shape[0], nbits), bool)
    bits[:, :rows.shape[1]] = rows.astype(np.float64) > thr[None, :rows.shape[1]]
    return pack(bits)
