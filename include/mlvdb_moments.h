/*
 * mlvdb_moments.h -- the raw first and second moments of the stored rows, computed on the device: the row count, the column
 * sums and the Gram matrix X^T X in fp64 (companion of mlvdb_hip.h, ABI version 7).  No row crosses the bus; the column
 * means, the covariance, principal axes (PCA planes and thresholds for mlvdb_bits_project), whitening and a low-dimensional
 * map of a corpus all follow from these dim + dim * dim numbers on the host.
 *
 * Everything below is exact: a NumPy model reproduces a call bit for bit, and two calls return identical bytes.
 *
 * The candidates are the live rows `where` matches (NULL: every live row), as the fp32 values mlvdb_index_get_rows returns,
 * in all three spaces.  *out_count is their number.
 *
 * Order of summation.
 *     every product x[r][i] * x[r][j] is taken in fp64 (exact there);
 *     the rows are split into slabs of MLVDB_MOMENTS_SLAB consecutive labels: slab s holds the labels
 *         [s * MLVDB_MOMENTS_SLAB, (s + 1) * MLVDB_MOMENTS_SLAB);
 *     a slab's sum of an entry is one fp64 accumulator started at +0.0 that runs over the slab's candidate rows in
 *         ascending label, one rounded add per row;
 *     the entry is the fold of the slab sums in ascending slab order, from +0.0, one rounded add per slab;
 *     out_sums[i] follows the same rule with the term (double)x[r][i];
 *     a row that is no candidate contributes nothing (adding +0.0 for it gives the same bits).
 * out_gram is the full symmetric matrix, row-major [dim][dim]: [j][i] has the bits of [i][j].
 *
 * With no candidate the count is 0 and both arrays are all +0.0.
 *
 * The moments are raw, not centred: cov = (gram - count * mean * mean^T) / (count - 1) loses digits when the mean dwarfs
 * the spread.
 *
 * Refusals: a null handle, a null output or a bad program is MLVDB_ERR_INVALID_ARG; dim above MLVDB_MOMENTS_MAX_DIM is
 * MLVDB_ERR_UNSUPPORTED (the workspace is sized by one slab's tiles).  A refused call writes nothing and launches nothing.
 */
#ifndef MLVDB_MOMENTS_H
#define MLVDB_MOMENTS_H

#include <stdint.h>

#include "mlvdb_hip.h"
#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_MOMENTS_SLAB 4096
#define MLVDB_MOMENTS_MAX_DIM 4096

/* out_sums [dim], out_gram [dim][dim]; the host waits once, for the three outputs. */
int mlvdb_row_moments(mlvdb_index* h, const mlvdb_where* where, int64_t* out_count, double* out_sums, double* out_gram);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_MOMENTS_H */
