/*
 * mlvdb_transform.h -- linear maps of the stored rows on the device: value = matrix . row - shift, as fp32 rows of out_dim
 * columns, appended to another index or copied down (companion of mlvdb_hip.h and mlvdb_project.h, ABI version 7).  A PCA
 * reduction, a whitening, a rotation or a 2-D map of the corpus with no stored row crossing the bus.
 *
 * Everything below is exact: a NumPy model reproduces a call byte for byte, and two calls return identical bytes.
 *
 * The value.  For row x_i (the fp32 values mlvdb_index_get_rows returns, in all three spaces) and output column j
 *     value[i][j] = (float)(proj(matrix[j], x_i) - shift[j])
 * where proj is exactly the projection of mlvdb_project.h (four slice sums, columns ascending, (S_0 + S_1) + (S_2 + S_3),
 * padding columns contribute +0.0), followed by one rounded fp64 subtract and one round-to-nearest-even conversion to fp32.
 * mlvdb_bits_project with planes = M, thresholds = t and a transform with M, shift = t therefore agree: bit j is set exactly
 * where the value before the conversion is > 0.
 *
 * matrix is [out_dim][dim] fp32, row-major, every value finite; shift is [out_dim] fp64, none NaN or infinite, NULL meaning
 * 0.0; out_dim is in 1 .. MLVDB_TRANSFORM_MAX_OUT.
 *
 * Refusals write nothing, append nothing and leave both handles as they were.  MLVDB_ERR_INVALID_ARG: a null handle, dst == h,
 * dst on another device, dst's dim != out_dim, a non-finite matrix or shift value, a bad program, neither sink, a null
 * `matched`, and a transformed value that is not finite in fp32 ("transform: a transformed value is not finite": found by the
 * kernel, read before anything is appended or copied).  MLVDB_ERR_UNSUPPORTED: out_dim out of range.  MLVDB_ERR_OVERFLOW:
 * matched > capacity with a host output (*matched is set).  MLVDB_ERR_OUT_OF_MEMORY: the result (matched * out_dim * 4 B, one
 * temporary device buffer of the call) cannot be allocated.
 */
#ifndef MLVDB_TRANSFORM_H
#define MLVDB_TRANSFORM_H

#include <stdint.h>

#include "mlvdb_hip.h"
#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_TRANSFORM_MAX_OUT 4096

/* The candidates are the live rows `where` matches (NULL: every live row), processed in ascending label; *matched = their
 * number.  Sinks, at least one of them:
 *   dst != NULL       the matched transformed rows are appended to dst as its labels *first_label .. *first_label + matched - 1
 *                     in candidate order, through the steps of mlvdb_index_append_device -- scatter, norms, shadow, row
 *                     statistics: dst then behaves as if the rows had been appended from the host.  One append, at the end.
 *   out_rows != NULL  the same rows, [matched][out_dim]; out_labels (optional) the candidates' labels, ascending.  `capacity`
 *                     is the room of both in rows.
 * first_label is optional and written only with a dst. */
int mlvdb_rows_transform(mlvdb_index* h, const float* matrix, int32_t out_dim, const double* shift,
                         const mlvdb_where* where, mlvdb_index* dst, int64_t capacity,
                         float* out_rows, int64_t* out_labels, int64_t* matched, int64_t* first_label);
/* The same function of n given vectors ([n][dim] row-major, taken as they are): out[n][out_dim].  A stored row, transformed
 * as a query, is the image the stored row got.  Computed on the device; 0 <= n <= 2^24, needs no stored row; a non-finite
 * result is refused the same way and nothing is written. */
int mlvdb_rows_transform_vectors(mlvdb_index* h, const float* vectors, int64_t n, const float* matrix,
                                 int32_t out_dim, const double* shift, float* out);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_TRANSFORM_H */
