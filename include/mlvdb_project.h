/*
 * mlvdb_project.h -- bit codes computed from the stored rows on the device: SimHash / random-hyperplane signatures and
 * thresholded (sign) codes, written straight into a bits column (companion of mlvdb_bits.h, ABI version 7).  No row and no
 * code crosses the bus; the searches, joins and duplicate groups of the bits family then run on what this call wrote.
 *
 * Everything below is exact: a NumPy model reproduces a call bit for bit, and two calls return identical bytes.
 *
 * The projection.  For a plane p (fp32, dim values) and a stored fp32 row x (the values mlvdb_index_get_rows returns, in all
 * three spaces), proj(p, x) is the non-l2 dot product of the exact scans:
 *     every product p[c] * x[c] is taken in fp64 (exact there);
 *     four slice sums S_0 .. S_3, each one fp64 accumulator started at +0.0: S_g runs over the columns c with
 *         (c mod 16) div 4 == g in ascending c, one rounded add per column;
 *     proj = (S_0 + S_1) + (S_2 + S_3);
 *     the padding columns (dim up to dim rounded up to 16) contribute +0.0.
 *
 * The planes are the caller's: planes[nbits][dim] fp32, row-major, every value finite.  Like the random numbers of
 * mlvdb_kmeans_seed, the randomness is not the library's.
 *
 * The bits.  Bit j of a row's code is  proj(planes[j], x) > thresholds[j]  -- strict, so a NaN projection gives 0.
 * thresholds is [nbits] fp64, none NaN; NULL means 0.0 for every bit.
 *
 * Sign mode: planes == NULL.  Bit c is  (double)x[c] > thresholds[c]  for c < dim, the bits dim .. nbits - 1 are 0, and
 * nbits must be dim rounded up to 64.
 *
 * Width.  nbits is a multiple of 64 in [64, 64 * MLVDB_BITS_MAX_WORDS]; words = nbits / 64; bit b of a code is bit b & 63 of
 * word b >> 6 (mlvdb_bits.h).
 *
 * Refusals are MLVDB_ERR_INVALID_ARG and write nothing: a column that is not a bits column, nbits no multiple of 64 or out
 * of range, sign mode with another nbits, a non-finite plane value, a NaN threshold, a null output, a bad program.
 */
#ifndef MLVDB_PROJECT_H
#define MLVDB_PROJECT_H

#include <stdint.h>

#include "mlvdb_bits.h"
#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The candidates are the live rows `where` matches (NULL: every live row); the program is evaluated once, before anything is
 * written, so it may read `attr` itself through EXISTS.  Every candidate's slot in bits column `attr` becomes a fresh code of
 * `words` words; every other row, tombstoned ones included, keeps the slot it had.  *matched = the candidates.  The column
 * then reads exactly as if mlvdb_bits_set_at had written the same codes (mlvdb_bits_get, the searches, snapshots, compact,
 * reset).  Pool: a call with total > 0 takes total * words elements of the attribute's pool, row r's code at
 * (old used) + r * words and zeros for the rows that are no candidates; mlvdb_index_compact repacks. */
int mlvdb_bits_project(mlvdb_index* h, int32_t attr, const float* planes, int32_t nbits, const double* thresholds,
                       const mlvdb_where* where, int64_t* matched);
/* The same function of n given vectors ([n][dim] row-major, taken as they are): out_codes[n][words].  The codes of a query
 * then have the bits the stored codes have.  Computed on the device; 0 <= n <= 2^24, needs no stored row. */
int mlvdb_bits_project_vectors(mlvdb_index* h, const float* vectors, int64_t n, const float* planes, int32_t nbits,
                               const double* thresholds, uint64_t* out_codes);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_PROJECT_H */
