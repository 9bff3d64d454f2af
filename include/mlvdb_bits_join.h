/*
 * mlvdb_bits_join.h -- similarity join over a binary vector column (mlvdb_bits.h): which stored rows hold a code within a
 * Hamming or Jaccard radius of the codes of given stored rows -- the deduplication question of mlvdb_join.h, asked of bit
 * codes.  The left codes never leave the device (companion of mlvdb_bits_range.h and mlvdb_join.h, ABI version 7).
 *
 * The rule.  Left row i has label a = left_labels[i]; the labels ascend strictly and lie in [0, total).  The partners of a
 * are the hits mlvdb_range_batch_bits would return for the query "the stored code of row a" with this `words`, `metric`,
 * `radius` and `where` (NULL: every live row) and unlimited capacity, from which
 *     MLVDB_JOIN_OTHERS   the entry a itself is removed,
 *     MLVDB_JOIN_LATER    every entry with label <= a is removed: every unordered pair once.
 * The candidates (live rows, matched by `where`, with a present code of exactly `words` words), the integers, the one fp64
 * division of Jaccard, the test d <= radius, the order (distance, then label), out_dist = (float)d and the optional
 * out_dist64 are the range entry's own.  A left label that is not itself a live row holding a code of `words` words has no
 * partners (count 0); `where` restricts the partners, not the left rows.
 *
 * Outputs and statuses follow mlvdb_range_batch_bits: out_counts[i] is exact and always written, out_offsets (n_left + 1
 * entries) is always written, 1 <= capacity <= MLVDB_BITS_RANGE_MAX_HITS (above: MLVDB_ERR_UNSUPPORTED).  A left row with
 * more than `capacity` partners gets an EMPTY segment and its exact count, and the call returns MLVDB_ERR_OVERFLOW after
 * serving the others.  Segments that need more than total_capacity entries: out_counts and out_offsets are written, the
 * hit arrays are not, and the return is MLVDB_ERR_OVERFLOW.  total_capacity == 0 with NULL hit arrays is a counting call.
 * A NaN radius, labels that do not ascend strictly or lie outside [0, total), an unknown mode or metric, a column that is
 * not a bits column, words outside 1..MLVDB_BITS_MAX_WORDS, capacity < 1, n_left outside 0..2^24 and a bad program are
 * MLVDB_ERR_INVALID_ARG.  Everything is validated on the host before any launch; a refused call writes nothing.
 * n_left == 0 and an empty index succeed (out_offsets[0] = 0).
 */
#ifndef MLVDB_BITS_JOIN_H
#define MLVDB_BITS_JOIN_H

#include <stdint.h>

#include "mlvdb_bits_range.h"
#include "mlvdb_join.h"

#ifdef __cplusplus
extern "C" {
#endif

int mlvdb_join_within_bits(mlvdb_index* h, int32_t attr, const int64_t* left_labels, int64_t n_left, int32_t mode,
                           int32_t words, int32_t metric, double radius, int64_t capacity, int64_t total_capacity,
                           const mlvdb_where* where, int64_t* out_labels, float* out_dist, double* out_dist64,
                           int64_t* out_offsets, int64_t* out_counts);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_BITS_JOIN_H */
