/*
 * mlvdb_bits_range.h -- range search over a binary vector column (mlvdb_bits.h): every row within a Hamming or Jaccard
 * radius of each code of a batch, with exact counts, packed like the hits of mlvdb_range_batch_packed (companion of
 * mlvdb_bits.h, ABI version 7).
 *
 * Everything is validated on the host before any launch; a refusal is MLVDB_ERR_INVALID_ARG (MLVDB_ERR_UNSUPPORTED for a
 * capacity above the limit) and writes nothing.
 */
#ifndef MLVDB_BITS_RANGE_H
#define MLVDB_BITS_RANGE_H

#include <stdint.h>

#include "mlvdb_bits.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_BITS_RANGE_MAX_HITS 16384 /* per query: what one workgroup sorts in LDS */

/* Query i is queries[i * words .. (i + 1) * words).  Candidates and distances are those of mlvdb_search_batch_bits: the live
 * rows with a present code of exactly `words` words that `where` (may be NULL) matches; d = popcount(q ^ x) for
 * MLVDB_BITS_HAMMING, the one fp64 division (u - i) / u (0.0 when u == 0) for MLVDB_BITS_JACCARD.  A row is a hit iff
 * d <= radius, compared on that fp64 value: a negative radius gives no hits, a NaN radius is refused.  0 <= nq <= 2^24.
 *
 * out_counts[i] = the exact number of hits of query i, always written.  out_offsets (nq + 1 entries) is always written:
 * query i's segment is entries out_offsets[i] .. out_offsets[i + 1] of out_labels / out_dist / out_dist64, its hits ranked
 * by (distance ascending, label ascending); out_dist = (float)d, out_dist64 (may be NULL) the fp64 distances;
 * out_offsets[nq] = the entries the segments need.  total_capacity = the entries the three arrays hold; 0 with NULL arrays
 * is a counting call.
 *
 * 1 <= capacity <= MLVDB_BITS_RANGE_MAX_HITS (above: MLVDB_ERR_UNSUPPORTED).  A query with more than `capacity` hits gets an
 * EMPTY segment and its exact count, and the call returns MLVDB_ERR_OVERFLOW after serving the other queries.  Segments that
 * need more than total_capacity entries: out_counts and out_offsets are written, out_labels / out_dist / out_dist64 are not,
 * and the return is MLVDB_ERR_OVERFLOW. */
int mlvdb_range_batch_bits(mlvdb_index* h, int32_t attr, const uint64_t* queries, int64_t nq, int32_t words, int32_t metric,
                           double radius, int64_t capacity, int64_t total_capacity, const mlvdb_where* where,
                           int64_t* out_labels, float* out_dist, double* out_dist64, int64_t* out_offsets,
                           int64_t* out_counts);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_BITS_RANGE_H */
