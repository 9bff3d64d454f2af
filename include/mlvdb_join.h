/*
 * mlvdb_join.h -- similarity join: which stored rows lie within a radius of given stored rows.  The queries are rows the
 * index already holds, gathered on the device; a row never meets itself and, in the LATER mode, every unordered pair is
 * reported once (companion of mlvdb_where.h; the ABI version of mlvdb_hip.h is unchanged).
 *
 * The rule.  Left row i has label a = left_labels[i]; the labels are strictly ascending and lie in [0, total).  A tombstoned
 * label is a valid left row -- its values are still stored, as for mlvdb_pair_distances and mlvdb_search_batch_like.  The
 * partners of left row i are the entries mlvdb_range_batch_packed_where would return for the query "the stored fp32 values
 * of row a" at this radius and this `where` (NULL: every live row) with unlimited capacity, from which
 *     MLVDB_JOIN_OTHERS   the entry a itself is removed,
 *     MLVDB_JOIN_LATER    every entry with label <= a is removed.
 * The order (fp64 distance, then label), the tie rule, the test dist <= radius on the fp64 distance against
 * (double)(float)radius and the fp32 bits of out_dist are the range search's own: the row's values go through the ordinary
 * query preparation, so they get the bits a copy of the row sent from the host would get.
 *
 * The outputs are packed like those of mlvdb_range_batch_packed: out_counts[i] is the exact number of partners of left row
 * i, also above `capacity`; the row returns its nearest min(count, capacity) partners as entries out_offsets[i] ..
 * out_offsets[i + 1] - 1 of out_labels / out_dist (total_capacity entries each).  out_offsets ([n_left + 1]) and out_counts
 * are always written.  total_capacity == 0 with NULL hit arrays is a counting call.
 */
#ifndef MLVDB_JOIN_H
#define MLVDB_JOIN_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_JOIN_OTHERS 0 /* partners of a: every live matching row b != a */
#define MLVDB_JOIN_LATER 1  /* partners of a: only b > a -- every unordered pair once */
#define MLVDB_JOIN_MAX_CAPACITY (MLVDB_MAX_TOPK_PAGED - 256)

/* Statuses.  MLVDB_ERR_OVERFLOW: the hits need more than total_capacity entries (out_counts / out_offsets hold the exact
 * counts and the layout the hits need, the hit arrays nothing), or a row has more partners than `capacity` (its nearest
 * `capacity` are returned).  MLVDB_ERR_UNSUPPORTED: capacity > MLVDB_JOIN_MAX_CAPACITY.  MLVDB_ERR_INVALID_ARG: labels
 * that do not ascend strictly or lie outside [0, total), an unknown mode, capacity < 1, total_capacity < 0, n_left < 0, a
 * null required buffer (left_labels, out_offsets, out_counts; out_labels and out_dist unless total_capacity == 0), a bad
 * program.  Everything is checked on the host before anything is launched; a refused call writes nothing.
 * n_left == 0 and an empty index succeed (out_offsets[0] = 0).  mlvdb_index_last_stats reports the range passes of the
 * (last wave of the) call. */
int mlvdb_join_within(mlvdb_index* h, const int64_t* left_labels, int64_t n_left, int32_t mode, float radius,
                      int64_t capacity, int64_t total_capacity, const mlvdb_where* where, int64_t* out_labels,
                      float* out_dist, int64_t* out_offsets, int64_t* out_counts);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_JOIN_H */
