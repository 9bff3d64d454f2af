/*
 * mlvdb_grouped.h -- grouped kNN: the nearest rows of each of the k nearest groups (companion of mlvdb_distinct.h; the ABI
 * version of mlvdb_hip.h is unchanged).
 *
 * Groups, liveness, `where`, max_groups, absent values and the canonical order (fp64 distance, label) are exactly those of
 * mlvdb_search_batch_distinct: the groups of a query and their ranking are those of that call with the same arguments, and
 * slot [i, j, 0] is its [i, j], bit for bit.  Per query i and returned group j:
 *   slots [i, j, 0 .. c) are the c = min(group_size, live allowed rows of group j) nearest rows of the group, in canonical
 *   order; out_group_counts[i, j] = c.
 * The tail of every group and every group beyond out_counts[i] is padded with label -1 / +inf (out_groups: INT64_MIN,
 * out_group_counts: 0).  Every returned distance has the bits mlvdb_pair_distances gives the pair, fp64 and fp32.
 * group_size == 1 equals mlvdb_search_batch_distinct; a column in which every row holds its own value equals
 * mlvdb_search_batch_ex in slot 0 of every group, both bit for bit.
 *
 * The groups come from the distinct stage (both of its routes, tuning key DISTINCT_OVERSAMPLE; mlvdb_stats.fallback_queries
 * keeps that stage's meaning).  The member stage has one route: the rows of the picked groups are listed by two passes over
 * the attribute column, and each list is scored against exactly the queries that picked its group.
 */
#ifndef MLVDB_GROUPED_H
#define MLVDB_GROUPED_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_GROUPED_MAX_SIZE 64 /* rows returned per group: one selection list of a wavefront */

/* 1 <= k <= MLVDB_MAX_TOPK and 1 <= group_size <= MLVDB_GROUPED_MAX_SIZE (larger: MLVDB_ERR_UNSUPPORTED).  attr, max_groups
 * and where: as in mlvdb_search_batch_distinct.  out_labels / out_dist: [nq, k, group_size]; out_counts: [nq] groups
 * returned; out_group_counts: [nq, k] rows returned per group; out_dist64 ([nq, k, group_size]) and out_groups ([nq, k]
 * group codes) are optional.  An undefined or float64 attr, a bad program, nq < 0, group_size < 1 or a null required buffer
 * is MLVDB_ERR_INVALID_ARG before anything is launched.  An empty or fully tombstoned index answers padding and launches
 * nothing. */
int mlvdb_search_batch_grouped(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t group_size,
                               int32_t attr, int64_t max_groups, const mlvdb_where* where, int64_t* out_labels,
                               float* out_dist, int32_t* out_counts, int32_t* out_group_counts, double* out_dist64,
                               int64_t* out_groups);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_GROUPED_H */
