/*
 * mlvdb_distinct.h -- distinct-by-attribute kNN: the nearest row of each of the k nearest groups (companion of mlvdb_where.h;
 * the ABI version of mlvdb_hip.h is unchanged).
 *
 * A group is one present value of an int64 attribute column (a float64 column is refused).  Among the live rows -- those the
 * optional `where` program matches, when one is given -- a group's representative is its best row by (fp64 distance, label),
 * the canonical order of this library, and the groups are ranked by their representatives in that same order.  Rows whose
 * value is absent (INT64_MIN) belong to no group and are never returned.  Per query:
 *   out_counts[i] = min(k, distinct present values among the live allowed rows); the tail is padded with label -1 / +inf
 *   (out_groups: INT64_MIN), as everywhere.
 * Distances are the exact scan's: a returned (query, label) pair has the bits mlvdb_pair_distances gives it, fp64 and fp32.
 * A column in which every row holds its own value makes the call equal to mlvdb_search_batch_ex, bit for bit.
 *
 * Two routes, one answer.  The list pass runs the plain device search for L = min(1024, max(64, DISTINCT_OVERSAMPLE x k))
 * neighbours per query and keeps the first entry of each group in rank order; a query is finished when k groups were kept
 * or the list held every live allowed row.  The others -- counted in mlvdb_stats.fallback_queries -- take a fused exact
 * scan whose selection lists hold one row per group.  Tuning key DISTINCT_OVERSAMPLE (mlvdb_index_set_tuning, default 4):
 * 0 skips the list pass, so every query takes the grouped scan.  The route changes the work, never the result.
 */
#ifndef MLVDB_DISTINCT_H
#define MLVDB_DISTINCT_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The k nearest groups of attribute column `attr` for nq queries.  1 <= k <= MLVDB_MAX_TOPK (larger: MLVDB_ERR_UNSUPPORTED).
 * max_groups: the caller's upper bound on the number of distinct present values of the column, 0 = unknown; it only lets a
 * query stop early (at most min(k, max_groups) groups are returned), a bound that is too small is the caller's error.
 * where: NULL, or one program restricting the rows first -- validated and applied exactly as in mlvdb_search_batch_where.
 * out_dist64 ([nq, k]) and out_groups ([nq, k] group codes of the hits) are optional.  An undefined or float64 attr, a bad
 * program, nq < 0 or a null buffer is MLVDB_ERR_INVALID_ARG before anything is launched. */
int mlvdb_search_batch_distinct(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t attr,
                                int64_t max_groups, const mlvdb_where* where, int64_t* out_labels, float* out_dist,
                                int32_t* out_counts, double* out_dist64, int64_t* out_groups);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_DISTINCT_H */
