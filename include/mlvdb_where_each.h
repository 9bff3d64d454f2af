/*
 * mlvdb_where_each.h -- per-query metadata filters in one batched kNN call (companion of mlvdb_where.h; the ABI version of
 * mlvdb_hip.h is unchanged).
 *
 * A call carries a list of distinct predicate programs (mlvdb_where, each validated exactly as mlvdb_where.h says) and, per
 * query, the index of its program in that list or -1 for "unfiltered".  Query i's outputs (labels, fp32 and fp64 distances,
 * count) are bit-identical to what a call for that query alone returns: mlvdb_search_batch_where with its program, or
 * mlvdb_search_batch_ex without a mask for -1.  So out_counts[i] = min(k, live rows matching its program), padded with
 * label -1 / +inf as everywhere, ranked by (distance, label).
 *
 * One pass over the attribute columns evaluates every program of the call into one 64-bit word per row (bit p: live and
 * matching program p) and counts the matches per program; the counts come back to the host in one synchronisation and each
 * program takes one route (reported in out_routes when given):
 *   MLVDB_WHERE_ROUTE_NONE    no query uses the program, or it matches no live row: nothing is scanned, its queries padded
 *   MLVDB_WHERE_ROUTE_GATHER  k <= MLVDB_MAX_TOPK and few matching rows: the exact fp64 distances of just those rows
 *                             (a label list built on the device, gathered with the exact scan's arithmetic)
 *   MLVDB_WHERE_ROUTE_SCAN    otherwise: the masked kNN scan of mlvdb_search_batch_where, once for the program's queries
 * GATHER is taken when k <= MLVDB_MAX_TOPK and matches * ceil(queries / 4) * 1000 <= live rows * WHERE_GATHER (tuning key,
 * mlvdb_index_set_tuning "WHERE_GATHER=..."; 0 = never gather).  The route changes the work, never the result.
 */
#ifndef MLVDB_WHERE_EACH_H
#define MLVDB_WHERE_EACH_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_WHERE_EACH_MAX_PROGRAMS 64 /* distinct programs per call: one bit each in a per-row uint64 */
#define MLVDB_WHERE_EACH_MAX_OPS 1024    /* ops over all programs of one call (staged in LDS) */

/* routes (out_routes) */
#define MLVDB_WHERE_ROUTE_NONE 0
#define MLVDB_WHERE_ROUTE_SCAN 1
#define MLVDB_WHERE_ROUTE_GATHER 2

/* kNN of nq queries, query i restricted to the rows programs[program_of_query[i]] matches (-1: unrestricted).
 * 1 <= n_programs <= MLVDB_WHERE_EACH_MAX_PROGRAMS (0 when no query is filtered: programs may then be NULL), at most
 * MLVDB_WHERE_EACH_MAX_OPS ops over all programs, every program_of_query entry in [-1, n_programs); anything else is
 * MLVDB_ERR_INVALID_ARG before anything is launched.  k in 1..MLVDB_MAX_TOPK_PAGED.  out_dist64 and out_routes
 * ([n_programs]) optional. */
int mlvdb_search_batch_where_each(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const mlvdb_where* programs,
                                  int32_t n_programs, const int32_t* program_of_query, int64_t* out_labels, float* out_dist,
                                  int32_t* out_counts, double* out_dist64, int32_t* out_routes);
/* out_matches[p] = live rows programs[p] matches, for all programs in one pass over the columns. */
int mlvdb_where_count_each(mlvdb_index* h, const mlvdb_where* programs, int32_t n_programs, int64_t* out_matches);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_WHERE_EACH_H */
