/*
 * mlvdb_where_each_range.h -- per-query metadata filters in one batched range call (companion of mlvdb_where_each.h; the
 * ABI version of mlvdb_hip.h is unchanged).
 *
 * The programs, program_of_query and the routes are those of mlvdb_where_each.h; the outputs are the packed ones of
 * mlvdb_range_batch_packed.  Query i's hits (entries out_offsets[i] .. out_offsets[i + 1] of out_labels / out_dist) and its
 * out_counts[i] are bit-identical to what a call for that query alone returns with the same radius and capacity:
 * mlvdb_range_batch_packed_where with its program, or mlvdb_range_batch_packed for -1.  A hit is a live row matching the
 * query's program whose fp64 distance is <= (double)radius; hits come nearest first, ties by ascending label; the count is
 * exact even above `capacity`.
 *
 * Routes (out_routes, one per program):
 *   MLVDB_WHERE_ROUTE_NONE    no query uses the program, or it matches no live row: its queries get count 0
 *   MLVDB_WHERE_ROUTE_GATHER  few matching rows: the exact fp64 distances of just those rows, hits counted exactly and listed
 *                             in bounded space (MLVDB_WHERE_EACH_RANGE_LIST hits per query); a query with more hits than its
 *                             list holds is served by the SCAN route of its program instead
 *   MLVDB_WHERE_ROUTE_SCAN    otherwise: the masked range pass of mlvdb_range_batch_packed_where, once for the program's queries
 * GATHER is taken when matches * ceil(queries / 4) * 1000 <= live rows * WHERE_GATHER (the tuning key of mlvdb_where_each.h;
 * 0 = never gather).  The route changes the work, never the result.
 */
#ifndef MLVDB_WHERE_EACH_RANGE_H
#define MLVDB_WHERE_EACH_RANGE_H

#include <stdint.h>

#include "mlvdb_where_each.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_WHERE_EACH_RANGE_LIST 8192 /* hits per query the GATHER route lists (more: that query takes the SCAN route) */

/* Range search of nq queries with one radius, query i restricted to the rows programs[program_of_query[i]] matches (-1:
 * unrestricted).  Programs and program_of_query are validated as mlvdb_search_batch_where_each validates them, the range
 * arguments as mlvdb_range_batch_packed does, all before anything is launched (MLVDB_ERR_INVALID_ARG otherwise).
 * out_offsets ([nq + 1]) and out_counts ([nq]) are always written.  MLVDB_ERR_OVERFLOW when the hits need more than
 * total_capacity entries (out_labels / out_dist then hold nothing) or when some query has more hits than `capacity` (the
 * nearest `capacity` are returned); MLVDB_ERR_UNSUPPORTED when a query has more than MLVDB_MAX_TOPK_PAGED hits and more were
 * asked for; when several apply, in this order.  out_routes ([n_programs]) optional. */
int mlvdb_range_batch_packed_where_each(mlvdb_index* h, const float* queries, int64_t nq, float radius, int64_t capacity,
                                        int64_t total_capacity, const mlvdb_where* programs, int32_t n_programs,
                                        const int32_t* program_of_query, int64_t* out_labels, float* out_dist,
                                        int64_t* out_offsets, int64_t* out_counts, int32_t* out_routes);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_WHERE_EACH_RANGE_H */
