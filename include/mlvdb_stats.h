/*
 * mlvdb_stats.h -- min, max, sum and count of an attribute column, per group of a second column, aggregated on the device
 * (companion of mlvdb_facet.h; the ABI version of mlvdb_hip.h is unchanged).
 *
 * The entry summarises column `attr` over the live rows -- those the optional `where` program matches, when one is given
 * (where == NULL: every live row; otherwise validated and meant exactly as in mlvdb_where_count).  Tombstoned rows never
 * count.  Per call:
 *   *matched   = the live matching rows (= mlvdb_where_count of the same program, or the live count),
 *   *by_absent = those of them with no value of `by` (0 when ungrouped),
 *   sum(out_rows) + *by_absent == *matched.
 * Everything is validated on the host before anything is launched; an index without rows answers zeros and launches
 * nothing.  Every number is accumulated by integer atomics whose result does not depend on the order in which they land:
 * two calls over the same index return identical bytes.
 */
#ifndef MLVDB_STATS_H
#define MLVDB_STATS_H

#include <stdint.h>

#include "mlvdb_facet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Statistics of scalar column `attr` (int64 or float64; a list, sparse, geo or undefined column is MLVDB_ERR_INVALID_ARG)
 * per distinct present value of int64 column `by` (as in mlvdb_facet_values: a float64, list, sparse, geo or undefined column
 * is MLVDB_ERR_INVALID_ARG), or over all matching rows as one group when by == -1: then out_keys[0] = 0 and *n_groups = 1
 * even when nothing matches.  1 <= max_groups <= MLVDB_FACET_MAX_VALUES; every array holds max_groups entries.
 *
 * Groups come back ascending by key in [0, *n_groups).  Per group:
 *   out_rows  = its live matching rows,
 *   out_count = those of them with a present value of `attr` (not INT64_MIN / NaN),
 *   out_min / out_max = the least and greatest present value, int64_t or double by the column's own type; unspecified when
 *     out_count is 0,
 *   out_sum_hi:out_sum_lo = a signed 128-bit integer, below.
 *
 * int64 columns: hi:lo is the exact sum of the present values; min / max compare as integers.
 *
 * float64 columns: min / max follow IEEE totalOrder on the present values (-0.0 below +0.0, +-inf ordinary values, NaN is
 * absent), so they are a function of the set of values.  hi:lo is the fixed-point sum S: let m be the largest finite |v| of
 * the group.  If m is 0 or the group holds an infinity, S = 0.  Otherwise E = floor(log2 m) (subnormals included) and
 *   S = sum of rint(v * 2^(61 - E)), rounding half to even, over the finite present values.
 * The scaling is exact, so each term is one rounding of a real number; |term| <= 2^62 and an index holds fewer than 2^31
 * rows, so |S| < 2^93.  The caller turns S into a double from out_min / out_max alone: NaN if the group holds both
 * infinities (min == -inf and max == +inf), that infinity if it holds one, otherwise S * 2^(E - 61) rounded once to double
 * (m = max(|min|, |max|); overflow gives +-inf, as IEEE addition would).  Consequences:
 *   |sum - true sum| <= count * 2^(E - 62), plus the final rounding;
 *   the sum is the correctly rounded true sum whenever every value lies within a factor 2^9 of m (every term is then exact).
 *
 * More than max_groups distinct values of `by` is MLVDB_ERR_OVERFLOW: *matched and *by_absent are still exact,
 * *n_groups > max_groups, the arrays are unspecified (exactly max_groups groups is success).  The device workspaces are
 * sized by max_groups, never by the corpus. */
int mlvdb_attr_stats(mlvdb_index* h, int32_t attr, int32_t by, const mlvdb_where* where, int64_t max_groups,
                     int64_t* out_keys, int64_t* out_rows, int64_t* out_count, void* out_min, void* out_max,
                     int64_t* out_sum_hi, uint64_t* out_sum_lo, int64_t* n_groups, int64_t* matched, int64_t* by_absent);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_STATS_H */
