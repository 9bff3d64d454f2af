/*
 * mlvdb_facet.h -- facet counts and histograms of attribute columns, aggregated on the device (companion of mlvdb_where.h;
 * the ABI version of mlvdb_hip.h is unchanged).
 *
 * Both entries count over the live rows -- those the optional `where` program matches, when one is given (where == NULL:
 * every live row; otherwise validated and meant exactly as in mlvdb_where_count).  Tombstoned rows never count.  Per call:
 *   *matched = the live matching rows (= mlvdb_where_count of the same program, or the live count),
 *   *absent  = those of them whose value of `attr` is absent (INT64_MIN / NaN),
 *   sum(out_counts) + *absent == *matched.
 * Everything is validated on the host before anything is launched; an index without rows answers all zeros and launches
 * nothing.  The counts are integers accumulated by atomics: two calls over the same index return identical arrays.
 */
#ifndef MLVDB_FACET_H
#define MLVDB_FACET_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_FACET_MAX_VALUES (1 << 20)
#define MLVDB_FACET_MAX_EDGES 4096

/* Value facets of int64 column `attr` (a float64 or undefined column is MLVDB_ERR_INVALID_ARG): the distinct present values
 * among the live matching rows, ascending, in out_values[0 .. *n_values) and the number of rows holding each in out_counts.
 * 1 <= max_values <= MLVDB_FACET_MAX_VALUES; both buffers hold max_values entries.  More than max_values distinct values is
 * MLVDB_ERR_OVERFLOW: *matched and *absent are still exact, *n_values > max_values, the arrays are unspecified (exactly
 * max_values distinct values is success).  The device workspaces are sized by max_values, never by the corpus. */
int mlvdb_facet_values(mlvdb_index* h, int32_t attr, const mlvdb_where* where, int64_t max_values, int64_t* out_values,
                       int64_t* out_counts, int64_t* n_values, int64_t* matched, int64_t* absent);

/* Histogram of column `attr` (int64 or float64) over `n_edges` bin edges of the column's own type (int64_t or double),
 * 1 <= n_edges <= MLVDB_FACET_MAX_EDGES, strictly ascending; float64 edges must not be NaN (+-inf is allowed), int64 edges
 * must not be INT64_MIN -- anything else is MLVDB_ERR_INVALID_ARG.  out_counts[i] (n_edges + 1 entries) = the live matching
 * rows with a present value v such that the number of edges <= v is i: slot 0 lies below the first edge, slot n_edges at or
 * above the last, a value equal to an edge belongs to the bin that edge opens (np.searchsorted(edges, v, side="right")).
 * int64 columns compare as integers, never through double; on float64 columns -0.0 == 0.0 and +-inf are ordinary values. */
int mlvdb_facet_bins(mlvdb_index* h, int32_t attr, const mlvdb_where* where, const void* edges, int32_t n_edges,
                     int64_t* out_counts, int64_t* matched, int64_t* absent);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_FACET_H */
