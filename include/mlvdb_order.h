/*
 * mlvdb_order.h -- ordered metadata queries: the top rows by an attribute column, ranked on the device (companion of
 * mlvdb_where.h; the ABI version of mlvdb_hip.h is unchanged).
 *
 * The candidates of a call are the live rows -- those the optional `where` program matches, when one is given (where ==
 * NULL: every live row; otherwise validated and meant exactly as in mlvdb_where_count) -- that hold a present value of
 * `attr` (not INT64_MIN on an int64 column, not NaN on a float64 one).  Tombstoned rows never count.  Per call:
 *   *matched = the live matching rows (= mlvdb_where_count of the same program, or the live count),
 *   *absent  = those of them whose value of `attr` is absent; they are never ranked,
 *   candidates = *matched - *absent.
 * The ranking is a total order: by value (int64 columns compare as integers, never through double; float64 columns as IEEE
 * doubles, so -0.0 and 0.0 tie and +-inf are ordinary values), ascending or -- descending != 0 -- descending, and rows of
 * equal value by ascending label in both directions.  The answer is therefore unique and two calls return identical arrays.
 * Everything is validated on the host before anything is launched; an index without rows answers zeros and launches nothing.
 */
#ifndef MLVDB_ORDER_H
#define MLVDB_ORDER_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_ORDER_MAX_ROWS 4096

/* Ranks [offset, offset + limit) of the candidates by column `attr` (int64 or float64; an undefined column is
 * MLVDB_ERR_INVALID_ARG): *n_out = clamp(candidates - offset, 0, limit) rows, their labels in out_labels[0 .. *n_out) and
 * their stored values, bit for bit (a stored -0.0 comes back as -0.0), in out_values[0 .. *n_out) -- int64_t or double by the
 * column's type.  Both buffers hold `limit` entries; entries beyond *n_out are unspecified.  offset >= 0, limit >= 1 and
 * offset + limit <= MLVDB_ORDER_MAX_ROWS, no pointer but `where` may be null -- anything else is MLVDB_ERR_INVALID_ARG.  The
 * device workspaces are sized by MLVDB_ORDER_MAX_ROWS and the selection's histograms, never by the corpus (a program is
 * evaluated into the one-byte row mask the filtered searches use); only the *n_out results and the scalars leave the device. */
int mlvdb_where_ordered(mlvdb_index* h, int32_t attr, int32_t descending, const mlvdb_where* where, int64_t offset,
                        int64_t limit, int64_t* out_labels, void* out_values, int64_t* n_out, int64_t* matched,
                        int64_t* absent);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_ORDER_H */
