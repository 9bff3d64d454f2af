/*
 * mlvdb_mutate.h -- the write side of the metadata columns: set values by label, update and delete rows by filter, on the
 * device (companion of mlvdb_where.h, ABI version 7).
 *
 * mlvdb_attr_set_at: values[j] -> row labels[j] of column `attr`.
 *   The host validates before anything is launched: the attribute is defined, every label lies in [0, total), no label
 *   appears twice (checked on a sorted copy: a duplicate would make the scatter a race).  Any violation is
 *   MLVDB_ERR_INVALID_ARG and nothing is written.  Tombstoned rows are skipped on the device; *updated = rows written.
 *   The sentinels (INT64_MIN / NaN) are values like any other, as in mlvdb_attr_set: writing one clears the row's value.
 *
 * mlvdb_attr_update_where: apply sets[0 .. n_sets) to every live row the program matches.
 *   1 <= n_sets <= MLVDB_MAX_ATTRS; each attribute appears at most once and must be defined; the program is validated as
 *   everywhere (mlvdb_where.h).  MLVDB_SET_ASSIGN stores `a` (float64 column: the bit pattern of the double; the absent
 *   sentinel clears the value).  MLVDB_SET_ADD adds `a` to the rows that hold a value (int64 column: an integer; float64
 *   column: the bit pattern of a double, NaN is refused on the host); absent rows stay absent.
 *   *matched = the live matching rows, whether or not they held a value for an ADD.
 *   A row's predicate and all of its assignments see the values from before the call: the program's columns and the
 *   assigned columns may be the same memory, each row is evaluated fully and then stored.
 *   An ADD result that cannot be stored -- an int64 sum that overflows or lands on INT64_MIN, a float64 sum that is NaN
 *   (inf + -inf) -- is never written, and the call is all or nothing: when any ADD is present, a first counting pass
 *   produces *refused = the live matching rows with an unstorable sum; if it is non-zero no column changes and the call
 *   still returns MLVDB_OK (the caller reads *refused).  With ASSIGNs only there is one pass and *refused = 0.
 *
 * mlvdb_tombstone_where: tombstone every live row the program matches; their labels ascending, as mlvdb_where_labels
 *   lists them.  Afterwards the handle is in exactly the state mlvdb_index_tombstone leaves when given those labels.
 *   capacity < *matches: nothing is tombstoned, *matches is exact and the return is MLVDB_OK -- the caller compares the two
 *   and calls again.  out_labels == NULL with capacity < 0: no labels wanted, tombstone and count only.
 */
#ifndef MLVDB_MUTATE_H
#define MLVDB_MUTATE_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_SET_ASSIGN 0 /* column := a */
#define MLVDB_SET_ADD 1    /* column += a for rows that hold a value */

typedef struct mlvdb_assign {
    int32_t attr;
    int32_t op;
    int64_t a;
} mlvdb_assign;

int mlvdb_attr_set_at(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, const void* values, int64_t* updated);

int mlvdb_attr_update_where(mlvdb_index* h, const mlvdb_where* where, const mlvdb_assign* sets, int32_t n_sets,
                            int64_t* matched, int64_t* refused);

int mlvdb_tombstone_where(mlvdb_index* h, const mlvdb_where* where, int64_t* out_labels, int64_t capacity, int64_t* matches);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_MUTATE_H */
