/*
 * mlvdb_where.h -- metadata filters evaluated on the device (companion of mlvdb_hip.h, ABI version 7).
 *
 * Attribute columns: up to MLVDB_MAX_ATTRS typed columns per index, one value per row, held in HBM next to the rows.
 * They follow every change of the rows: appended rows start absent, capacity regrowth copies them,
 * mlvdb_index_compact gathers them with the rows, mlvdb_index_reset drops their values (definitions stay).
 *
 * Absent values are sentinels (no bitmap):
 *   MLVDB_ATTR_INT64    INT64_MIN
 *   MLVDB_ATTR_FLOAT64  NaN
 * (a third type, MLVDB_ATTR_INT64_LIST = 3, a set of int64 per row with ops of its own, lives in mlvdb_list.h)
 * (and a fourth, MLVDB_ATTR_SPARSE = 4, a sparse vector per row in the same storage, in mlvdb_sparse.h)
 * (and a fifth, MLVDB_ATTR_GEO = 5, a location per row stored as an int64 with ops of its own, in mlvdb_geo.h)
 * (and a sixth, MLVDB_ATTR_BITS = 6, a bit code per row in the list column's storage, in mlvdb_bits.h)
 * so mlvdb_attr_set stores either as "absent" (which is how a caller clears a value); a caller whose data may hold
 * INT64_MIN as a real value must refuse it at ingest (the Python Index does).
 *
 * Predicate program: postfix, at most MLVDB_WHERE_MAX_OPS ops over a boolean stack of depth <= MLVDB_WHERE_MAX_DEPTH.
 *   TRUE                 push true
 *   EQ NE LT LE GT GE    push (row's value of `attr`) <op> a;  float64 columns: a holds the bit pattern of the double
 *   IN                   push: the row's int64 value is in set[a .. a + b) (a range of the set table, sorted ascending)
 *   EXISTS               push: the row has a value for `attr`
 *   AND OR               pop two, push the result
 *   NOT                  flip the top
 * Semantics on an absent value: every comparison, EQ and IN is false; NE is NOT EQ, so an absent value matches NE.
 * A row matches when the program leaves true; tombstoned rows never match.
 *
 * Every program is validated on the host before anything is launched (stack depth never below 1 and exactly 1 at
 * the end, attributes defined, each op valid for its column's type -- LT..GE, EQ, NE on both types, IN on int64 only
 * --, set ranges inside the table and sorted): a refused program is MLVDB_ERR_INVALID_ARG, never a device fault.
 * The row mask a program evaluates to stays on the device; the masked kNN and range entries consume it exactly as
 * mlvdb_search_batch_ex consumes a host mask (a masked-out row looks tombstoned to every kernel of the call).
 */
#ifndef MLVDB_WHERE_H
#define MLVDB_WHERE_H

#include <stdint.h>

#include "mlvdb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_MAX_ATTRS 16
#define MLVDB_WHERE_MAX_OPS 64
#define MLVDB_WHERE_MAX_DEPTH 32

/* column types */
#define MLVDB_ATTR_INT64 1
#define MLVDB_ATTR_FLOAT64 2

/* ops */
#define MLVDB_WHERE_TRUE 0
#define MLVDB_WHERE_EQ 1
#define MLVDB_WHERE_NE 2
#define MLVDB_WHERE_LT 3
#define MLVDB_WHERE_LE 4
#define MLVDB_WHERE_GT 5
#define MLVDB_WHERE_GE 6
#define MLVDB_WHERE_IN 7
#define MLVDB_WHERE_EXISTS 8
#define MLVDB_WHERE_AND 9
#define MLVDB_WHERE_OR 10
#define MLVDB_WHERE_NOT 11

typedef struct mlvdb_where_op {
    int32_t op;
    int32_t attr;
    int64_t a;
    int64_t b;
} mlvdb_where_op;

typedef struct mlvdb_where {
    const mlvdb_where_op* ops;
    int32_t n_ops;
    const int64_t* set; /* int64 values the IN ops index into, each op's range sorted (may be NULL when n_set == 0) */
    int64_t n_set;
} mlvdb_where;

/* Define column `attr` (0..MLVDB_MAX_ATTRS-1) with `type`, every row absent.  Redefining with the same type keeps
 * the values; another type is MLVDB_ERR_INVALID_ARG. */
int mlvdb_attr_define(mlvdb_index* h, int32_t attr, int32_t type);
/* Values of rows [first, first + n) (host, n int64 or double values by the column's type). */
int mlvdb_attr_set(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, const void* values);
int mlvdb_attr_get(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, void* out_values);

/* Number of live rows the program matches. */
int mlvdb_where_count(mlvdb_index* h, const mlvdb_where* where, int64_t* matches);
/* Ascending labels of the live matching rows: the first min(capacity, matches) of them; *matches always exact. */
int mlvdb_where_labels(mlvdb_index* h, const mlvdb_where* where, int64_t* out_labels, int64_t capacity, int64_t* matches);
/* mlvdb_search_batch_ex restricted to the rows the program matches: the same labels and fp64 distances as
 * mlvdb_search_batch_ex given the host-built mask of the same predicate; out_counts[i] = min(k, matching live rows),
 * padded as there.  out_dist64 optional. */
int mlvdb_search_batch_where(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const mlvdb_where* where,
                             int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_dist64);
/* mlvdb_range_batch_packed restricted to the rows the program matches. */
int mlvdb_range_batch_packed_where(mlvdb_index* h, const float* queries, int64_t nq, float radius, int64_t capacity,
                                   int64_t total_capacity, const mlvdb_where* where, int64_t* out_labels, float* out_dist,
                                   int64_t* out_offsets, int64_t* out_counts);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_WHERE_H */
