/*
 * mlvdb_list.h -- list-valued attribute columns: a set of int64 per row (tags, ACL groups, categories), filtered, written
 * and faceted on the device (companion of mlvdb_where.h, ABI version 7).
 *
 * Column type MLVDB_ATTR_INT64_LIST.  The column itself stays the 8-byte-per-row column every attribute has; for a list it
 * holds a slot,
 *     (offset << 8) | len        the row's list is pool[offset, offset + len), len <= MLVDB_LIST_MAX_LEN
 *     INT64_MIN                  the row has no list (absent)
 * and the attribute owns a value pool of int64 in HBM.  The values of one row are strictly ascending (sorted, unique: a
 * list is a set) and never INT64_MIN.  An empty list (len == 0) is a present value, distinct from absent.
 *
 * The pool is append-only and regrows by doubling: every write appends its lists and points the rows' slots at them, so
 * an overwritten list stays behind as garbage.  mlvdb_index_compact is the only place that reclaims it: after the slots
 * moved with their rows it repacks every pool (an exclusive scan of the live rows' lengths in the new row order gives the
 * new offsets, one pass copies the lists, the slots are rewritten), also when no row was tombstoned.  Lists are
 * immutable, so several rows may share one pool range (mlvdb_attr_list_update_where does that); the repack gives every
 * row a range of its own.  mlvdb_index_reset empties the pools and keeps the definitions.
 *
 * Slots cannot be forged: mlvdb_attr_set, mlvdb_attr_get, mlvdb_attr_set_at and mlvdb_attr_update_where refuse a list
 * column, and every entry that needs a scalar column (distinct, grouped, maxsim `by`, mlvdb_where_ordered,
 * mlvdb_facet_values, mlvdb_facet_bins) refuses it too.
 *
 * Predicate ops (valid on list columns only; EQ..GE and IN are refused on them, EXISTS reads the slot as it is):
 *   HAS       push: the row's list contains a
 *   HAS_ANY   push: the row's list intersects set[a, a + b)   (the range sorted ascending; b == 0 matches nothing)
 *   HAS_ALL   push: the row's list holds every value of set[a, a + b)   (the range strictly ascending, b >= 1)
 *   LEN       push: a <= len <= b
 * An absent row makes all four false.  a and b of a set range must each be below 2^31.
 *
 * Everything is validated on the host before any launch; a refusal is MLVDB_ERR_INVALID_ARG and writes nothing.
 */
#ifndef MLVDB_LIST_H
#define MLVDB_LIST_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_ATTR_INT64_LIST 3 /* accepted by mlvdb_attr_define */
#define MLVDB_LIST_MAX_LEN 255

#define MLVDB_WHERE_HAS 12
#define MLVDB_WHERE_HAS_ANY 13
#define MLVDB_WHERE_HAS_ALL 14
#define MLVDB_WHERE_LEN 15

/* Lists of rows [first, first + n) in CSR form: row first + i gets values[offsets[i], offsets[i + 1]) (offsets[0] >= 0).
 * present (n bytes, or NULL: all present): 0 makes the row absent, and its range must be empty.  Refused: offsets that
 * decrease, a list longer than MLVDB_LIST_MAX_LEN, a list that is not strictly ascending, an INT64_MIN element. */
int mlvdb_attr_list_set(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, const int64_t* offsets,
                        const int64_t* values, const uint8_t* present);
/* The list sibling of mlvdb_attr_set_at: list i -> row labels[i].  Labels inside [0, total), none twice; tombstoned rows
 * are skipped on the device, *updated = rows written. */
int mlvdb_attr_list_set_at(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, const int64_t* offsets,
                           const int64_t* values, const uint8_t* present, int64_t* updated);
/* Lists of rows [first, first + n) (tombstoned rows included: they keep what they hold) as CSR with out_offsets[0] == 0.
 * *needed = their number of values, always exact; capacity < *needed: nothing else is written and the return is
 * MLVDB_OK -- the caller compares the two and calls again.  out_present (n bytes, may be NULL): 0 for an absent row. */
int mlvdb_attr_list_get(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int64_t* out_offsets, int64_t* out_values,
                        uint8_t* out_present, int64_t capacity, int64_t* needed);
/* Every live row the program matches gets this one list (clear != 0: becomes absent; values is ignored).  The list is
 * appended to the pool once and the rows share its slot.  The program may read the column it assigns: a row is evaluated
 * fully before it is stored.  *matched = the live matching rows. */
int mlvdb_attr_list_update_where(mlvdb_index* h, const mlvdb_where* where, int32_t attr, const int64_t* values,
                                 int32_t n_values, int32_t clear, int64_t* matched);
/* *pool_used = values allocated in the attribute's pool, *pool_live = the sum of the lengths of the live rows' lists. */
int mlvdb_attr_list_stats(mlvdb_index* h, int32_t attr, int64_t* pool_used, int64_t* pool_live);
/* mlvdb_facet_values of a list column: out_counts[v] = live matching rows whose list holds out_values[v] (ascending
 * values, the same max_values / MLVDB_ERR_OVERFLOW rule).  *absent = matching rows that contribute no value (an absent or
 * an empty list).  A row counts under every value it holds, so sum(out_counts) + *absent == *matched does NOT hold here. */
int mlvdb_facet_list_values(mlvdb_index* h, int32_t attr, const mlvdb_where* where, int64_t max_values, int64_t* out_values,
                            int64_t* out_counts, int64_t* n_values, int64_t* matched, int64_t* absent);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_LIST_H */
