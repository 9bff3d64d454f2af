/*
 * mlvdb_sparse.h -- sparse vector columns: a bag of (term, weight) pairs per row (SPLADE / BM25-style lexical vectors), and
 * the exact top-k inner product of a batch of sparse queries against them on the device (companion of mlvdb_list.h, ABI
 * version 7).
 *
 * Column type MLVDB_ATTR_SPARSE.  It shares the list column's storage (mlvdb_list.h): the 8-byte column value is the slot
 *     (offset << 8) | len        the row's vector is pool[offset, offset + len), len <= MLVDB_SPARSE_MAX_NNZ
 *     INT64_MIN                  the row has no vector (absent)
 * into the attribute's append-only int64 pool, and a pool element is
 *     ((int64)term << 32) | bits(weight)        term in [0, 2^31), weight a finite fp32
 * with the terms of a row strictly ascending -- so the elements are strictly ascending, non-negative int64 and every
 * invariant of the list pool holds.  An empty vector (len == 0) is a present value, distinct from absent.  Regrowth, the
 * repack in mlvdb_index_compact, mlvdb_index_reset and mlvdb_attr_list_stats treat the column like a list column.
 *
 * In a program (mlvdb_where.h) the column takes EXISTS and LEN only.  Every entry that needs a scalar column, the raw list
 * entries (mlvdb_attr_list_set, _set_at, _get, _update_where: they could forge duplicate terms or non-finite weights) and
 * mlvdb_facet_list_values refuse it.
 *
 * Everything is validated on the host before any launch; a refusal is MLVDB_ERR_INVALID_ARG and writes nothing.
 */
#ifndef MLVDB_SPARSE_H
#define MLVDB_SPARSE_H

#include <stdint.h>

#include "mlvdb_list.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_ATTR_SPARSE 4 /* accepted by mlvdb_attr_define */
#define MLVDB_SPARSE_MAX_NNZ MLVDB_LIST_MAX_LEN
#define MLVDB_SPARSE_MAX_QUERY_TERMS 1024

/* Vectors of rows [first, first + n) in CSR form: row first + i gets (terms[j], weights[j]) for j in
 * [offsets[i], offsets[i + 1]) (offsets[0] >= 0).  present (n bytes, or NULL: all present): 0 makes the row absent, and its
 * range must be empty.  Refused: offsets that decrease, more than MLVDB_SPARSE_MAX_NNZ entries in a row, a negative term,
 * terms of a row that are not strictly ascending, a weight that is not finite. */
int mlvdb_sparse_set(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, const int64_t* offsets, const int32_t* terms,
                     const float* weights, const uint8_t* present);
/* The by-label sibling (mlvdb_attr_list_set_at): vector i -> row labels[i].  Labels inside [0, total), none twice;
 * tombstoned rows are skipped on the device, *updated = rows written. */
int mlvdb_sparse_set_at(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, const int64_t* offsets,
                        const int32_t* terms, const float* weights, const uint8_t* present, int64_t* updated);
/* Vectors of rows [first, first + n) as CSR with out_offsets[0] == 0, by the protocol of mlvdb_attr_list_get: *needed = their
 * number of entries, always exact; capacity < *needed: nothing else is written and the return is MLVDB_OK.  out_present
 * (n bytes, may be NULL): 0 for an absent row. */
int mlvdb_sparse_get(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int64_t* out_offsets, int32_t* out_terms,
                     float* out_weights, uint8_t* out_present, int64_t capacity, int64_t* needed);
/* Exact lexical kNN.  Query i is (q_terms[j], q_weights[j]) for j in [q_offsets[i], q_offsets[i + 1]) (q_offsets[0] == 0):
 * 0..MLVDB_SPARSE_MAX_QUERY_TERMS entries, terms in [0, 2^31) strictly ascending, weights finite.  Candidates are the live
 * rows whose vector is present (empty included) and that `where` (may be NULL) matches.  score(q, r) = the sum over the
 * shared terms of (double)wq * (double)wr, accumulated in fp64; a pair's score is a pure function of the two vectors (the
 * same 64 bits in any batch, position, filter, k).  Rows rank by (score descending, label ascending); a row without a
 * shared term scores +0.0 and ranks like any other.  1 <= k <= MLVDB_MAX_TOPK (above: MLVDB_ERR_UNSUPPORTED).
 * out_labels [nq, k] padded with -1, out_score [nq, k] = (float)score padded with -inf, out_score64 (may be NULL) the fp64
 * scores, out_counts[i] = min(k, candidates). */
int mlvdb_search_batch_sparse(mlvdb_index* h, int32_t attr, const int64_t* q_offsets, const int32_t* q_terms,
                              const float* q_weights, int64_t nq, int32_t k, const mlvdb_where* where, int64_t* out_labels,
                              float* out_score, int32_t* out_counts, double* out_score64);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_SPARSE_H */
