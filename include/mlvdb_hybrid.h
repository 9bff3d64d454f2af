/*
 * mlvdb_hybrid.h -- hybrid search: a dense and a sparse kNN answer fused into one ranked list on the device (companion of
 * mlvdb_sparse.h and mlvdb_where.h; the ABI version of mlvdb_hip.h is unchanged).
 *
 * Candidate lists.  Per query, D is exactly what mlvdb_search_batch_ex returns at top_k = fetch_dense -- with a `where`
 * program, what mlvdb_search_batch_where returns: labels, fp64 distances, count -- and S exactly what
 * mlvdb_search_batch_sparse returns at k = fetch_sparse (with the same program): rows with a present vector only, fp64
 * scores, ranked by (score descending, label ascending).  There is no special case: an empty sparse query gets the
 * label-ordered zero-score list the sparse search gives it (a caller without a sparse query wants the plain search).
 * C is the union of the labels of D and S, |C| <= fetch_dense + fetch_sparse <= 1088.
 *
 * Completion.  Every c in C gets both components, whichever list found it:
 *     dd(c)  the index's distance, the bits of mlvdb_pair_distances(query, c); for a member of D the list's own value
 *     ss(c)  the sparse score, the bits mlvdb_search_batch_sparse reports for the pair (a pair's score is a pure function of
 *            the two vectors); +0.0 for a row whose sparse vector is absent (only D can contribute such a row)
 *
 * Methods, all in fp64, each a fixed sequence of rounded operations (rank_D / rank_S: 0-based positions in the lists):
 *     MLVDB_FUSE_RRF       t_d = w_dense / (c + (double)(rank_D + 1)) if c is in D, else +0.0; t_s likewise with w_sparse and
 *                          rank_S; fused = t_d + t_s
 *     MLVDB_FUSE_LINEAR    fused = w_sparse * ss - w_dense * dd   (two rounded products, one rounded subtraction; for cosine
 *                          and ip this orders like the textbook w_dense * sim + w_sparse * ss)
 *     MLVDB_FUSE_RELATIVE  min-max over the COMPLETED UNION C, not over each leg's own list:
 *                          nd = (dmax - dd) / (dmax - dmin), 0.0 when dmax == dmin;
 *                          ns = (ss - smin) / (smax - smin), 0.0 when smax == smin;
 *                          fused = w_dense * nd + w_sparse * ns
 *
 * Rows rank by (fused descending, label ascending).  out_labels [nq, k] is padded with -1, out_fused [nq, k] with -inf,
 * out_counts[i] = min(k, |C|).  Optional outputs ([nq, k] each, NULL to skip): out_dist64 / out_sparse64 the completed
 * components of each hit (padding: +inf / -inf), out_rank_dense / out_rank_sparse its position in D / S, -1 when it is not in
 * that list (and as padding).
 */
#ifndef MLVDB_HYBRID_H
#define MLVDB_HYBRID_H

#include <stdint.h>

#include "mlvdb_sparse.h"
#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_FUSE_RRF 0
#define MLVDB_FUSE_LINEAR 1
#define MLVDB_FUSE_RELATIVE 2
#define MLVDB_HYBRID_MAX_FETCH_DENSE 1024

/* queries: [nq, dim] fp32.  The sparse queries are a CSR exactly as for mlvdb_search_batch_sparse (q_offsets[0] == 0, at most
 * MLVDB_SPARSE_MAX_QUERY_TERMS terms each, strictly ascending, finite weights); attr is a sparse column.
 * Limits, all checked on the host before anything is launched: 1 <= k <= MLVDB_MAX_TOPK, 1 <= fetch_dense <=
 * MLVDB_HYBRID_MAX_FETCH_DENSE, 1 <= fetch_sparse <= MLVDB_MAX_TOPK, k <= fetch_dense + fetch_sparse; w_dense, w_sparse and
 * rrf_c finite and >= 0.  k or a fetch size above its limit: MLVDB_ERR_UNSUPPORTED; everything else (a column that is not
 * sparse, a malformed query, a negative or non-finite weight, a NaN, an unknown method, a null buffer, k > fetch_dense +
 * fetch_sparse, a bad program): MLVDB_ERR_INVALID_ARG.  A refusal writes nothing.
 * where: NULL, or one program, evaluated ONCE, that restricts both legs.
 * nq = 0, an empty index and a fully tombstoned index succeed (nothing / only padding written). */
int mlvdb_search_batch_hybrid(mlvdb_index* h, const float* queries, int32_t attr, const int64_t* q_offsets,
                              const int32_t* q_terms, const float* q_weights, int64_t nq, int32_t k, int32_t fetch_dense,
                              int32_t fetch_sparse, int32_t method, double w_dense, double w_sparse, double rrf_c,
                              const mlvdb_where* where, int64_t* out_labels, double* out_fused, int32_t* out_counts,
                              double* out_dist64, double* out_sparse64, int32_t* out_rank_dense, int32_t* out_rank_sparse);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_HYBRID_H */
