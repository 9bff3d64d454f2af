/*
 * mlvdb_like.h -- search by stored examples ("more like this"): the queries are built on the device from rows the index
 * already holds, and the examples are taken out of the ranked lists there too (companion of mlvdb_where.h; the ABI version
 * of mlvdb_hip.h is unchanged).
 *
 * The query.  Query i has the examples j = example_offsets[i] .. example_offsets[i + 1] - 1, in the order given, m_i of
 * them.  For column c, in fp64:
 *     acc = base_queries ? (double)base_queries[i][c] : 0.0
 *     for each example j:  acc = acc + t_j * (double)x_j[c]
 * -- one rounded product and one rounded addition per example, no fma -- where x_j is the stored fp32 row of label
 * example_labels[j] and
 *     t_j = example_weights[j]                        on l2 and ip indexes,
 *     t_j = example_weights[j] * inv_j                on a cosine index, one rounded product formed once per example,
 * with inv_j = 1 / (|x_j| + 1e-30), the bits the query preparation of this library gives that row's values when they come
 * as a query (the norm term mlvdb_pair_distances uses for them): cosine examples contribute as unit vectors.
 * The query value is (float)acc, rounded once; out_queries ([nq, dim], optional) receives these bits.
 * A label may repeat inside a query: it is summed each time it appears.  A tombstoned label is still a valid example -- its
 * values are still stored, as for mlvdb_pair_distances.
 *
 * The hits.  E_i is the set of distinct example labels of query i, M = max_i |E_i| over the call.  The hits of query i are
 * what mlvdb_search_batch_ex returns for out_queries[i] at top_k = k + M -- with a `where` program, what
 * mlvdb_search_batch_where returns -- with the entries whose label is in E_i removed, the order kept, the first k of them:
 * out_counts[i] is their number, out_labels / out_dist / out_dist64 ([nq, k] each) carry the plain search's own bits for
 * them, the tail is padded with label -1 / +inf.  This is exact: the k + M nearest rows contain the k nearest rows that
 * are no example.  With exclude_examples == 0 nothing is removed, the inner search runs at top_k = k, and the call equals
 * the plain search of out_queries, bit for bit.
 *
 * A synthesised query that comes out all zero (the same row as a positive and a negative example, say) or non-finite is
 * given to the inner search as it is, and that search has no rule for either when it comes from the host: an all-zero
 * query gets the norm term of a zero vector (cosine: every live row at distance 1, so the hits are the lowest live labels
 * that are no example), a non-finite one the distances its values produce.  Neither is refused.
 */
#ifndef MLVDB_LIKE_H
#define MLVDB_LIKE_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_LIKE_MAX_FETCH 1024
#define MLVDB_LIKE_MAX_EXAMPLES 64

/* Limits, all checked on the host before anything is launched: 1 <= k, k + M <= MLVDB_LIKE_MAX_FETCH, every
 * m_i <= MLVDB_LIKE_MAX_EXAMPLES; exceeding one of them: MLVDB_ERR_UNSUPPORTED.  MLVDB_ERR_INVALID_ARG: offsets that do not
 * ascend from 0, a label outside [0, total), a weight that is not finite, a query with no example and no base row, a null
 * required buffer (example_offsets, out_labels, out_dist, out_counts; example_labels and example_weights when there is an
 * example), nq < 0, k < 1, a bad program.
 * where: NULL, or one program restricting the rows of the inner search -- validated and applied exactly as in
 * mlvdb_search_batch_where; the examples themselves need not match it.
 * base_queries, out_dist64 and out_queries are optional.  nq = 0 and an empty index succeed (nothing / only padding
 * written; out_queries then holds the base rows).  mlvdb_index_last_stats reports the inner search of the (last chunk of
 * the) call. */
int mlvdb_search_batch_like(mlvdb_index* h, const int64_t* example_labels, const double* example_weights,
                            const int64_t* example_offsets, const float* base_queries, int64_t nq, int32_t k,
                            int32_t exclude_examples, const mlvdb_where* where, int64_t* out_labels, float* out_dist,
                            int32_t* out_counts, double* out_dist64, float* out_queries);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_LIKE_H */
