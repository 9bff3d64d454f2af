/*
 * mlvdb_maxsim.h -- late-interaction search: documents ranked by the summed distance of each query token to the
 * document's best row (companion of mlvdb_distinct.h / mlvdb_grouped.h; the ABI version of mlvdb_hip.h is unchanged).
 *
 * Query i is the token rows tokens[token_offsets[i] .. token_offsets[i + 1]), T_i of them, each of `dim` floats.  A
 * document is one present value of int64 column `attr`, as in mlvdb_distinct.h: rows with an absent value belong to no
 * document, only live rows count and, when `where` is given, only rows it matches (the counted rows).
 *
 * For token t and document g, best(t, g) is the smallest fp64 distance between t and a counted row of g, in the index's
 * space, with the bits mlvdb_pair_distances gives the pair.
 *   score(i, g) = (((0.0 + best(t0, g)) + best(t1, g)) + ...) in fp64, in the order the tokens were given.
 * Documents are ranked ascending by (score, group code): the order is total, so the answer depends neither on the launch
 * geometry nor on the order in which the device's atomics arrive.
 *
 * With T_i == 1 for every query the call equals mlvdb_search_batch_distinct with the same attr / where (groups, fp64 and
 * fp32 distances, counts; the match label is its label); with every row holding its own value it equals
 * mlvdb_search_batch_ex.  Every pass is the exact fp64 scan: nothing here is approximate.
 */
#ifndef MLVDB_MAXSIM_H
#define MLVDB_MAXSIM_H

#include <stdint.h>

#include "mlvdb_facet.h"
#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_MAXSIM_MAX_TOKENS 128                    /* tokens of one query */
#define MLVDB_MAXSIM_MAX_GROUPS MLVDB_FACET_MAX_VALUES /* documents among the counted rows */

/* 1 <= k <= MLVDB_MAX_TOPK (larger: MLVDB_ERR_UNSUPPORTED).  token_offsets holds nq + 1 entries, starts at 0 and is
 * strictly increasing (a query without tokens is refused); a query holds at most MLVDB_MAXSIM_MAX_TOKENS tokens.
 *   out_groups        [nq, k] group codes in rank order, INT64_MIN padded
 *   out_score         [nq, k] (float)score, +inf padded
 *   out_counts        [nq]    min(k, documents among the counted rows)
 *   out_score64       optional [nq, k] the fp64 score, +inf padded
 *   out_match_labels  optional [total_tokens, k]: row (token_offsets[i] + t, j) = the label of the best row of query i's
 *                     j-th document for its token t, by (fp64 distance, label); -1 padded
 *   out_match_dist64  optional [total_tokens, k]: that pair's distance, +inf padded; out_score64[i, j] is, bit for bit,
 *                     the sequential fp64 sum of out_match_dist64[token_offsets[i] + t, j] over t
 * Bad offsets, too many tokens in a query, an undefined or float64 attr, a bad program, nq < 0 or a null required buffer
 * is MLVDB_ERR_INVALID_ARG, all before anything is launched; non-finite token values are treated as
 * mlvdb_search_batch_ex treats non-finite queries (a distance that is NaN is never a best distance).  More than
 * MLVDB_MAXSIM_MAX_GROUPS documents among the counted rows is MLVDB_ERR_OVERFLOW.  An empty or fully tombstoned index
 * answers padding and launches nothing.  The queries are processed in chunks whose [token, document] workspace fits
 * MAXSIM_WS_MB MiB (a tuning key, default 1024; always at least one query); every setting returns the same bytes. */
int mlvdb_search_batch_maxsim(mlvdb_index* h, const float* tokens, const int64_t* token_offsets, int64_t nq, int32_t k,
                              int32_t attr, const mlvdb_where* where, int64_t* out_groups, float* out_score,
                              int32_t* out_counts, double* out_score64, int64_t* out_match_labels,
                              double* out_match_dist64);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_MAXSIM_H */
