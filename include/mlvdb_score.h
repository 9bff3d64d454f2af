/*
 * mlvdb_score.h -- scored kNN: rank rows by a formula of the vector distance and the attribute columns (companion of
 * mlvdb_where.h; the ABI version of mlvdb_hip.h is unchanged).
 *
 * The score of a (query, row) pair is a postfix program over a stack of fp64 values.  Every operation is one IEEE-754
 * binary64 operation, rounded to nearest even, never contracted with its neighbour:
 *   CONST        push the double whose bits are in `a`
 *   DIST         push the row's distance to the query in the index's space: the bits mlvdb_pair_distances(query, label) gives
 *   ATTR         push the row's value of column `attr`: an INT64 column converted with (double)v (rounded to nearest), a
 *                FLOAT64 column as is; an absent value (INT64_MIN / NaN) pushes the double whose bits are in `a` -- the
 *                default, which may itself be NaN ("no default")
 *   MATCH        push 1.0 if the row matches conds[a], else 0.0: exactly mlvdb_where_count's semantics of that program,
 *                list and geo ops included
 *   ADD SUB MUL DIV   pop y, pop x, push x <op> y
 *   MIN          pop y, pop x, push x <= y ? x : (y < x ? y : NaN)
 *   MAX          pop y, pop x, push x >= y ? x : (y > x ? y : NaN)     (this form fixes signed zeros and NaN, unlike fmin / fmax)
 *   NEG ABS      flip / clear the sign bit of the top
 *
 * Ranking.  A row is a candidate if it is live, matches `where` (NULL: every live row) and its score is not NaN.  NaN
 * propagates through every op above, so an absent attribute without a default and 0/0 both drop the row: that is the way to
 * skip such rows.  +-inf are ordinary scores.  Per query the min(k, candidates) candidates with the smallest score come back
 * in ascending (score, label) order -- -0.0 and +0.0 compare equal, ties go to the lower label.  out_score carries the fp64
 * score, out_dist64 the bits DIST had for that hit.  The tail is padded with label -1 and +inf; out_counts tells padding
 * from a real +inf score.  The answer is exact -- the top k over all candidates, no candidate window -- and two calls
 * return identical bytes.
 *
 * Limits, all checked on the host before anything is launched (a refused program is MLVDB_ERR_INVALID_ARG, never a device
 * fault): 1 <= n_ops <= MLVDB_SCORE_MAX_OPS; the stack never holds fewer values than an op pops, at most
 * MLVDB_SCORE_MAX_DEPTH, and exactly one at the end; n_conds <= MLVDB_SCORE_MAX_CONDS programs of together at most
 * MLVDB_WHERE_MAX_OPS ops, each validated as mlvdb_where_count validates it; ATTR on a defined INT64 / FLOAT64 column only
 * (list, sparse, geo and bits columns are refused); a MATCH index inside conds.
 */
#ifndef MLVDB_SCORE_H
#define MLVDB_SCORE_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_SCORE_MAX_OPS 32
#define MLVDB_SCORE_MAX_DEPTH 8
#define MLVDB_SCORE_MAX_CONDS 8

/* ops */
#define MLVDB_SCORE_CONST 0
#define MLVDB_SCORE_DIST 1
#define MLVDB_SCORE_ATTR 2
#define MLVDB_SCORE_MATCH 3
#define MLVDB_SCORE_ADD 4
#define MLVDB_SCORE_SUB 5
#define MLVDB_SCORE_MUL 6
#define MLVDB_SCORE_DIV 7
#define MLVDB_SCORE_MIN 8
#define MLVDB_SCORE_MAX 9
#define MLVDB_SCORE_NEG 10
#define MLVDB_SCORE_ABS 11

typedef struct mlvdb_score_op {
    int32_t op;
    int32_t attr; /* ATTR: the column */
    int64_t a;    /* CONST: the double's bits; ATTR: the default's bits; MATCH: the index into conds */
} mlvdb_score_op;

typedef struct mlvdb_score {
    const mlvdb_score_op* ops;
    int32_t n_ops;
    const mlvdb_where* conds; /* the programs MATCH refers to (may be NULL when n_conds == 0) */
    int32_t n_conds;
} mlvdb_score;

/* The k best-scored candidates for nq queries.  1 <= k <= MLVDB_MAX_TOPK (larger: MLVDB_ERR_UNSUPPORTED).
 * where: NULL, or one program restricting the rows first -- validated and applied exactly as in mlvdb_search_batch_where.
 * out_labels, out_score: [nq, k]; out_counts: [nq]; out_dist64 ([nq, k], +inf in the padded tail) is optional.  nq = 0 and
 * an empty index succeed.  mlvdb_index_last_stats reports the scan of the last chunk of queries. */
int mlvdb_search_batch_scored(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, const mlvdb_score* score,
                              const mlvdb_where* where, int64_t* out_labels, double* out_score, int32_t* out_counts,
                              double* out_dist64);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_SCORE_H */
