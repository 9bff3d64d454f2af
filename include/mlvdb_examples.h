/*
 * mlvdb_examples.h -- recommend and discover: rank the rows against a SET of examples, each judged on its own (companion of
 * mlvdb_like.h, which averages its examples into one query; the ABI version of mlvdb_hip.h is unchanged).
 *
 * Examples.  Query i owns the examples j = example_offsets[i] .. example_offsets[i + 1] - 1, in the order given, at most
 * MLVDB_EXAMPLES_MAX of them.  example_labels[j] >= 0: the example is the stored fp32 row of that label, read in device
 * memory (a tombstoned label is valid, as it is for mlvdb_pair_distances).  example_labels[j] == -1: the example is row j of
 * example_vectors ([example_offsets[nq], dim] fp32, every value finite; may be NULL when no label is -1).
 *
 * Distances.  d_j(x) is the distance between example j, used as a query, and row x in the index's space: the very bits
 * mlvdb_pair_distances returns for that vector and label.
 *
 * Ranking.  Every candidate row gets a key (tier: int32, value: fp64); rows are ranked ascending by (tier, value, label).
 * -0.0 and +0.0 compare equal, ties go to the lower label, a row whose value is NaN is no candidate, +-inf are ordinary values.
 *   MLVDB_EXAMPLES_BEST      roles POS / NEG in any order, at least one example.  p = min over POS of d_j, n = min over NEG
 *                            of d_j, +inf for an empty set (a NaN distance makes its minimum NaN).  With a POS example and
 *                            (no NEG example or p < n) the row is tier 0 with value p; otherwise tier 1 with value -n (the
 *                            sign bit flipped): the farthest from its nearest disliked example first.
 *   MLVDB_EXAMPLES_DISCOVER  the first example has role TARGET, m >= 0 pairs (POS, NEG) follow, adjacent and in that order.
 *                            tier = #{pairs : not (d_pos < d_neg)}, value = d_target.  With m = 0 this is the plain exact
 *                            search.
 *   MLVDB_EXAMPLES_CONTEXT   m >= 1 pairs (POS, NEG), no target.  tier = 0, value = s_m with s_0 = 0.0 and
 *                            s_{i+1} = s_i + (d_pos_i > d_neg_i ? d_pos_i - d_neg_i : 0.0): one rounded fp64 operation per
 *                            step, in pair order, never contracted.
 *
 * Candidates.  A row is a candidate if it is live and matches `where` (NULL: every live row; one program, validated and
 * applied exactly as in mlvdb_search_batch_where).  With exclude_examples != 0 a row whose label is among the query's own
 * stored example labels is no candidate either.
 *
 * Outputs.  out_labels [nq, k] padded with -1, out_tier [nq, k] padded with INT32_MAX, out_value [nq, k] padded with +inf,
 * out_counts [nq] = min(k, candidates).  The answer is the exact top k over all candidates, and two calls return identical
 * bytes.
 *
 * Refusals, all on the host before the first launch and with nothing written: k < 1, nq < 0, offsets that do not ascend from
 * 0, an empty bag, a label outside [-1, total), a non-finite raw vector, a role sequence the mode does not allow, an unknown
 * mode, a bad program, a null required buffer: MLVDB_ERR_INVALID_ARG.  k > MLVDB_MAX_TOPK and a bag of more than
 * MLVDB_EXAMPLES_MAX examples: MLVDB_ERR_UNSUPPORTED.  nq = 0 and an empty index succeed.
 */
#ifndef MLVDB_EXAMPLES_H
#define MLVDB_EXAMPLES_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_EXAMPLES_MAX 64

/* modes */
#define MLVDB_EXAMPLES_BEST 0
#define MLVDB_EXAMPLES_DISCOVER 1
#define MLVDB_EXAMPLES_CONTEXT 2

/* roles */
#define MLVDB_EXAMPLE_POS 0
#define MLVDB_EXAMPLE_NEG 1
#define MLVDB_EXAMPLE_TARGET 2

int mlvdb_search_batch_examples(mlvdb_index* h, int32_t mode, const int64_t* example_labels, const float* example_vectors,
                                const int32_t* example_roles, const int64_t* example_offsets, int64_t nq, int32_t k,
                                int32_t exclude_examples, const mlvdb_where* where, int64_t* out_labels, int32_t* out_tier,
                                double* out_value, int32_t* out_counts);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_EXAMPLES_H */
