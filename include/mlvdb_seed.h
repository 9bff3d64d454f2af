/*
 * mlvdb_seed.h -- greedy k-means++ seeding of the stored rows on the device: m rows picked one after the other, each drawn
 * with probability proportional to its distance from the rows picked so far, the best of `trials` draws kept per step
 * (companion of mlvdb_cluster.h, whose mlvdb_kmeans takes the picks as centroid labels; the ABI version of mlvdb_hip.h is
 * unchanged).  Everything below is stated so that a NumPy model reproduces the call bit for bit.
 *
 * Candidates.  The live rows that `where` matches (NULL: every live row), the program evaluated once, exactly as in
 * mlvdb_kmeans.  total = the rows of the index, tombstoned ones included; a label is a row's number in [0, total).
 *
 * Distances.  d(s, x) = the bits mlvdb_pair_distances returns for the query "stored fp32 row of label s" and label x -- the
 * distance of mlvdb_cluster.h.  The trial rows are gathered on the device: no vector crosses the bus.
 * clamp(d) = d > 0 ? d : +0.0, so a NaN, -0.0 and the tiny negatives cosine can give all become +0.0.
 * Spaces: l2 (the squared distance: d is the D^2 weight as it stands) and cosine (1 - cos, half the squared chord).
 *
 * The sum tree T(w).  P = the smallest power of two >= max(total, MLVDB_SEED_BLOCK).  w[x] is +0.0 for every label that is
 * no candidate and for every label >= total.  Level 0 is w; level l+1 [i] = level l [2i] + level l [2i+1], one rounded fp64
 * add, never contracted; the root is the single entry of level log2 P.
 *
 * descend(T, r), called only when root > 0.  From the root, at a node with left child sum a and right child sum b:
 *   b == 0: left;  else a == 0: right;  else r < a: left;  else r = r - a (one rounded subtract), right.
 * The leaf reached is the label; its weight is > 0 (the rule never enters a zero subtree).
 * draw(T, u) = descend(T, u * root), one rounded multiply.
 *
 * u: [m][trials] doubles, each in [0, 1) -- the caller's random numbers; the call draws none of its own.
 *
 * Step 0.  T1 = the tree of 1.0 over the candidates (its sums are exact integers).  c_0 = draw(T1, u[0][0]);
 *   best(x) = clamp(d(c_0, x)) for every candidate; out_potential[0] = root(T(best)).
 * Step j = 1 .. m - 1.  B = T(best).  For t = 0 .. trials - 1:
 *   s_t = draw(B, u[j][t]) if root(B) > 0, otherwise draw(T1, u[j][t]) (every candidate coincides with a pick: a duplicate
 *   pick is allowed then);  p_t(x) = clamp(d(s_t, x)) < best(x) ? clamp(d(s_t, x)) : best(x);  phi_t = root(T(p_t)).
 *   The winner is the lowest t with the smallest phi_t (strict < in ascending t; trials may coincide).
 *   c_j = s_winner, best = p_winner, out_potential[j] = phi_winner.
 * out_labels[j] = c_j, in pick order; *matched = the candidates.  Two calls return identical bytes.
 *
 * Device memory one call takes beside the index, with n = total rows and the planes' stride n rounded up to 4:
 *   8 (trials + 1) n bytes (best and one plane per trial), + 8 (trials + 1) 2 P / MLVDB_SEED_BLOCK (levels 8 .. log2 P of
 *   every trial's tree and of T1; the levels inside a block of MLVDB_SEED_BLOCK labels are never stored),
 *   + 4 trials (dim + ld) + 8 m (trials + 2) + O(1) (the trial rows dense and staged, u, the outputs).
 * A seeding of m steps reads the rows m times: at step j >= 1 one scan scores all trials (several when ld > 1024).
 *
 * Refusals, with nothing written: m outside 1 .. MLVDB_CLUSTER_MAX, trials outside 1 .. MLVDB_SEED_MAX_TRIALS, a u outside
 * [0, 1) or not finite, a null u or output, a bad program: MLVDB_ERR_INVALID_ARG.  An ip index, more than 2^31 - 1 rows:
 * MLVDB_ERR_UNSUPPORTED.  Fewer candidates than m (an empty index included; known after the program's one count):
 * MLVDB_ERR_INVALID_ARG with *matched written and the other outputs untouched.
 */
#ifndef MLVDB_SEED_H
#define MLVDB_SEED_H

#include <stdint.h>

#include "mlvdb_cluster.h"
#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_SEED_MAX_TRIALS 8
#define MLVDB_SEED_BLOCK 256

int mlvdb_kmeans_seed(mlvdb_index* h, int32_t m, int32_t trials, const double* u, const mlvdb_where* where,
                      int64_t* out_labels, double* out_potential, int64_t* matched);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_SEED_H */
