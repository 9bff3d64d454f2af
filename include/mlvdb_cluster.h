/*
 * mlvdb_cluster.h -- partition the stored rows: nearest-centroid assignment and Lloyd's k-means on the device, the cluster id
 * written into an int64 attribute column (companion of mlvdb_examples.h and mlvdb_mutate.h; the ABI version of mlvdb_hip.h is
 * unchanged).
 *
 * Centroids.  m of them, 1 <= m <= MLVDB_CLUSTER_MAX, given the way mlvdb_search_batch_examples takes examples:
 * centroid_labels[j] >= 0 is the stored fp32 row of that label, read in device memory (a tombstoned label is valid, as it is
 * for mlvdb_pair_distances); centroid_labels[j] == -1 is row j of centroid_vectors ([m, dim] fp32, every value finite; may be
 * NULL when no label is -1).  centroid_labels == NULL: every centroid is raw.
 *
 * Candidates.  The live rows that `where` matches (NULL: every live row; one program, validated and applied exactly as in
 * mlvdb_search_batch_where).  The program is evaluated ONCE, before anything is written, so it may read assign_attr itself.
 *
 * The rule (mlvdb_assign_nearest, and every iteration of mlvdb_kmeans).  For a candidate x start from c(x) = -1,
 * best = +inf; for j = 0 .. m - 1 in this order centroid j wins -- c(x) = j, best = d_j(x) -- when d_j(x) < best.  d_j(x) is the
 * distance between centroid j, used as a query, and row x in the index's space: the very bits mlvdb_pair_distances returns
 * for that vector and label.  Ties therefore go to the lower j, a NaN never wins and neither does +inf; a candidate left at
 * c(x) = -1 is UNASSIGNED.  The members of j are the candidates with c(x) = j.
 *
 * The blocked sum.  Every sum over the members of a cluster below is taken in this order and no other: the members in
 * ascending label order, cut into segments of MLVDB_CLUSTER_SEGMENT members (the last may be shorter); each segment summed
 * left to right in fp64 starting from +0.0; the segment sums summed left to right starting from +0.0.  One rounded fp64
 * operation per step, never contracted.
 *
 * mlvdb_assign_nearest.  Works for l2, cosine and ip.
 *   assign_attr >= 0: a defined MLVDB_ATTR_INT64 column; it receives c(x) for every candidate, INT64_MIN (absent) for an
 *   unassigned one.  Rows that are no candidates, tombstoned rows included, are not touched.  assign_attr == -1: no column is
 *   written.  out_rows[j] = the members of j; out_cost[j] = the blocked sum of their fp64 best distances;
 *   *matched = the candidates, so sum(out_rows) + unassigned == *matched.
 *
 * mlvdb_kmeans.  Lloyd's algorithm from the given centroids C_0; l2 and cosine only (no mean minimises ip:
 * MLVDB_ERR_UNSUPPORTED; mlvdb_assign_nearest still serves ip).  For t = 1 .. T:
 *   A_t    = the assignment against C_{t-1} by the rule;
 *   C_t[j] = the mean of the members of j under A_t: per column the blocked sum of the addends, divided by the member count
 *            in fp64, rounded once to fp32.  A cluster without members keeps C_{t-1}[j].
 *            l2: the addend is (double)x_c.  cosine (spherical k-means): the addend is (double)x_c * w(x) with
 *            w(x) = 1 / (sqrt(nx) + 1e-30), where nx is the scans' own sum of squares of the row: with s_g the sum over
 *            kb = 0, 1, ... and then i = 0 .. 3 of the (exact) fp64 squares of columns 16 kb + 4 g + i, left to right from +0.0,
 *            nx = (s_0 + s_1) + (s_2 + s_3).  It is a pure function of the row; no second norm exists in the library;
 *   stop after the first t >= 2 with A_t == A_{t-1} (*converged = 1), otherwise at T = max_iterations (*converged = 0),
 *   1 <= max_iterations <= MLVDB_CLUSTER_MAX_ITERATIONS.
 *   Returned: out_centroids = C_T ([m, dim] fp32), out_rows / out_cost / *matched of A_T as above, assign_attr holds A_T,
 *   *iterations = T.  When *converged is 1, C_T == C_{T-1} bit for bit, so the column is also the assignment against the
 *   returned centroids; when it is 0, mlvdb_assign_nearest with C_T gives that assignment.
 *   An empty index or a call without candidates succeeds with C_T = C_0 and zeros.
 *
 * The answer depends on the index contents and the arguments only: two calls return identical bytes.
 *
 * Device memory one call takes beside the index, with n = total rows, c = candidates, ld = dim rounded up to 16:
 *   20 n bytes (best distance, tile state, assignment, member list), + 8 n for cosine k-means (w),
 *   + 4 m ceil(n / 4096) (the listing's histograms) + 8 (ld + 1) (c / MLVDB_CLUSTER_SEGMENT + m) (the segment sums)
 *   + 4 m (dim + ld) + O(m) (the centroids, dense and staged).
 * The segment sums are what makes this more than a fixed number of bytes per row: 8 (ld + 1) / 256 B per candidate, i.e.
 * ld / 32 -- 24 B at 768 columns, 44 to 52 B per row in all there, under 2 % of the 3 KiB the row itself takes.  They buy the
 * sum stage one wave per (segment, column slice) instead of one per (cluster, column slice).
 *
 * Refusals, all on the host before the first launch and with nothing written: m outside 1 .. MLVDB_CLUSTER_MAX, a label
 * outside [-1, total), a raw centroid without centroid_vectors or with a non-finite value, an assign_attr that is neither -1
 * nor a defined MLVDB_ATTR_INT64 column, max_iterations < 1, a bad program, a null output: MLVDB_ERR_INVALID_ARG.
 * max_iterations > MLVDB_CLUSTER_MAX_ITERATIONS, mlvdb_kmeans on an ip index, more than 2^31 - 1 rows: MLVDB_ERR_UNSUPPORTED.
 */
#ifndef MLVDB_CLUSTER_H
#define MLVDB_CLUSTER_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_CLUSTER_MAX 1024
#define MLVDB_CLUSTER_SEGMENT 256
#define MLVDB_CLUSTER_MAX_ITERATIONS 1000

int mlvdb_assign_nearest(mlvdb_index* h, const int64_t* centroid_labels, const float* centroid_vectors, int32_t m,
                         const mlvdb_where* where, int32_t assign_attr, int64_t* out_rows, double* out_cost, int64_t* matched);

int mlvdb_kmeans(mlvdb_index* h, const int64_t* centroid_labels, const float* centroid_vectors, int32_t m,
                 int32_t max_iterations, const mlvdb_where* where, int32_t assign_attr, float* out_centroids,
                 int64_t* out_rows, double* out_cost, int32_t* iterations, int32_t* converged, int64_t* matched);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_CLUSTER_H */
