/*
 * mlvdb_mmr.h -- diversified kNN: greedy maximal-marginal-relevance (MMR) selection on the device (companion of
 * mlvdb_where.h; the ABI version of mlvdb_hip.h is unchanged).
 *
 * Candidates.  Per query the candidate list is exactly what mlvdb_search_batch_ex returns at top_k = fetch_k -- with a
 * `where` program, what mlvdb_search_batch_where returns: labels c_0..c_{m-1} in the canonical order of this library
 * (fp64 distance, label), their fp64 distances dq_i to the query, m = count <= fetch_k.
 *
 * Selection, all in fp64.  S is the ordered list of picked positions; the first pick is position 0.  After each pick s,
 * for every candidate i: mind_i = min(mind_i, D(s, i)).  The next pick is the unpicked i that minimises
 *     obj_i = lambda * dq_i - (1.0 - lambda) * mind_i
 * -- two rounded products and one rounded subtraction, (1.0 - lambda) formed once on the host -- ties to the lower
 * position; selection stops after min(k, m) picks.
 * Direction of D: D(s, i) is the index's distance with the stored fp32 values of row c_s as the QUERY and row c_i as the
 * ROW; its bits are what mlvdb_pair_distances gives for (values of row c_s, label c_i).  For cosine D(s, i) and D(i, s)
 * may differ in the last bit; for l2 and ip they do not.
 * The index's distance serves all three spaces; for cosine and ip the order of the picks is that of the textbook
 * lambda * sim(q, i) - (1 - lambda) * max_j sim(i, j) with sim = 1 - d.
 *
 * Outputs, in pick order ([nq, k] each): out_labels / out_dist / out_dist64 carry the candidate list's own bits for the
 * picked entries (so they equal mlvdb_pair_distances(query, label), fp64 and the once-rounded fp32); out_rank the picked
 * position in the candidate list; out_objective obj at the time of the pick (first pick: lambda * dq_0);
 * out_counts[i] = min(k, m).  The tail is padded with label -1 / +inf, rank -1 and objective +inf.
 * lambda = 1 returns the first k entries of the plain search at fetch_k, bit for bit; fetch_k = k a permutation of the
 * plain top-k.
 */
#ifndef MLVDB_MMR_H
#define MLVDB_MMR_H

#include <stdint.h>

#include "mlvdb_where.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_MMR_MAX_FETCH 1024

/* Limits, all checked before anything is launched: 1 <= k <= MLVDB_MAX_TOPK, k <= fetch_k <= MLVDB_MMR_MAX_FETCH,
 * 0 <= lambda <= 1 (not NaN).  k > MLVDB_MAX_TOPK, fetch_k > MLVDB_MMR_MAX_FETCH, or a dim whose selection state --
 * ld x 8 bytes for the picked row plus fetch_k x 20 bytes per-candidate state -- exceeds 64 KiB of LDS:
 * MLVDB_ERR_UNSUPPORTED; everything else (nq < 0, a null buffer, a bad program): MLVDB_ERR_INVALID_ARG.
 * where: NULL, or one program restricting the rows first -- validated and applied exactly as in mlvdb_search_batch_where.
 * out_dist64, out_rank and out_objective are optional.  nq = 0 and an empty index succeed (nothing / only padding written).
 * mlvdb_index_last_stats reports the plain search of the (last chunk of the) call. */
int mlvdb_search_batch_mmr(mlvdb_index* h, const float* queries, int64_t nq, int32_t k, int32_t fetch_k, double lambda,
                           const mlvdb_where* where, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                           double* out_dist64, int32_t* out_rank, double* out_objective);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_MMR_H */
