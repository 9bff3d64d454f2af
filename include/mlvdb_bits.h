/*
 * mlvdb_bits.h -- binary vector columns: one fixed-width bit code per row (perceptual hashes, SimHash / MinHash signatures,
 * binarised embeddings, chemical fingerprints), and the exact top-k Hamming or Jaccard (Tanimoto) distance of a batch of
 * codes against them on the device (companion of mlvdb_list.h, ABI version 7).
 *
 * Column type MLVDB_ATTR_BITS.  It shares the list column's storage (mlvdb_list.h): the 8-byte column value is the slot
 *     (offset << 8) | words      the row's code is pool[offset, offset + words), 1 <= words <= MLVDB_BITS_MAX_WORDS
 *     INT64_MIN                  the row has no code (absent)
 * into the attribute's append-only int64 pool.  Word w of a code holds its bits 64w .. 64w + 63 (bit b of the code is bit
 * b & 63 of word b >> 6); a pool element is an arbitrary 64-bit pattern.  Regrowth, the repack in mlvdb_index_compact,
 * mlvdb_index_reset and mlvdb_attr_list_stats treat the column like a list column.
 *
 * The column has no width of its own: a present row has the width it was written with, and a search of width `words` takes
 * as candidates only the rows whose code holds exactly `words` words -- a row of another width behaves like an absent one.
 *
 * In a program (mlvdb_where.h) the column takes EXISTS only.  Every entry that needs a scalar column, the raw list entries,
 * the sparse entries and mlvdb_facet_list_values refuse it.
 *
 * Everything is validated on the host before any launch; a refusal is MLVDB_ERR_INVALID_ARG and writes nothing.
 */
#ifndef MLVDB_BITS_H
#define MLVDB_BITS_H

#include <stdint.h>

#include "mlvdb_list.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_ATTR_BITS 6 /* accepted by mlvdb_attr_define */
#define MLVDB_BITS_MAX_WORDS 255 /* a code is 1..255 64-bit words (64 .. 16,320 bits): the slot's 8-bit length */
#define MLVDB_BITS_HAMMING 0
#define MLVDB_BITS_JACCARD 1

/* Codes of rows [first, first + n): row first + i gets codes[i * words .. (i + 1) * words).  present (n bytes, or NULL: all
 * present): 0 makes the row absent, and its words are ignored.  Refused: words outside 1..MLVDB_BITS_MAX_WORDS, a null
 * codes with n > 0, a row range outside [0, total). */
int mlvdb_bits_set(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int32_t words, const uint64_t* codes,
                   const uint8_t* present);
/* The by-label sibling (mlvdb_attr_list_set_at): code i -> row labels[i].  Labels inside [0, total), none twice; tombstoned
 * rows are skipped on the device, *updated = rows written. */
int mlvdb_bits_set_at(mlvdb_index* h, int32_t attr, const int64_t* labels, int64_t n, int32_t words, const uint64_t* codes,
                      const uint8_t* present, int64_t* updated);
/* Codes of rows [first, first + n), back to back in row order, by the protocol of mlvdb_attr_list_get: out_words[i] = the
 * width of row first + i in words (0: absent), *needed = their sum, always exact; capacity (in words) < *needed: neither
 * out_words nor out_codes is written and the return is MLVDB_OK. */
int mlvdb_bits_get(mlvdb_index* h, int32_t attr, int64_t first, int64_t n, int32_t* out_words, uint64_t* out_codes,
                   int64_t capacity, int64_t* needed);
/* Exact kNN over bit codes.  Query i is queries[i * words .. (i + 1) * words).  Candidates are the live rows with a present
 * code of exactly `words` words that `where` (may be NULL) matches.  With x the row's code and q the query,
 *     MLVDB_BITS_HAMMING   d = popcount(q ^ x)
 *     MLVDB_BITS_JACCARD   i = popcount(q & x), u = popcount(q) + popcount(x) - i, d = (double)(u - i) / (double)u,
 *                          and 0.0 when u == 0
 * -- integers, and one correctly rounded fp64 division of two integers: the same 64 bits in any batch, position, filter, k.
 * Rows rank by (distance ascending, label ascending).  1 <= k <= MLVDB_MAX_TOPK (above: MLVDB_ERR_UNSUPPORTED, outputs
 * untouched); 0 <= nq <= 2^24.  out_labels [nq, k] padded with -1, out_dist [nq, k] = (float)d padded with +inf, out_dist64
 * (may be NULL) the fp64 distances, out_counts[i] = min(k, candidates). */
int mlvdb_search_batch_bits(mlvdb_index* h, int32_t attr, const uint64_t* queries, int64_t nq, int32_t words, int32_t metric,
                            int32_t k, const mlvdb_where* where, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                            double* out_dist64);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_BITS_H */
