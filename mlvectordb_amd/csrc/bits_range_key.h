// The 64-bit key the bits walks hand to bits_range_sort_kernel (kernels_bits_range.hip, kernels_bits_join.hip).
#pragma once
#include "internal.h"

namespace mlvdb {

// (distance, row) as one integer that orders like the pair.  Hamming distances are integers; two distinct Jaccard quotients
// of denominators <= 32,640 differ by more than 2^-31 (>= 3.75e-9), the scaling by 2^31 is exact, and equal
// quotients give equal keys, so floor(d * 2^31) is strictly monotone on the distances that occur.  Rows stay below 2^31.
__device__ __forceinline__ uint64_t range_key(int32_t metric, int32_t ham, double d, int64_t row) {
    const uint64_t hi = metric == MLVDB_BITS_JACCARD ? (uint64_t)(d * 2147483648.0) : (uint64_t)ham;
    return hi << 32 | (uint64_t)row;
}

}  // namespace mlvdb
