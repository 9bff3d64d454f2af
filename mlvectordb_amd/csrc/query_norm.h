// The norm term of a query (qaux), in two pieces shared by every kernel that prepares one, so that a row taken as a query
// (kernels_mmr.hip) gets the bits launch_query_prep gives its values.
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"

namespace mlvdb {

// A 256-thread block: thread t holds the fp64 fma sum of v_c^2 over the padded columns c = t, t + 256, ... ascending;
// query_norm_wave_sum folds a wave's lanes (every lane ends with the wave's sum), lane 0 of wave w stores it to sums[w], and
// after a barrier query_aux_from_sums gives 1/(|q|+1e-30) (cosine) or |q| (l2, ip).
__device__ __forceinline__ double query_norm_wave_sum(double s) {
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
__device__ __forceinline__ double query_aux_from_sums(const double* sums, int space) {
    const double nrm = __builtin_sqrt((sums[0] + sums[1]) + (sums[2] + sums[3]));
    return space == kSpaceCosine ? 1.0 / (nrm + 1e-30) : nrm;
}

}  // namespace mlvdb
