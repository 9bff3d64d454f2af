// The fixed 16-lane fp64 fold of the sparse kernels (kernels_sparse.hip: the scan; kernels_hybrid.hip: the gathered scorer).
// Both must fold a pair's 16 partial sums by the same operations for a pair's score to be one value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mlvdb {

constexpr int kSparseBitmapBits = 8192;  // B: <= 1/8 full with a full union
constexpr int kSparseBitmapWords = kSparseBitmapBits / 32;

// v of lane (lane ^ 1), (lane ^ 2), then of the mirrored lane of its half row and of its row: after the first two steps a
// quad holds one value, after the third a half row does, so the mirrors read "the other quad" and "the other half".
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// The sum of the 16 lanes of a DPP row, the same bits on each of them.  Full wave only.
__device__ __forceinline__ double row16_sum(double v) {
    v = v + dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
    v = v + dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    v = v + dpp_f64<0x141>(v);  // row_half_mirror
    v = v + dpp_f64<0x140>(v);  // row_mirror
    return v;
}

}  // namespace mlvdb
