// Metadata filters on the device (include/mlvdb_where.h): the predicate program over the attribute columns -> the row
// mask of a filtered kNN / range call, and the attribute columns' share of the index's lifecycle (absent fill, compaction
// gather).  The program reaches the kernel validated (api.hip: where_prepare), so nothing here checks it again.
#include <algorithm>

#include "internal.h"
#include "where_common.h"

namespace mlvdb {

// One thread per row, grid-stride.  The program (<= 64 ops, 2 KiB) is staged in LDS and evaluated by where_eval_row
// (where_common.h).
__global__ __launch_bounds__(256) void where_eval_kernel(const WhereOp* __restrict__ prog, int32_t n_ops,
                                                         const int64_t* __restrict__ set, const float* __restrict__ rn,
                                                         int64_t total, uint8_t* __restrict__ mask,
                                                         unsigned long long* __restrict__ matches) {
    __shared__ WhereOp sp[kWhereMaxOps];
    __shared__ unsigned long long block_hits;
    if ((int)threadIdx.x < n_ops) sp[threadIdx.x] = prog[threadIdx.x];
    if (threadIdx.x == 0) block_hits = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long wave_hits = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // i0 is uniform over the block: every lane of a wave runs the same iterations (the ballot below needs all of them)
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < total;
        const bool match = where_eval_row(sp, n_ops, set, i, in);
        const bool hit = in && match && rn[i] == rn[i];  // tombstoned rows (NaN norm) never match
        if (in) mask[i] = hit ? 1 : 0;
        const unsigned long long b = __ballot(hit);
        if (lane == 0) wave_hits += __popcll(b);
    }
    if (lane == 0 && wave_hits) atomicAdd(&block_hits, wave_hits);
    __syncthreads();
    if (threadIdx.x == 0 && block_hits) atomicAdd(matches, block_hits);
}

hipError_t launch_where_eval(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, int64_t total,
                             uint8_t* mask, unsigned long long* matches, hipStream_t s) {
    if (total == 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    where_eval_kernel<<<(unsigned)blocks, 256, 0, s>>>(prog, n_ops, set, rn, total, mask, matches);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void attr_fill_kernel(int64_t* __restrict__ col, int64_t value, int64_t first, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        col[first + i] = value;
}

hipError_t launch_attr_fill(int64_t* col, int64_t value, int64_t first, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 16);
    attr_fill_kernel<<<(unsigned)blocks, 256, 0, s>>>(col, value, first, n);
    return hipGetLastError();
}

// compaction: ncol[new] = col[old_of_new[new]] for the live rows (ncol already absent-filled beyond them)
__global__ __launch_bounds__(256) void attr_gather_kernel(const int64_t* __restrict__ col, int64_t* __restrict__ ncol,
                                                          const int32_t* __restrict__ old_of_new, int64_t live) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < live; i += (int64_t)gridDim.x * blockDim.x)
        ncol[i] = col[old_of_new[i]];
}

hipError_t launch_attr_gather(const int64_t* col, int64_t* ncol, const int32_t* old_of_new, int64_t live, hipStream_t s) {
    if (live <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((live + 255) / 256, 256 * 16);
    attr_gather_kernel<<<(unsigned)blocks, 256, 0, s>>>(col, ncol, old_of_new, live);
    return hipGetLastError();
}

}  // namespace mlvdb
