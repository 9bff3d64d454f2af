// Metadata filters on the device (include/mlvdb_where.h): the predicate program over the attribute columns -> the row
// mask of a filtered kNN / range call, and the attribute columns' share of the index's lifecycle (absent fill, compaction
// gather).  The program reaches the kernel validated (api.hip: where_prepare), so nothing here checks it again.
#include <algorithm>

#include "internal.h"

namespace mlvdb {

// One thread per row, grid-stride.  The program (<= 64 ops, 2 KiB) is staged in LDS; the boolean stack is one 32-bit
// register (bit 0 = top).  Every op of the program is uniform over the wave, so the branches below never diverge; what
// differs per lane is only the value each column op loads (8 coalesced bytes per row and referenced op).
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
        uint32_t st = 0;
        for (int p = 0; p < n_ops; ++p) {
            const WhereOp o = sp[p];
            if (o.op == MLVDB_WHERE_AND || o.op == MLVDB_WHERE_OR) {
                const uint32_t x = st & 1u, y = (st >> 1) & 1u;
                st = ((st >> 2) << 1) | (o.op == MLVDB_WHERE_AND ? (x & y) : (x | y));
                continue;
            }
            if (o.op == MLVDB_WHERE_NOT) {
                st ^= 1u;
                continue;
            }
            bool bit = true;  // MLVDB_WHERE_TRUE
            if (o.op != MLVDB_WHERE_TRUE) {
                const int64_t raw = in ? static_cast<const int64_t*>(o.col)[i] : INT64_MIN;
                if (o.type == MLVDB_ATTR_INT64) {
                    const bool have = raw != INT64_MIN;
                    switch (o.op) {
                        case MLVDB_WHERE_EQ: bit = have && raw == o.a; break;
                        case MLVDB_WHERE_NE: bit = !(have && raw == o.a); break;
                        case MLVDB_WHERE_LT: bit = have && raw < o.a; break;
                        case MLVDB_WHERE_LE: bit = have && raw <= o.a; break;
                        case MLVDB_WHERE_GT: bit = have && raw > o.a; break;
                        case MLVDB_WHERE_GE: bit = have && raw >= o.a; break;
                        case MLVDB_WHERE_EXISTS: bit = have; break;
                        default: {  // MLVDB_WHERE_IN: binary search of set[a, a + b), sorted ascending
                            int64_t lo = o.a, hi = o.a + o.b;
                            while (lo < hi) {
                                const int64_t mid = lo + ((hi - lo) >> 1);
                                if (set[mid] < raw) lo = mid + 1; else hi = mid;
                            }
                            bit = have && lo < o.a + o.b && set[lo] == raw;
                        }
                    }
                } else {  // float64: absent = NaN, so every ordered comparison of an absent value is false by itself
                    const double v = __longlong_as_double(raw), a = __longlong_as_double(o.a);
                    switch (o.op) {
                        case MLVDB_WHERE_EQ: bit = v == a; break;
                        case MLVDB_WHERE_NE: bit = !(v == a); break;
                        case MLVDB_WHERE_LT: bit = v < a; break;
                        case MLVDB_WHERE_LE: bit = v <= a; break;
                        case MLVDB_WHERE_GT: bit = v > a; break;
                        case MLVDB_WHERE_GE: bit = v >= a; break;
                        default: bit = v == v;  // MLVDB_WHERE_EXISTS
                    }
                }
            }
            st = (st << 1) | (bit ? 1u : 0u);
        }
        const bool hit = in && (st & 1u) && rn[i] == rn[i];  // tombstoned rows (NaN norm) never match
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
