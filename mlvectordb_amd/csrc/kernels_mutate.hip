// The write side of the attribute columns (include/mlvdb_mutate.h): values scattered to labelled rows, assignments applied
// to the rows a predicate program matches, and the tombstones of a filtered delete.  Programs, labels and assignments reach
// these kernels validated (api.hip), so nothing here checks them again.
#include <algorithm>

#include "internal.h"
#include "where_common.h"

namespace mlvdb {

namespace {
constexpr int kMutateMaxBlocks = 256 * 16;  // where_eval_kernel's cap: one stride covers 1,048,576 rows

inline unsigned mutate_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, kMutateMaxBlocks); }

// One wave's votes -> its lane 0's counter (every lane of the wave must call it).
__device__ __forceinline__ void wave_count(bool vote, int lane, unsigned long long& acc) {
    const unsigned long long b = __ballot(vote);
    if (lane == 0) acc += __popcll(b);
}
}  // namespace

// col[labels[j]] = values[j] for the live rows among the labels (distinct and inside [0, total): checked on the host);
// *updated += rows written.  One thread per label, grid-stride.
__global__ __launch_bounds__(256) void attr_scatter_kernel(int64_t* __restrict__ col, const int64_t* __restrict__ labels,
                                                           const int64_t* __restrict__ values, int64_t n,
                                                           const float* __restrict__ rn,
                                                           unsigned long long* __restrict__ updated) {
    __shared__ unsigned long long block_hits;
    if (threadIdx.x == 0) block_hits = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long wave_hits = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j0 = (int64_t)blockIdx.x * blockDim.x; j0 < n; j0 += stride) {  // j0 uniform over the block (ballot)
        const int64_t j = j0 + threadIdx.x;
        bool live = false;
        if (j < n) {
            const int64_t label = labels[j];
            live = rn[label] == rn[label];  // tombstoned rows keep what they hold
            if (live) col[label] = values[j];
        }
        wave_count(live, lane, wave_hits);
    }
    if (lane == 0 && wave_hits) atomicAdd(&block_hits, wave_hits);
    __syncthreads();
    if (threadIdx.x == 0 && block_hits) atomicAdd(updated, block_hits);
}

hipError_t launch_attr_scatter(int64_t* col, const int64_t* labels, const int64_t* values, int64_t n, const float* rn,
                               unsigned long long* updated, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    attr_scatter_kernel<<<mutate_blocks(n), 256, 0, s>>>(col, labels, values, n, rn, updated);
    return hipGetLastError();
}

// where_eval_kernel's shape with the stores fused in: one thread per row, grid-stride, the program and the assignments staged
// in LDS.  A row is evaluated fully (every column the program reads) before anything of it is stored, and an assignment reads
// only its own column at its own row, so the program's columns and the assigned columns may be the same memory: no column is
// reached through a __restrict__ or read-only-cached pointer here.  kStore == false is the counting pass of a call with
// ADDs: counters[0] += live matching rows, counters[1] += those of them with a sum that cannot be stored; nothing is
// written.  kStore == true counts the same and stores every storable value.
template <bool kStore>
__global__ __launch_bounds__(256) void attr_update_kernel(const WhereOp* __restrict__ prog, int32_t n_ops,
                                                          const int64_t* __restrict__ set, const MutateSet* __restrict__ sets,
                                                          int32_t n_sets, const float* __restrict__ rn, int64_t total,
                                                          unsigned long long* __restrict__ counters) {
    __shared__ WhereOp sp[kWhereMaxOps];
    __shared__ MutateSet ss[MLVDB_MAX_ATTRS];
    __shared__ unsigned long long block_hits, block_bad;
    if ((int)threadIdx.x < n_ops) sp[threadIdx.x] = prog[threadIdx.x];
    if ((int)threadIdx.x < n_sets) ss[threadIdx.x] = sets[threadIdx.x];
    if (threadIdx.x == 0) block_hits = block_bad = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long wave_hits = 0, wave_bad = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {  // i0 uniform over the block (ballot)
        const int64_t i = i0 + threadIdx.x;
        const bool in = i < total;
        const bool match = where_eval_row(sp, n_ops, set, i, in);
        const bool hit = in && match && rn[i] == rn[i];  // tombstoned rows (NaN norm) never match
        bool bad = false;
        for (int j = 0; j < n_sets; ++j) {  // uniform over the wave: what differs per lane is the row's value
            const MutateSet a = ss[j];
            if (a.op == MLVDB_SET_ASSIGN) {
                if (kStore && hit) a.col[i] = a.a;
                continue;
            }
            if (!hit) continue;
            const int64_t old = a.col[i];
            if (a.type == MLVDB_ATTR_INT64) {
                if (old == INT64_MIN) continue;  // absent stays absent
                long long sum;
                const bool over = __builtin_add_overflow((long long)old, (long long)a.a, &sum);
                if (over || sum == INT64_MIN)
                    bad = true;
                else if (kStore)
                    a.col[i] = sum;
            } else {
                const double v = __longlong_as_double(old);
                if (v != v) continue;
                const double sum = v + __longlong_as_double(a.a);
                if (sum != sum)
                    bad = true;
                else if (kStore)
                    a.col[i] = __double_as_longlong(sum);
            }
        }
        wave_count(hit, lane, wave_hits);
        wave_count(bad, lane, wave_bad);
    }
    if (lane == 0 && wave_hits) atomicAdd(&block_hits, wave_hits);
    if (lane == 0 && wave_bad) atomicAdd(&block_bad, wave_bad);
    __syncthreads();
    if (threadIdx.x == 0 && block_hits) atomicAdd(counters, block_hits);
    if (threadIdx.x == 0 && block_bad) atomicAdd(counters + 1, block_bad);
}

hipError_t launch_attr_update(const WhereOp* prog, int32_t n_ops, const int64_t* set, const MutateSet* sets, int32_t n_sets,
                              const float* rn, int64_t total, bool store, unsigned long long* counters, hipStream_t s) {
    if (total <= 0) return hipSuccess;
    if (store)
        attr_update_kernel<true><<<mutate_blocks(total), 256, 0, s>>>(prog, n_ops, set, sets, n_sets, rn, total, counters);
    else
        attr_update_kernel<false><<<mutate_blocks(total), 256, 0, s>>>(prog, n_ops, set, sets, n_sets, rn, total, counters);
    return hipGetLastError();
}

// The rows of `mask` become tombstones: rn = NaN and, for the rows the int8 shadow holds (i < i8_rows; 0: no shadow), their
// row pairs patched by tombstone_rp8_kernel's rule (the error / norm slot always, the scale slot unless the space is l2).
__global__ __launch_bounds__(256) void tombstone_mask_kernel(const uint8_t* __restrict__ mask, float* __restrict__ rn,
                                                             float* __restrict__ rp8, int64_t i8_rows, int l2, int64_t total) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        if (!mask[i]) continue;
        rn[i] = __uint_as_float(0x7fc00000u);  // the NaN tombstone_kernel writes
        if (i < i8_rows) {
            rp8[2 * i + 1] = __builtin_nanf("");
            if (!l2) rp8[2 * i] = __builtin_nanf("");
        }
    }
}

hipError_t launch_tombstone_mask(const uint8_t* mask, float* rn, float* rp8, int64_t i8_rows, int l2, int64_t total,
                                 hipStream_t s) {
    if (total <= 0) return hipSuccess;
    tombstone_mask_kernel<<<mutate_blocks(total), 256, 0, s>>>(mask, rn, rp8, rp8 ? i8_rows : 0, l2, total);
    return hipGetLastError();
}

}  // namespace mlvdb
