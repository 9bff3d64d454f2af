// Facet counts and histograms of attribute columns (include/mlvdb_facet.h): one pass over the norms (liveness), the columns
// the predicate program reads and the faceted column.  The program is evaluated here (where_common.h), not read back from a
// row mask: the pass writes nothing per row.  Launch shape of where_eval_kernel: 256 threads, grid-stride, one row per thread
// and pass, i0 uniform over the block so that every ballot sees whole waves.
#include <algorithm>

#include "internal.h"
#include "wave_peel.h"
#include "where_common.h"

namespace mlvdb {

namespace {

constexpr unsigned long long kFacetEmpty = 0x8000000000000000ull;  // INT64_MIN: never a present value

// Open addressing, linear probing: the key is claimed by a 64-bit compare-and-swap, the count added behind it.
__device__ __forceinline__ bool lds_insert(unsigned long long* keys, uint32_t* counts, int64_t key, uint32_t n) {
    uint32_t s = (uint32_t)facet_hash(key) & (kFacetLdsSlots - 1);
    for (int p = 0; p < kFacetLdsProbes; ++p) {
        const unsigned long long prev = atomicCAS(&keys[s], kFacetEmpty, (unsigned long long)key);
        if (prev == kFacetEmpty || prev == (unsigned long long)key) {
            atomicAdd(&counts[s], n);
            return true;
        }
        s = (s + 1) & (kFacetLdsSlots - 1);
    }
    return false;
}

// ... in HBM: whoever claims an empty slot counts one more distinct value (exact while the table is not full).  Once more
// than max_values are counted the call is an overflow whatever follows, so further inserts are dropped; a full table flags
// the overflow itself.
__device__ __forceinline__ void global_insert(const FacetTable& t, int64_t key, unsigned long long n) {
    if (__hip_atomic_load(&t.ctr[kFacetDistinct], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > t.max_values) return;
    uint64_t s = facet_hash(key) & t.mask;
    for (uint64_t p = 0; p <= t.mask; ++p) {
        const unsigned long long prev = atomicCAS(&t.keys[s], kFacetEmpty, (unsigned long long)key);
        if (prev == kFacetEmpty) atomicAdd(&t.ctr[kFacetDistinct], 1ull);
        if (prev == kFacetEmpty || prev == (unsigned long long)key) {
            atomicAdd(&t.counts[s], n);
            return;
        }
        s = (s + 1) & t.mask;
    }
    atomicOr(&t.ctr[kFacetOverflow], 1ull);
}

// row i: live and matching -> hit, its value of `col` -> raw (only loaded for a hit)
__device__ __forceinline__ bool facet_row(const WhereOp* sp, int32_t n_ops, const int64_t* __restrict__ set,
                                          const float* __restrict__ rn, const int64_t* __restrict__ col, int64_t i,
                                          int64_t total, int64_t& raw) {
    const bool in = i < total;
    const bool live = in && rn[i] == rn[i];  // tombstoned rows (NaN norm) never count
    const bool hit = live && (n_ops == 0 || where_eval_row(sp, n_ops, set, i, live));
    raw = hit ? col[i] : INT64_MIN;
    return hit;
}

}  // namespace

__global__ __launch_bounds__(256) void facet_values_kernel(const WhereOp* __restrict__ prog, int32_t n_ops,
                                                           const int64_t* __restrict__ set, const float* __restrict__ rn,
                                                           const int64_t* __restrict__ col, int64_t total, FacetTable t) {
    __shared__ WhereOp sp[kWhereMaxOps];
    __shared__ unsigned long long lkeys[kFacetLdsSlots];
    __shared__ uint32_t lcounts[kFacetLdsSlots];
    __shared__ unsigned long long block_matched, block_absent;
    if ((int)threadIdx.x < n_ops) sp[threadIdx.x] = prog[threadIdx.x];
    for (int s = threadIdx.x; s < kFacetLdsSlots; s += blockDim.x) {
        lkeys[s] = kFacetEmpty;
        lcounts[s] = 0;
    }
    if (threadIdx.x == 0) block_matched = block_absent = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long wave_matched = 0, wave_absent = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        int64_t v;
        const bool hit = facet_row(sp, n_ops, set, rn, col, i0 + threadIdx.x, total, v);
        const bool has = hit && v != INT64_MIN;
        const unsigned long long bh = __ballot(hit), ba = __ballot(hit && !has);
        if (lane == 0) {
            wave_matched += __popcll(bh);
            wave_absent += __popcll(ba);
        }
        wave_peel_add(has, v, [&](int64_t key, uint32_t n) {
            if (!lds_insert(lkeys, lcounts, key, n)) global_insert(t, key, n);
        });
    }
    if (lane == 0 && wave_matched) atomicAdd(&block_matched, wave_matched);
    if (lane == 0 && wave_absent) atomicAdd(&block_absent, wave_absent);
    __syncthreads();
    for (int s = threadIdx.x; s < kFacetLdsSlots; s += blockDim.x)
        if (lkeys[s] != kFacetEmpty) global_insert(t, (int64_t)lkeys[s], lcounts[s]);
    if (threadIdx.x == 0 && block_matched) atomicAdd(&t.ctr[kFacetMatched], block_matched);
    if (threadIdx.x == 0 && block_absent) atomicAdd(&t.ctr[kFacetAbsent], block_absent);
}

hipError_t launch_facet_values(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* col,
                               int64_t total, const FacetTable& t, hipStream_t s) {
    if (total == 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    facet_values_kernel<<<(unsigned)blocks, 256, 0, s>>>(prog, n_ops, set, rn, col, total, t);
    return hipGetLastError();
}

// The value kernel over a list column (include/mlvdb_list.h): `col` holds slots into `pool`, and a hit row counts once under
// every value of its list.  Step j of the walk peels the j-th values of the wave's rows together; the walk is as long as the
// wave's longest list (the bound is a ballot, so every lane runs every round the peel's ballots need).
__global__ __launch_bounds__(256) void facet_list_values_kernel(const WhereOp* __restrict__ prog, int32_t n_ops,
                                                                const int64_t* __restrict__ set, const float* __restrict__ rn,
                                                                const int64_t* __restrict__ col,
                                                                const int64_t* __restrict__ pool, int64_t total, FacetTable t) {
    __shared__ WhereOp sp[kWhereMaxOps];
    __shared__ unsigned long long lkeys[kFacetLdsSlots];
    __shared__ uint32_t lcounts[kFacetLdsSlots];
    __shared__ unsigned long long block_matched, block_absent;
    if ((int)threadIdx.x < n_ops) sp[threadIdx.x] = prog[threadIdx.x];
    for (int s = threadIdx.x; s < kFacetLdsSlots; s += blockDim.x) {
        lkeys[s] = kFacetEmpty;
        lcounts[s] = 0;
    }
    if (threadIdx.x == 0) block_matched = block_absent = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long wave_matched = 0, wave_absent = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        int64_t slot;
        const bool hit = facet_row(sp, n_ops, set, rn, col, i0 + threadIdx.x, total, slot);
        const int len = slot == INT64_MIN ? 0 : (int)(slot & 0xff);  // (no hit: INT64_MIN)
        const int64_t* lp = pool + (slot >> 8);                      // (never read when len == 0)
        const unsigned long long bh = __ballot(hit), ba = __ballot(hit && len == 0);
        if (lane == 0) {
            wave_matched += __popcll(bh);
            wave_absent += __popcll(ba);
        }
        for (int j = 0; __ballot(j < len); ++j) {
            const bool has = j < len;
            const int64_t v = has ? lp[j] : INT64_MIN;
            wave_peel_add(has, v, [&](int64_t key, uint32_t n) {
                if (!lds_insert(lkeys, lcounts, key, n)) global_insert(t, key, n);
            });
        }
    }
    if (lane == 0 && wave_matched) atomicAdd(&block_matched, wave_matched);
    if (lane == 0 && wave_absent) atomicAdd(&block_absent, wave_absent);
    __syncthreads();
    for (int s = threadIdx.x; s < kFacetLdsSlots; s += blockDim.x)
        if (lkeys[s] != kFacetEmpty) global_insert(t, (int64_t)lkeys[s], lcounts[s]);
    if (threadIdx.x == 0 && block_matched) atomicAdd(&t.ctr[kFacetMatched], block_matched);
    if (threadIdx.x == 0 && block_absent) atomicAdd(&t.ctr[kFacetAbsent], block_absent);
}

hipError_t launch_facet_list_values(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* col,
                                    const int64_t* pool, int64_t total, const FacetTable& t, hipStream_t s) {
    if (total == 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    facet_list_values_kernel<<<(unsigned)blocks, 256, 0, s>>>(prog, n_ops, set, rn, col, pool, total, t);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void facet_collect_kernel(FacetTable t, long long* __restrict__ out_keys,
                                                            unsigned long long* __restrict__ out_counts) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = t.keys[s];
        if (key == kFacetEmpty) continue;
        const unsigned long long at = atomicAdd(&t.ctr[kFacetCursor], 1ull);
        if (at < t.max_values) {  // (an overflowed table may hold more: its arrays are unspecified, never out of bounds)
            out_keys[at] = (long long)key;
            out_counts[at] = t.counts[s];
        }
    }
}

hipError_t launch_facet_collect(const FacetTable& t, long long* out_keys, unsigned long long* out_counts, hipStream_t s) {
    const int64_t blocks = std::min<int64_t>(((int64_t)t.mask + 256) / 256, 256 * 16);
    facet_collect_kernel<<<(unsigned)blocks, 256, 0, s>>>(t, out_keys, out_counts);
    return hipGetLastError();
}

// Dynamic LDS: n_edges edges (8 bytes each) then the block's n_edges + 1 bins.  The bin of a value is the number of edges
// <= it, found by a binary search of `steps` rounds for every lane (top = the largest power of two <= n_edges).
template <bool F64>
__global__ __launch_bounds__(256) void facet_bins_kernel(const WhereOp* __restrict__ prog, int32_t n_ops,
                                                         const int64_t* __restrict__ set, const float* __restrict__ rn,
                                                         const int64_t* __restrict__ col, int64_t total,
                                                         const int64_t* __restrict__ edges, int32_t n_edges, int32_t top,
                                                         unsigned long long* __restrict__ bins,
                                                         unsigned long long* __restrict__ ctr) {
    extern __shared__ unsigned long long facet_lds[];
    __shared__ WhereOp sp[kWhereMaxOps];
    __shared__ unsigned long long block_matched, block_absent;
    int64_t* le = reinterpret_cast<int64_t*>(facet_lds);
    uint32_t* lbins = reinterpret_cast<uint32_t*>(le + n_edges);
    if ((int)threadIdx.x < n_ops) sp[threadIdx.x] = prog[threadIdx.x];
    for (int s = threadIdx.x; s < n_edges; s += blockDim.x) le[s] = edges[s];
    for (int s = threadIdx.x; s <= n_edges; s += blockDim.x) lbins[s] = 0;
    if (threadIdx.x == 0) block_matched = block_absent = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    unsigned long long wave_matched = 0, wave_absent = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        int64_t raw;
        const bool hit = facet_row(sp, n_ops, set, rn, col, i0 + threadIdx.x, total, raw);
        const double dv = __longlong_as_double(raw);
        const bool has = hit && (F64 ? dv == dv : raw != INT64_MIN);
        const unsigned long long bh = __ballot(hit), ba = __ballot(hit && !has);
        if (lane == 0) {
            wave_matched += __popcll(bh);
            wave_absent += __popcll(ba);
        }
        int bin = 0;
        for (int step = top; step > 0; step >>= 1) {
            const int p = bin + step;
            if (p <= n_edges) {
                const int64_t e = le[p - 1];
                if (F64 ? __longlong_as_double(e) <= dv : e <= raw) bin = p;
            }
        }
        wave_peel_add(has, (int64_t)bin, [&](int64_t b, uint32_t n) { atomicAdd(&lbins[b], n); });
    }
    if (lane == 0 && wave_matched) atomicAdd(&block_matched, wave_matched);
    if (lane == 0 && wave_absent) atomicAdd(&block_absent, wave_absent);
    __syncthreads();
    for (int s = threadIdx.x; s <= n_edges; s += blockDim.x)
        if (lbins[s]) atomicAdd(&bins[s], (unsigned long long)lbins[s]);
    if (threadIdx.x == 0 && block_matched) atomicAdd(&ctr[kFacetMatched], block_matched);
    if (threadIdx.x == 0 && block_absent) atomicAdd(&ctr[kFacetAbsent], block_absent);
}

hipError_t launch_facet_bins(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* col,
                             int32_t type, int64_t total, const int64_t* edges, int32_t n_edges, unsigned long long* bins,
                             unsigned long long* ctr, hipStream_t s) {
    if (total == 0) return hipSuccess;
    static std::atomic<uint64_t> configured_i64{0}, configured_f64{0};
    const bool f64 = type == MLVDB_ATTR_FLOAT64;
    const void* kernel = f64 ? reinterpret_cast<const void*>(&facet_bins_kernel<true>)
                             : reinterpret_cast<const void*>(&facet_bins_kernel<false>);
    // the largest request (4096 edges: 49,156 bytes) is above 48 KiB
    const int max_lds = kFacetMaxEdges * (int)sizeof(int64_t) + (kFacetMaxEdges + 1) * (int)sizeof(uint32_t);
    if (hipError_t e = ensure_dynamic_lds(f64 ? configured_f64 : configured_i64, kernel, max_lds)) return e;
    const size_t lds = (size_t)n_edges * sizeof(int64_t) + ((size_t)n_edges + 1) * sizeof(uint32_t);
    int32_t top = 1;
    while (top * 2 <= n_edges) top *= 2;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    if (f64)
        facet_bins_kernel<true><<<(unsigned)blocks, 256, lds, s>>>(prog, n_ops, set, rn, col, total, edges, n_edges, top, bins, ctr);
    else
        facet_bins_kernel<false><<<(unsigned)blocks, 256, lds, s>>>(prog, n_ops, set, rn, col, total, edges, n_edges, top, bins, ctr);
    return hipGetLastError();
}

}  // namespace mlvdb
