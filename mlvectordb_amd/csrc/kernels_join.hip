// Similarity join (include/mlvdb_join.h): the kernels around the range passes of a wave of <= 256 left rows.
//   join_gather_queries_kernel   one 256-thread block per left row: its stored fp32 values from the panel layout (layout.h)
//                                to the dense [n, dim] batch the range passes prepare like any query sent from the host.
//   join_mask_advance_kernel     LATER: the labels [lo, hi) -- the rows below the wave's first label that the previous wave
//                                still saw -- become NaN in the masked norms and, when the int8 shadow serves the call, in
//                                the masked row pairs (an l2 pair keeps its x slot, the group's scale: mask_pairs_kernel).
//   join_strip_kernel            one 256-thread block per left row over its ranked list (<= cap_eff entries): the entries
//                                with label == a (OTHERS) or <= a (LATER) are dropped, the order kept -- a ballot per
//                                wavefront and the four wave counts through LDS give every kept entry its position behind a
//                                running base -- the first `capacity` survivors go to the wave's dense outputs.  The exact
//                                count is the number of survivors when the list is whole; a truncated list (count > cap_eff)
//                                can only be missing the row itself when nothing but the row can be in the way (OTHERS, or
//                                the first row of a LATER wave): count = inner count - [a is a hit], the latter from the
//                                pair-distance arithmetic on (a, a), whose bits are the range search's.  Any other
//                                truncated row is flagged: the driver runs it again at the head of a wave of its own.
//   join_pack_kernel             one block per left row: its kept entries from the dense outputs into the call's packed
//                                array behind `base` + the kept counts of the wave's resolved rows before it.
// No atomics, no scratch; every branch around a ballot or a barrier is uniform over the block.
#include "internal.h"

namespace mlvdb {

__global__ __launch_bounds__(256) void join_gather_queries_kernel(const float* __restrict__ X,
                                                                  const int64_t* __restrict__ labels, const int32_t dim,
                                                                  const int32_t ld, float* __restrict__ out) {
    const int64_t i = blockIdx.x;
    const float* row = X + layout_offset(labels[i], 0, ld);
    for (int c = threadIdx.x; c < dim; c += 256) out[i * dim + c] = row[(int64_t)(c >> 4) * kGroupFloats + (c & 15)];
}

__global__ __launch_bounds__(256) void join_mask_advance_kernel(float* __restrict__ rn, float2* __restrict__ rp, const int l2,
                                                                const int64_t lo, const int64_t hi) {
    const float nan = __builtin_nanf("");
    for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (int64_t)gridDim.x * blockDim.x) {
        rn[i] = nan;
        if (rp) rp[i] = make_float2(l2 ? rp[i].x : nan, nan);
    }
}

__global__ __launch_bounds__(256) void join_strip_kernel(const int64_t* __restrict__ l_lab, const float* __restrict__ l_dist,
                                                         const int64_t* __restrict__ l_cnt, const int64_t cap_eff,
                                                         const int64_t* __restrict__ left, const int32_t mode,
                                                         const double* __restrict__ self64, const float radius,
                                                         const float* __restrict__ rn, const int64_t capacity,
                                                         int64_t* __restrict__ out_labels, float* __restrict__ out_dist,
                                                         int64_t* __restrict__ out_count, int32_t* __restrict__ out_kept,
                                                         int32_t* __restrict__ out_flag) {
    __shared__ int wave_kept[4];
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t a = left[i];
    const int64_t cnt = l_cnt[i] > 0 ? l_cnt[i] : 0;
    const int64_t n = cnt < cap_eff ? cnt : cap_eff;  // entries of the list
    const int64_t l0 = i * cap_eff, o0 = i * capacity;
    int64_t kept = 0;  // survivors so far: the running base of the compaction (the same in every thread)
    for (int64_t e0 = 0; e0 < n; e0 += 256) {
        const int64_t e = e0 + threadIdx.x;
        const bool have = e < n;
        const int64_t lab = have ? l_lab[l0 + e] : -1;
        const bool keep = have && (mode == MLVDB_JOIN_LATER ? lab > a : lab != a);
        const unsigned long long votes = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(votes);
        __syncthreads();
        int64_t pos = kept + __popcll(votes & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += wave_kept[w];
        if (keep && pos < capacity) {
            out_labels[o0 + pos] = lab;
            out_dist[o0 + pos] = l_dist[l0 + e];
        }
        kept += wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
        __syncthreads();  // (the next round writes wave_kept again)
    }
    if (threadIdx.x == 0) {
        const bool truncated = cnt > cap_eff;
        const bool alone = mode == MLVDB_JOIN_OTHERS || i == 0;  // nothing but the row itself can be in the way
        int64_t count = kept;
        if (truncated && alone) {
            // a NaN norm: tombstoned or masked out, never a hit; a NaN distance fails the test like the range search's
            const bool self_hit = self64 && rn[a] == rn[a] && self64[i] <= (double)radius;
            count = cnt - (self_hit ? 1 : 0);
        }
        out_count[i] = count;
        out_kept[i] = (int32_t)(kept < capacity ? kept : capacity);
        out_flag[i] = truncated && !alone ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void join_pack_kernel(const int64_t* __restrict__ d_lab, const float* __restrict__ d_dist,
                                                        const int32_t* __restrict__ kept, const int32_t* __restrict__ flag,
                                                        const int64_t capacity, const int64_t base,
                                                        int64_t* __restrict__ p_lab, float* __restrict__ p_dist) {
    __shared__ int wave_sum[4];
    const int i = blockIdx.x;  // (a wave has <= 256 rows: thread j looks at row j)
    int before = (int)threadIdx.x < i && !flag[threadIdx.x] ? kept[threadIdx.x] : 0;
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = before;
    __syncthreads();
    if (flag[i]) return;  // (uniform over the block; no barrier follows)
    const int64_t at = base + wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    const int n = kept[i];
    for (int e = threadIdx.x; e < n; e += 256) {
        p_lab[at + e] = d_lab[(int64_t)i * capacity + e];
        p_dist[at + e] = d_dist[(int64_t)i * capacity + e];
    }
}

hipError_t launch_join_gather_queries(const float* X, const int64_t* labels, int32_t n, int32_t dim, int32_t ld, float* out,
                                      hipStream_t s) {
    if (n <= 0) return hipSuccess;
    join_gather_queries_kernel<<<n, 256, 0, s>>>(X, labels, dim, ld, out);
    return hipGetLastError();
}

hipError_t launch_join_mask_advance(float* rn, float* rp8, int l2, int64_t lo, int64_t hi, hipStream_t s) {
    if (hi <= lo) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((hi - lo + 255) / 256, 256 * 16);
    join_mask_advance_kernel<<<(unsigned)blocks, 256, 0, s>>>(rn, reinterpret_cast<float2*>(rp8), l2, lo, hi);
    return hipGetLastError();
}

hipError_t launch_join_strip(const int64_t* l_lab, const float* l_dist, const int64_t* l_cnt, int64_t cap_eff,
                             const int64_t* left, int32_t n, int32_t mode, const double* self64, float radius, const float* rn,
                             int64_t capacity, int64_t* out_labels, float* out_dist, int64_t* out_count, int32_t* out_kept,
                             int32_t* out_flag, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    join_strip_kernel<<<n, 256, 0, s>>>(l_lab, l_dist, l_cnt, cap_eff, left, mode, self64, radius, rn, capacity, out_labels,
                                        out_dist, out_count, out_kept, out_flag);
    return hipGetLastError();
}

hipError_t launch_join_pack(const int64_t* d_lab, const float* d_dist, const int32_t* kept, const int32_t* flag, int32_t n,
                            int64_t capacity, int64_t base, int64_t* p_lab, float* p_dist, hipStream_t s) {
    if (n <= 0 || n > kJoinWave) return n <= 0 ? hipSuccess : hipErrorInvalidValue;
    join_pack_kernel<<<n, 256, 0, s>>>(d_lab, d_dist, kept, flag, capacity, base, p_lab, p_dist);
    return hipGetLastError();
}

}  // namespace mlvdb
