// The gathered walk: what where_gather_kernel, where_gather_range_kernel (kernels_where_each.hip) and grouped_gather_kernel
// (kernels_grouped.hip) share.  A block of kGatherWaves waves scores one interval of a list of int32 row labels against a
// tile of <= QT queries, with the arithmetic of the exact scan (scan_common.h), so a row scores bit-identically here and
// there.  A kernel resolves its tile's queries (qid[t], -1 = empty slot), stages them, picks its interval and hands every
// scored (slot, row) pair to its sink; the two top-k kernels end with the block merge.  Every function here is executed by
// the whole block (they hold barriers and full-wave operations).
#pragma once
#include "scan_common.h"

namespace mlvdb {

constexpr int kGatherWaves = 4;  // waves per block (256 threads), 16 labels each per step

// qs[t][0 .. ld) = query qid[t] of Qpad as fp64 (zeros for an empty slot), qinv[t] = its qaux; then the block's barrier.
// For a block of NW waves: the streamed scans (panel_walk.h) stage their tiles with it too.
// (qinv is read behind all the copies: read between them, it costs where_gather_kernel<cosine, 2> ten VGPRs and with them
// one of its four waves per SIMD.)
template <int QT, int NW = kGatherWaves>
__device__ __forceinline__ void gather_stage_queries(double* qs, const float* __restrict__ Qpad,
                                                     const double* __restrict__ qaux, const int (&qid)[QT], int ld,
                                                     double (&qinv)[QT]) {
#pragma unroll
    for (int t = 0; t < QT; ++t)
        for (int c = threadIdx.x; c < ld; c += NW * 64)
            qs[t * ld + c] = qid[t] >= 0 ? (double)Qpad[(int64_t)qid[t] * ld + c] : 0.0;
#pragma unroll
    for (int t = 0; t < QT; ++t) qinv[t] = qid[t] >= 0 ? qaux[qid[t]] : 0.0;
    __syncthreads();
}

// The rows labels[begin, end) against the staged tile: each wave gathers 16 rows per step with the panel addressing of
// pair_distance_kernel (lanes 16 g + r: row r, column slice g) and scores them with accumulate_rows / finish_distance.
// sink(t, have, dist, row) is called for every slot t of every step by all 64 lanes, never under a predicate (a sink may
// ballot and shuffle); `have`: this lane holds a row of the interval and is the one of its four lanes that reports it.
template <int SPACE, int QT, class Sink>
__device__ __forceinline__ void gather_walk(const float* __restrict__ X, const int32_t* __restrict__ labels, int64_t begin,
                                            int64_t end, const double* qs, int ld, const double (&qinv)[QT], Sink&& sink) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, r = lane & 15;
    for (int64_t j0 = begin + wave * 16; j0 < end; j0 += kGatherWaves * 16) {
        const int64_t j = j0 + r;
        const bool have = j < end;
        const bool mine = have && lane < 16;
        const int64_t row = have ? labels[j] : 0;  // (row 0 keeps the address valid)
        const float* base[1] = {X + (row >> 4) * (int64_t)(kPanelRows * ld) + (row & 15) * 16 + g * 4};
        double acc[1][QT], nx[1];
        accumulate_rows<SPACE, QT, 1, 8>(base, qs, ld, g, acc, nx);
#pragma unroll
        for (int t = 0; t < QT; ++t) sink(t, mine, finish_distance<SPACE>(acc[0][t], nx[0], qinv[t]), (int32_t)row);
    }
}

// The lists of all waves through LDS (smem: [waves][QT][64] distances, then as many labels; it aliases the query tile,
// hence the barrier first) into one list of k entries per filled slot: out(t)[0 .. k), the slot's partial list.
template <int QT, int NW = kGatherWaves, class Out>
__device__ __forceinline__ void gather_block_merge(char* smem, const WaveTopK (&top)[QT], const int (&qid)[QT], int k,
                                                   Out&& out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    double* ld_d = reinterpret_cast<double*>(smem);                                            // [NW][QT][64]
    int32_t* ld_l = reinterpret_cast<int32_t*>(smem + (size_t)NW * QT * 64 * sizeof(double));  // [NW][QT][64]
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        ld_d[(wave * QT + t) * 64 + lane] = top[t].d;
        ld_l[(wave * QT + t) * 64 + lane] = top[t].l;
    }
    __syncthreads();
    for (int t = wave; t < QT; t += NW) {
        if (qid[t] < 0) continue;  // (wave-uniform)
        WaveTopK m;
        m.init();
        for (int w2 = 0; w2 < NW; ++w2) {
            const double cd = ld_d[(w2 * QT + t) * 64 + lane];
            const int32_t cl = ld_l[(w2 * QT + t) * 64 + lane];
            m.offer(lane < k && cl != kNoLabel, cd, cl, k, lane);
        }
        if (lane < k) {
            TopEntry e;
            e.d = m.d;
            e.l = m.l;
            e.pad = 0;
            out(t)[lane] = e;
        }
    }
}

}  // namespace mlvdb
