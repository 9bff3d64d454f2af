// The streamed walk: what exact_scan_kernel, exact_range_kernel (kernels_exact.hip), distinct_scan_kernel
// (kernels_distinct.hip) and maxsim_scan_kernel (kernels_maxsim.hip) share -- the streamed counterpart of gather_walk.h,
// whose query staging and block merge it uses.  A block of NW waves streams its share of the row panels against a tile of
// <= QT queries with the arithmetic of scan_common.h.  A kernel resolves its tile's queries (qid[t], -1 = empty slot),
// stages them (gather_stage_queries<QT, NW>) and hands every scored (slot, row) pair to its sink.  Below it, the kernel
// that folds the partial lists of every top-k scan.  The device functions are executed by the whole block.
#pragma once
#include "gather_walk.h"

namespace mlvdb {

// Rows [0, row_end) of X against the staged tile: a wave takes PW panels of 16 rows per step, the steps of the nblk
// blocks (gridDim.x) interleaved wave by wave, and scores them with accumulate_rows<SPACE, QT, PW, PF, NT> /
// finish_distance.  Per panel row, every lane first calls st = row_state(row, in) -- `in`: this lane holds a row of the
// range and is the one of its four lanes that reports it; the kernel reads the row's liveness there, once per row -- and
// then sink(t, st, dist, row) for every slot t.  Both are called by all 64 lanes, never under a predicate (a sink may
// ballot and shuffle).
template <int SPACE, int QT, int PW, int NW, int PF, bool NT, class RowState, class Sink>
__device__ __forceinline__ void panel_walk(const float* __restrict__ X, int ld, int64_t row_end, int nblk, const double* qs,
                                           const double (&qinv)[QT], RowState&& row_state, Sink&& sink) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, r = lane & 15;
    const int64_t panel_end = (row_end + 15) >> 4;
    const int64_t ntasks = (panel_end + PW - 1) / PW;
    for (int64_t task = (int64_t)blockIdx.x * NW + wave; task < ntasks; task += (int64_t)nblk * NW) {
        const float* base[PW];
        int64_t panel[PW];
#pragma unroll
        for (int p = 0; p < PW; ++p) {
            panel[p] = task * PW + p;
            const int64_t pp = panel[p] < panel_end ? panel[p] : 0;  // keep the address valid
            base[p] = X + pp * (int64_t)(kPanelRows * ld) + lane_group_offset(lane);
        }
        double acc[PW][QT];
        double nx[PW];
        accumulate_rows<SPACE, QT, PW, PF, NT>(base, qs, ld, g, acc, nx);
#pragma unroll
        for (int p = 0; p < PW; ++p) {
            const int64_t row = panel[p] * kPanelRows + r;
            const auto st = row_state(row, lane < 16 && panel[p] < panel_end && row < row_end);
#pragma unroll
            for (int t = 0; t < QT; ++t) sink(t, st, finish_distance<SPACE>(acc[p][t], nx[p], qinv[t]), (int32_t)row);
        }
    }
}

// The live-row state of the three kernels that read the norms: in && rn[row] is no NaN (NaN marks a tombstoned or
// masked-out row).
__device__ __forceinline__ bool panel_row_live(const float* __restrict__ rn, int64_t row, bool in) {
    if (in) {
        const float nrm = rn[row];
        in = nrm == nrm;
    }
    return in;
}

// One block (4 waves) per selected query: each wave folds a quarter of the nblk x k partial entries, wave 0 folds the four
// lists and writes the final answer at the original query index.  NEGATE: the entries hold (-score, row) and the outputs
// are the scores again (a zero comes out as +0.0), padded with -inf -- the sparse search's merge.
template <bool NEGATE>
__global__ __launch_bounds__(256) void exact_merge_kernel(const TopEntry* __restrict__ partial, const int32_t* nq_sel_dev,
                                                          const int32_t* qsel, int32_t nblk, int32_t k, int64_t* out_labels,
                                                          float* out_dist, int32_t* out_counts, double* out_d64) {
    __shared__ double sd[4][64];
    __shared__ int32_t sl[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sel = blockIdx.x;
    if (nq_sel_dev && sel >= *nq_sel_dev) return;
    const int q = qsel ? qsel[sel] : sel;
    const TopEntry* src = partial + (int64_t)sel * nblk * k;
    const int64_t n = (int64_t)nblk * k;
    WaveTopK m;
    m.init();
    for (int64_t i0 = (int64_t)wave * 64; i0 < n; i0 += 256) {
        const int64_t i = i0 + lane;
        TopEntry e;
        e.d = __builtin_inf();
        e.l = kNoLabel;
        if (i < n) e = src[i];
        m.offer(e.l != kNoLabel, e.d, e.l, k, lane);
    }
    sd[wave][lane] = m.d;
    sl[wave][lane] = m.l;
    __syncthreads();
    if (wave != 0) return;
    WaveTopK f;
    f.init();
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
        const double cd = sd[w2][lane];
        const int32_t cl = sl[w2][lane];
        f.offer(lane < k && cl != kNoLabel, cd, cl, k, lane);
    }
    const bool valid = lane < k && f.l != kNoLabel;
    if (lane < k) {
        const double d = NEGATE ? -f.d : f.d, pad = NEGATE ? -__builtin_inf() : __builtin_inf();
        out_labels[(int64_t)q * k + lane] = valid ? (int64_t)f.l : -1;
        out_dist[(int64_t)q * k + lane] = valid ? (float)d : (float)pad;
        if (out_d64) out_d64[(int64_t)q * k + lane] = valid ? d : pad;
    }
    const int cnt = __popcll(__ballot(valid));
    if (lane == 0) out_counts[q] = cnt;
}

}  // namespace mlvdb
