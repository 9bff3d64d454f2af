// Clustering (include/mlvdb_cluster.h): nearest-centroid assignment, the ordered member lists and the blocked sums.
//   assign_scan_kernel     exact_scan_kernel's shape, geometry and arithmetic -- plan_exact's tiles, gather_stage_queries,
//                          panel_walk; accumulate_rows / finish_distance give every d_j the scans' bits.  One launch works on
//                          ONE tile of up to QT centroids and folds them, j ascending, into (best, idx) in two registers:
//                          panel_walk hands the sink the slots of a row back to back.  The tiles of an assignment are walked
//                          by successive launches in ascending order, so "the lower j wins a tie" holds across them: every
//                          tile but the first loads (best, idx) of its row, every tile but the last stores it -- one lane
//                          per row, 12 B, coalesced -- and the last writes the final pair, compares idx with the previous
//                          iteration's and counts the rows that moved: ballot / popcount per row step into a register, one
//                          integer atomic per wave at the end.  No list, no merge.
//   cluster_weight_kernel  cosine k-means: w(x) = 1 / (sqrt(nx) + 1e-30) of every row, nx summed in accumulate_rows' order.
//   cluster_hist_kernel    the listing is a stable counting sort by cluster id: one wave per kClusterListRows rows counts its
//   cluster_offsets_kernel rows per cluster (integer LDS atomics: a count has no order); one block turns the [block][cluster]
//   cluster_fill_kernel    counts into each block's first slot inside its cluster, the member counts and the clusters' bases;
//                          the same waves walk their rows again in order and rank the rows of one cluster inside a step by
//                          a ballot, so every cluster's members come out in ascending label order.
//   cluster_sum_kernel     one wave per (segment, 64-column slice), one lane per column: the segment's members in order, the
//                          row's 64-byte group pieces through layout.h's addressing (16 lanes per piece, every byte of each
//                          sector used), one fp64 add per member in a register -> the segment's partial.  The slice behind
//                          the last column is the cost: the members' best distances, folded in the same order.
//   cluster_finish_kernel  per (cluster, column) the partials of its segments in order, the division, the rounding to fp32; a
//                          cluster without members keeps its centroid.
//   cluster_write_kernel   the assignment into the int64 column, plain vector stores.
// Everything that sums is fp64, one rounded operation per step in the order the header states (the library is built with
// -ffp-contract=off, restated below for this file).  The only atomics are integer counters.  No scratch.
#include <algorithm>

#include "internal.h"
#include "panel_walk.h"

#pragma clang fp contract(off)

namespace mlvdb {

constexpr int kClusterListThreads = 64;  // one wave per listing block: the fill kernel ranks a step's rows by lane
static_assert(kClusterListThreads == 64, "cluster_hist_kernel / cluster_fill_kernel walk 64 rows per step, one per lane of one wave");

template <int SPACE, int QT, int PW, int NW>
__global__ __launch_bounds__(NW * 64) void assign_scan_kernel(const AssignArgs a, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    const int lane = threadIdx.x & 63;
    const int r = lane & 15;
    int qid[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) qid[t] = a.first + t < a.m ? a.first + t : -1;
    double qinv[QT];
    gather_stage_queries<QT, NW>(qs, a.Qpad, a.qaux, qid, a.ld, qinv);  // (ends with the barrier)
    if (SPACE == kSpaceCosine) {  // (per lane, as in examples_scan_kernel: the scalar registers are the scarce ones)
#pragma unroll
        for (int t = 0; t < QT; ++t) qinv[t] = lane_read(qinv[t], lane);
    }
    const int nvalid = a.m - a.first;  // slots t < nvalid hold a centroid; an empty slot's distance never takes part
    const bool first = a.flags & kClusterFirst, last = a.flags & kClusterLast;
    const int32_t base = a.first;
    const float* const rn_r = a.rn + r;
    double* const best_r = a.best + r;
    int32_t* const sidx_r = a.sidx + r;
    int32_t* const assign_r = a.assign + r;

    double best = __builtin_inf();
    int32_t idx = -1;
    uint32_t nmoved = 0;
    // (no prefetch banks, as in examples_scan_kernel: their block counters and clamps are scalars)
    panel_walk<SPACE, QT, PW, NW, 0, /*NT=*/true>(
        a.X, a.ld, a.total, nblk, qs, qinv,
        [&](int64_t row, bool in) {
            const bool live = panel_row_live(rn_r, row - r, in);
            best = __builtin_inf();
            idx = -1;
            if (!first && live) {  // what the tile before left
                best = best_r[row - r];
                idx = sidx_r[row - r];
            }
            return live;
        },
        [&](int t, bool live, double dist, int32_t row) {
            if (t < nvalid && dist < best) {  // (a NaN compares false: it never wins)
                best = dist;
                idx = base + t;
            }
            if (t != QT - 1) return;
            if (!last) {  // (block-uniform)
                if (live) {
                    best_r[row - r] = best;
                    sidx_r[row - r] = idx;
                }
                return;
            }
            bool moved = false;
            if (live) {
                moved = assign_r[row - r] != idx;
                assign_r[row - r] = idx;
                best_r[row - r] = best;
            }
            nmoved += (uint32_t)__popcll(__ballot(moved));
        });
    if (last && lane == 0 && nmoved) atomicAdd(a.moved, (unsigned long long)nmoved);
}

// One wave per panel of 16 rows, lane 16 g + r on row r and column slice g: accumulate_rows' nx -- per lane the squares of
// its four columns of every group in order (a square of an fp32 value is exact in fp64, so the fma is a plain add), then
// (g0 + g1) + (g2 + g3).
__global__ __launch_bounds__(256) void cluster_weight_kernel(const float* __restrict__ X, const int32_t ld, const int64_t total,
                                                             double* __restrict__ w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t panel = (int64_t)blockIdx.x * 4 + wave;
    if (panel * kPanelRows >= total) return;  // (wave-uniform; no barrier below)
    const float* base = X + panel * (int64_t)(kPanelRows * ld) + lane_group_offset(lane);
    double nx = 0.0;
    for (int kb = 0; kb < (ld >> 4); ++kb) {
        const float4 x = *reinterpret_cast<const float4*>(base + (int64_t)kb * kGroupFloats);
        nx = __builtin_fma((double)x.x, (double)x.x, nx);
        nx = __builtin_fma((double)x.y, (double)x.y, nx);
        nx = __builtin_fma((double)x.z, (double)x.z, nx);
        nx = __builtin_fma((double)x.w, (double)x.w, nx);
    }
    nx += __shfl_xor(nx, 16);
    nx += __shfl_xor(nx, 32);
    const int64_t row = panel * kPanelRows + (lane & 15);
    if (lane < 16 && row < total) w[row] = 1.0 / (__builtin_sqrt(nx) + 1e-30);
}

// ------------------------------------------------------------------------------ the ordered member lists
__global__ __launch_bounds__(kClusterListThreads) void cluster_hist_kernel(const int32_t* __restrict__ assign, const int64_t total, const int32_t m,
                                                          int32_t* __restrict__ hist, unsigned long long* matched) {
    __shared__ int32_t cnt[kClusterMax];
    const int lane = threadIdx.x;
    for (int c = lane; c < m; c += 64) cnt[c] = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * kClusterListRows, r1 = r0 + kClusterListRows < total ? r0 + kClusterListRows : total;
    uint32_t ncand = 0;
    for (int64_t row0 = r0; row0 < r1; row0 += 64) {
        const int64_t row = row0 + lane;
        const int32_t c = row < r1 ? assign[row] : kClusterNoCandidate;
        ncand += (uint32_t)__popcll(__ballot(c != kClusterNoCandidate));
        if (c >= 0 && c < m) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    for (int c = lane; c < m; c += 64) hist[(int64_t)blockIdx.x * m + c] = cnt[c];
    if (lane == 0 && ncand) atomicAdd(matched, (unsigned long long)ncand);
}

// One block, thread c on cluster c: hist[b][c] becomes block b's first slot inside cluster c (the exclusive running sum over
// the blocks), counts[c] the members of c, base[c] the exclusive sum of the counts over the clusters.
__global__ __launch_bounds__(kClusterMax) void cluster_offsets_kernel(int32_t* __restrict__ hist, const int64_t nblocks,
                                                                      const int32_t m, int64_t* __restrict__ counts,
                                                                      int64_t* __restrict__ base) {
    __shared__ int64_t scan[2][kClusterMax];
    const int c = threadIdx.x;
    int64_t running = 0;
    if (c < m) {
        for (int64_t b = 0; b < nblocks; ++b) {
            const int32_t v = hist[b * m + c];
            hist[b * m + c] = (int32_t)running;  // (a cluster holds fewer than 2^31 rows: check_row_limit)
            running += v;
        }
        counts[c] = running;
    }
    int from = 0;
    scan[0][c] = c < m ? running : 0;
    __syncthreads();
    for (int step = 1; step < kClusterMax; step <<= 1) {  // (inclusive Hillis-Steele over the counts)
        scan[from ^ 1][c] = scan[from][c] + (c >= step ? scan[from][c - step] : 0);
        from ^= 1;
        __syncthreads();
    }
    if (c < m) base[c] = scan[from][c] - running;
}

// (a block is ONE wave -- launch_cluster_list launches kClusterListThreads = 64 threads: lane order is label order, and the
// ballots see every row of a step)
__global__ __launch_bounds__(kClusterListThreads) void cluster_fill_kernel(const int32_t* __restrict__ assign, const int64_t total, const int32_t m,
                                                          const int32_t* __restrict__ hist, const int64_t* __restrict__ base,
                                                          int32_t* __restrict__ members) {
    __shared__ int64_t cur[kClusterMax];  // the next free slot of every cluster for this block's rows
    const int lane = threadIdx.x;
    for (int c = lane; c < m; c += 64) cur[c] = base[c] + hist[(int64_t)blockIdx.x * m + c];
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * kClusterListRows, r1 = r0 + kClusterListRows < total ? r0 + kClusterListRows : total;
    for (int64_t row0 = r0; row0 < r1; row0 += 64) {
        const int64_t row = row0 + lane;
        const int32_t c = row < r1 ? assign[row] : kClusterNoCandidate;
        const bool todo = c >= 0 && c < m;
        unsigned long long pending = __ballot(todo);
        while (pending) {  // (wave-uniform) one cluster of this step per turn, its rows ranked by lane = by label
            const int leader = __ffsll((long long)pending) - 1;
            const int32_t cl = __shfl(c, leader);
            const unsigned long long same = __ballot(todo && c == cl);
            const int64_t at = cur[cl];  // (every lane reads before the leader moves it on)
            if (todo && c == cl) members[at + __popcll(same & ((1ull << lane) - 1ull))] = (int32_t)row;
            if (lane == leader) cur[cl] = at + __popcll(same);
            __syncthreads();  // the next turn may read this slot: the store is visible before any lane goes on
            pending &= ~same;
        }
    }
}

// ------------------------------------------------------------------------------ the blocked sums
template <bool COSINE>
__global__ __launch_bounds__(64) void cluster_sum_kernel(const float* __restrict__ X, const int32_t ld,
                                                         const ClusterSegment* __restrict__ segs,
                                                         const int32_t* __restrict__ members, const double* __restrict__ w,
                                                         const double* __restrict__ best, const int32_t first_slice,
                                                         const int32_t nslices, double* __restrict__ partial) {
    const int lane = threadIdx.x;
    const ClusterSegment seg = segs[blockIdx.x];
    const int32_t* const mem = members + seg.begin;
    double* const out = partial + (int64_t)blockIdx.x * (ld + 1);
    const int slice = (int)blockIdx.y + first_slice;
    if (slice == nslices) {  // (block-uniform) the cost: 64 best distances per load, folded lane by lane in member order
        double s = 0.0;
        for (int j0 = 0; j0 < seg.count; j0 += 64) {
            const int n = seg.count - j0 < 64 ? seg.count - j0 : 64;
            const double v = lane < n ? best[mem[j0 + lane]] : 0.0;
            for (int i = 0; i < n; ++i) s = s + __shfl(v, i);
        }
        if (lane == 0) out[ld] = s;
        return;
    }
    const int col = slice * 64 + lane;
    if (col >= ld) return;
    const float* const xc = X + (int64_t)(col >> 4) * kGroupFloats + (col & 15);  // layout_offset(row, col, ld) less the row's part
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < seg.count; ++j) {
        const int64_t row = mem[j];
        const double x = (double)xc[(row >> 4) * (int64_t)(kPanelRows * ld) + (row & 15) * 16];
        s = COSINE ? s + x * w[row] : s + x;
    }
    out[col] = s;
}

__global__ __launch_bounds__(256) void cluster_finish_kernel(const double* __restrict__ partial, const int32_t* __restrict__ seg_first,
                                                             const int64_t* __restrict__ counts, const int32_t dim, const int32_t ld,
                                                             const int32_t first_col, float* __restrict__ cent,
                                                             double* __restrict__ cost) {
    const int c = blockIdx.x;
    const int32_t s0 = seg_first[c], s1 = seg_first[c + 1];
    const int64_t n = counts[c];
    for (int col = first_col + threadIdx.x; col <= ld; col += 256) {
        double s = 0.0;
        for (int32_t g = s0; g < s1; ++g) s = s + partial[(int64_t)g * (ld + 1) + col];
        if (col == ld)
            cost[c] = s;
        else if (col < dim && n > 0)
            cent[(int64_t)c * dim + col] = (float)(s / (double)n);
    }
}

__global__ __launch_bounds__(256) void cluster_write_kernel(const int32_t* __restrict__ assign, const int64_t total,
                                                            int64_t* __restrict__ column) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= total) return;
    const int32_t c = assign[row];
    if (c != kClusterNoCandidate) column[row] = c >= 0 ? (int64_t)c : INT64_MIN;
}

// ------------------------------------------------------------------------------ host side
ExactPlan plan_assign(int64_t nrows, int32_t ld, int32_t qt) {
    // plan_exact for one tile of qt queries: for a batch of exactly qt = 1, 2, 4 or 8 queries its tile rule (the largest
    // such width not above the batch, halved until the image fits) returns the width cluster_tile_width chose
    return plan_exact(nrows, ld, qt, 1);
}

hipError_t launch_assign_scan(const AssignArgs& a, const ExactPlan& p, hipStream_t s) {
    if (a.total <= 0) return hipSuccess;
    if (a.first < 0 || a.first >= a.m || a.first % p.qt != 0) return hipErrorInvalidValue;  // (tiles start at multiples of p.qt)
    AssignArgs t = a;  // the tile's place in the chain follows from its first centroid
    t.flags = (a.first == 0 ? kClusterFirst : 0u) | (a.first + p.qt >= a.m ? kClusterLast : 0u);
    return with_exact_tile(a.space, p.qt, [&](auto sp, auto qt, auto pw, auto nw) {
        constexpr auto kern = assign_scan_kernel<decltype(sp)::value, decltype(qt)::value, decltype(pw)::value, decltype(nw)::value>;
        const size_t lds = (size_t)p.qt * a.ld * sizeof(double);  // the query image alone (within kQueryImageMaxLds)
        if (hipError_t e = ensure_instance_lds<kern>(lds, kQueryImageMaxLds); e != hipSuccess) return e;
        kern<<<p.nblk, p.threads, lds, s>>>(t, p.nblk);
        return hipGetLastError();
    });
}

hipError_t launch_cluster_weights(const float* X, int32_t ld, int64_t total, double* w, hipStream_t s) {
    if (total <= 0) return hipSuccess;
    const int64_t panels = (total + kPanelRows - 1) / kPanelRows;
    cluster_weight_kernel<<<(unsigned)((panels + 3) / 4), 256, 0, s>>>(X, ld, total, w);
    return hipGetLastError();
}

hipError_t launch_cluster_list(const int32_t* assign, int64_t total, int32_t m, int32_t* hist, int64_t* counts, int64_t* base,
                               int32_t* members, unsigned long long* matched, hipStream_t s) {
    if (total <= 0 || m < 1 || m > kClusterMax) return hipErrorInvalidValue;
    const int64_t nblocks = cluster_list_blocks(total);
    cluster_hist_kernel<<<(unsigned)nblocks, kClusterListThreads, 0, s>>>(assign, total, m, hist, matched);
    cluster_offsets_kernel<<<1, kClusterMax, 0, s>>>(hist, nblocks, m, counts, base);
    cluster_fill_kernel<<<(unsigned)nblocks, kClusterListThreads, 0, s>>>(assign, total, m, hist, base, members);
    return hipGetLastError();
}

hipError_t launch_cluster_sums(const float* X, int32_t dim, int32_t ld, bool cosine, const ClusterSegment* segs, int32_t nsegs,
                               const int32_t* seg_first, const int32_t* members, const double* w, const double* best,
                               const int64_t* counts, int32_t m, bool means, double* partial, float* cent, double* cost,
                               hipStream_t s) {
    const int32_t nslices = (ld + 63) / 64, first_slice = means ? 0 : nslices;
    if (nsegs > 0) {
        const dim3 grid((unsigned)nsegs, (unsigned)(nslices + 1 - first_slice));
        if (cosine)
            cluster_sum_kernel<true><<<grid, 64, 0, s>>>(X, ld, segs, members, w, best, first_slice, nslices, partial);
        else
            cluster_sum_kernel<false><<<grid, 64, 0, s>>>(X, ld, segs, members, w, best, first_slice, nslices, partial);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    cluster_finish_kernel<<<m, 256, 0, s>>>(partial, seg_first, counts, dim, ld, means ? 0 : ld, cent, cost);
    return hipGetLastError();
}

hipError_t launch_cluster_write(const int32_t* assign, int64_t total, int64_t* column, hipStream_t s) {
    if (total <= 0) return hipSuccess;
    cluster_write_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(assign, total, column);
    return hipGetLastError();
}

}  // namespace mlvdb
