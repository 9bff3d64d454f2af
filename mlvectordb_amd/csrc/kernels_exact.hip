// Exact streaming scan: fp64 distances of every live row against a tile of QT queries, fused
// wave-level top-k, per-block partial lists, final merge.
//
// This is the universal exact path of the library: it serves small query batches at HBM
// speed (the fp64 arithmetic for <= 8 queries hides under the corpus stream), it seeds the
// thresholds of the bf16 filter path, and it is the fallback for any query the filter path
// gives up on.  It takes the place of hnswlib's knn_query as called from the reference
// (src/mlvectordb/implementations/index.py:111), computed exhaustively.
#include <algorithm>
#include <cstdlib>

#include "internal.h"
#include "panel_walk.h"

namespace mlvdb {

template <int SPACE, int QT, int PW, int NW>
__global__ __launch_bounds__(NW * 64) void exact_scan_kernel(const ExactArgs a, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    const int lane = threadIdx.x & 63;
    const int nq_sel = a.nq_sel_dev ? min(*a.nq_sel_dev, a.nq_sel) : a.nq_sel;
    if ((int)blockIdx.y * QT >= nq_sel) return;  // block-uniform: nothing selected for this query tile

    int qid[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int sel = blockIdx.y * QT + t;
        qid[t] = sel < nq_sel ? (a.qsel ? a.qsel[sel] : sel) : -1;
    }
    double qinv[QT];
    gather_stage_queries<QT, NW>(qs, a.Qpad, a.qaux, qid, a.ld, qinv);

    double cur_d[QT];
    int32_t cur_l[QT];
    WaveTopK top[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const bool has_cur = a.cursor_d != nullptr && qid[t] >= 0;
        cur_d[t] = has_cur ? a.cursor_d[qid[t]] : -__builtin_inf();
        cur_l[t] = has_cur ? a.cursor_l[qid[t]] : -1;
        top[t].init();
    }
    // every row is read once per launch, hence the non-temporal loads
    panel_walk<SPACE, QT, PW, NW, (QT == 8 ? 4 : 0), /*NT=*/true>(
        a.X, a.ld, a.row_end, nblk, qs, qinv, [&](int64_t row, bool in) { return panel_row_live(a.rn, row, in); },
        [&](int t, bool live, double dist, int32_t row) {
            const bool want = live && qid[t] >= 0 && entry_less(cur_d[t], cur_l[t], dist, row);
            top[t].offer(want, dist, row, a.k, lane);
        });
    gather_block_merge<QT, NW>(smem, top, qid, a.k, [&](int t) {
        return a.partial + ((int64_t)(blockIdx.y * QT + t) * nblk + blockIdx.x) * a.k;
    });
}

// Range-query candidate generator: same scan, but every live row with dist <= radius is
// appended to its query's candidate list (rescored and sorted by launch_range_rescore's kernels).  QT queries per block, their fp64
// image [QT][ld] in LDS: launch_exact_range_scan picks 4 / 2 / 1 by the row width.
template <int SPACE, int QT>
__global__ __launch_bounds__(512) void exact_range_kernel(const FilterArgs a, const double radius, const int nblk,
                                                          const int32_t* qsel, const int32_t nsel) {
    constexpr int PW = 2, NW = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    int qid[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int sel = blockIdx.y * QT + t;
        qid[t] = sel < nsel ? (qsel ? qsel[sel] : sel) : -1;
    }
    double qinv[QT];
    gather_stage_queries<QT, NW>(qs, a.Qpad, a.qaux, qid, a.ld, qinv);
    panel_walk<SPACE, QT, PW, NW, 0, /*NT=*/false>(
        a.X, a.ld, a.total, nblk, qs, qinv, [&](int64_t row, bool in) { return panel_row_live(a.rn, row, in); },
        [&](int t, bool live, double dist, int32_t row) {
            if (live && qid[t] >= 0 && dist <= radius) {
                const uint32_t slot = atomicAdd(&a.cnt[qid[t]], 1u);
                if (slot < (uint32_t)a.cand_cap) {
                    CandEntry e;
                    e.u = 0.f;
                    e.row = row;
                    a.cand[(int64_t)qid[t] * a.cand_cap + slot] = e;
                } else {
                    a.overflow[qid[t]] = 1u;
                }
            }
        });
}

hipError_t launch_exact_range_scan(const FilterArgs& a, float radius, const int32_t* qsel, int32_t nsel, hipStream_t s) {
    if (!qsel) nsel = a.nq;
    if (nsel <= 0) return hipSuccess;
    // the query tile halves until its fp64 image fits 64 KiB of LDS, as plan_exact's does: 4 queries up to ld = 2048, 2 up to
    // 4096, 1 beyond (ld <= 8192).  Four queries of an ld > 5120 would ask for more LDS than a CU has (160 KiB).
    int qt = 4;
    while (qt > 1 && (size_t)qt * a.ld * sizeof(double) > 64 * 1024) qt >>= 1;
    const int nqtiles = (nsel + qt - 1) / qt;
    const int64_t ntasks = ((a.total + 15) / 16 + 1) / 2;
    int64_t nblk = (ntasks + 7) / 8;
    const int64_t cap = std::max<int64_t>(8, 1024 / nqtiles);
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    const size_t lds = (size_t)qt * a.ld * sizeof(double);
    return with_space_qt(a.space, qt, [&](auto sp, auto qtc) {
        constexpr auto kern = exact_range_kernel<decltype(sp)::value, decltype(qtc)::value>;
        // the halving above keeps the image within kQueryImageMaxLds
        if (hipError_t e = ensure_instance_lds<kern>(lds, kQueryImageMaxLds); e != hipSuccess) return e;
        kern<<<dim3((unsigned)nblk, nqtiles), 512, lds, s>>>(a, (double)radius, (int)nblk, qsel, nsel);
        return hipGetLastError();
    });
}

// ------------------------------------------------------------------------------ host side
// ------------------------------------------------------------------ exact distances of given (query, label) pairs
// The vector-level face of the same arithmetic (reference README.md:30-41,178-181: SimpleVector.distance / similarity):
// out[q][j] = distance of query q to row labels[q][j] in the index's space, fp64, by the very accumulate_rows the exact
// scan and the rescoring use -- so a pair scored here is bit-identical to the score a search returns for it.
// Block (q, chunk): 4 waves, each scores 16 pairs per step.  label < 0: +inf (search padding passes through).
template <int SPACE>
__global__ __launch_bounds__(256) void pair_distance_kernel(const float* __restrict__ X, const float* __restrict__ Qpad,
                                                            const double* __restrict__ qaux, const int64_t* __restrict__ labels,
                                                            int32_t m, int32_t ld, double* __restrict__ out64,
                                                            float* __restrict__ out32) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [ld]
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, r = lane & 15;
    for (int c = threadIdx.x; c < ld; c += 256) qs[c] = (double)Qpad[(int64_t)q * ld + c];
    __syncthreads();
    const double qinv = qaux[q];
    const int64_t* lab = labels + (int64_t)q * m;
    for (int j0 = (blockIdx.y * 4 + wave) * 16; j0 < m; j0 += gridDim.y * 64) {
        const int j = j0 + r;
        const bool have = j < m;
        const int64_t row = have ? lab[j] : -1;
        const int64_t rr = row >= 0 ? row : 0;
        const float* base[1] = {X + (rr >> 4) * (int64_t)(kPanelRows * ld) + (rr & 15) * 16 + g * 4};
        double acc[1][1], nx[1];
        accumulate_rows<SPACE, 1, 1, 8>(base, qs, ld, g, acc, nx);
        const double d = row >= 0 ? finish_distance<SPACE>(acc[0][0], nx[0], qinv) : __builtin_inf();
        if (have && lane < 16) {
            out64[(int64_t)q * m + j] = d;
            if (out32) out32[(int64_t)q * m + j] = (float)d;
        }
    }
}

// ------------------------------------------------------------------ exact k-th best of a PREFIX of the rows (small batches)
// The seed of a filter pass of <= 8 queries: exact fp64 distances of rows 0..m-1 (accumulate_rows: the scores every other
// exact path gives them), tombstoned rows +inf, one 16-row group per wave so the few thousand rows spread over the chip as
// m/64 blocks per query; filter_prefix_thr_kernel (kernels_filter.hip) then takes the k-th best per query by a radix select
// on order keys (per-wave sorted top-k lists with fp64 lane shuffles took 34 us for 3840 rows: profiles/r03).
// Replaces the dense int8 seeding pass + exact-threshold refine (two latency chains, 23 us at batch 1) where the fp64
// arithmetic of m x nq rows costs nothing.
template <int SPACE, int PF>
__global__ __launch_bounds__(256) void prefix_exact_kernel(const float* __restrict__ X, const float* __restrict__ rn,
                                                           const float* __restrict__ Qpad, const double* __restrict__ qaux,
                                                           int32_t m, int32_t ld, double* __restrict__ out64) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [ld]
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, r = lane & 15;
    const int nw = blockDim.x >> 6;
    for (int c = threadIdx.x; c < ld; c += blockDim.x) qs[c] = (double)Qpad[(int64_t)q * ld + c];
    __syncthreads();
    const double qinv = qaux[q];
    for (int j0 = (blockIdx.y * nw + wave) * 16; j0 < m; j0 += gridDim.y * nw * 16) {
        const int j = j0 + r;
        const bool have = j < m;
        const int64_t rr = have ? j : 0;
        const float* base[1] = {X + (rr >> 4) * (int64_t)(kPanelRows * ld) + (rr & 15) * 16 + g * 4};
        double acc[1][1], nx[1];
        accumulate_rows<SPACE, 1, 1, PF>(base, qs, ld, g, acc, nx);
        if (have && lane < 16) {
            const float nrm = rn[rr];
            const double d = finish_distance<SPACE>(acc[0][0], nx[0], qinv);
            out64[(int64_t)q * m + j] = nrm == nrm && d == d ? d : __builtin_inf();
        }
    }
}

hipError_t launch_prefix_exact(const float* X, const float* rn, const float* Qpad, const double* qaux, int32_t nq, int32_t m,
                               int32_t ld, int32_t space, double* d64, hipStream_t s) {
    if (nq <= 0 || m <= 0) return hipErrorInvalidValue;
    const size_t lds = (size_t)ld * sizeof(double);
    // a whole 768-column row in flight per lane (24 groups x two banks) when the row is a whole number of such halves:
    // one round trip per row instead of three (the kernel is one latency chain per wave)
    const bool pf24 = (ld / 16) % 24 == 0;
    const int nw = 4;  // waves per block, 16 rows each
    const dim3 grid((unsigned)nq, (unsigned)(((int64_t)m + 16 * nw - 1) / (16 * nw)));
    return with_space(space, [&](auto sp) {
        auto launch = [&](auto pf) {
            constexpr auto kern = prefix_exact_kernel<decltype(sp)::value, decltype(pf)::value>;
            // one query's image: within kQueryImageMaxLds
            if (hipError_t e = ensure_instance_lds<kern>(lds, kQueryImageMaxLds); e != hipSuccess) return e;
            kern<<<grid, nw * 64, lds, s>>>(X, rn, Qpad, qaux, m, ld, d64);
            return hipGetLastError();
        };
        return pf24 ? launch(std::integral_constant<int, 24>{}) : launch(std::integral_constant<int, 8>{});
    });
}

hipError_t launch_pair_distances(const float* X, const float* Qpad, const double* qaux, const int64_t* labels, int32_t nq,
                                 int32_t m, int32_t ld, int32_t space, double* out64, float* out32, hipStream_t s) {
    if (nq <= 0 || m <= 0) return hipSuccess;
    const size_t lds = (size_t)ld * sizeof(double);
    const dim3 grid((unsigned)nq, (unsigned)std::min<int64_t>(64, ((int64_t)m + 63) / 64));
    return with_space(space, [&](auto sp) {
        constexpr auto kern = pair_distance_kernel<decltype(sp)::value>;
        // one query's image: within kQueryImageMaxLds
        if (hipError_t e = ensure_instance_lds<kern>(lds, kQueryImageMaxLds); e != hipSuccess) return e;
        kern<<<grid, 256, lds, s>>>(X, Qpad, qaux, labels, m, ld, out64, out32);
        return hipGetLastError();
    });
}

ExactPlan plan_exact(int64_t nrows, int32_t ld, int32_t nq_sel, int32_t k) {
    ExactPlan p;
    int qt = nq_sel >= 8 ? 8 : nq_sel >= 4 ? 4 : nq_sel >= 2 ? 2 : 1;
    while (qt > 1 && (size_t)qt * ld * sizeof(double) > 64 * 1024) qt >>= 1;
    p.qt = qt;
    const int nw = kExactTiles[exact_tile_index(qt)].nw, pw = kExactTiles[exact_tile_index(qt)].pw;
    p.threads = nw * 64;
    p.nqtiles = (nq_sel + qt - 1) / qt;
    const int64_t npanels = (nrows + 15) / 16;
    const int64_t ntasks = (npanels + pw - 1) / pw;
    int64_t nblk = (ntasks + nw - 1) / nw;
    // one block per CU is the sweet spot for the streaming scan (profiles/r01/exact_ab_nt_1m.txt); with several query
    // tiles the corpus is split over fewer blocks each
    int64_t cap = std::min<int64_t>(256, 1024 / p.nqtiles);
    if (cap < 8) cap = 8;
    if (nblk > cap) nblk = cap;
    if (nblk < 1) nblk = 1;
    p.nblk = (int)nblk;
    const size_t q_bytes = (size_t)qt * ld * sizeof(double);
    const size_t m_bytes = (size_t)nw * qt * 64 * (sizeof(double) + sizeof(int32_t));
    p.lds_bytes = q_bytes > m_bytes ? q_bytes : m_bytes;
    (void)k;
    return p;
}

hipError_t launch_exact_scan(const ExactArgs& a, const ExactPlan& p, hipStream_t s) {
    if (a.nq_sel <= 0) return hipSuccess;
    return with_exact_tile(a.space, p.qt, [&](auto sp, auto qt, auto pw, auto nw) {
        constexpr auto kern = exact_scan_kernel<decltype(sp)::value, decltype(qt)::value, decltype(pw)::value, decltype(nw)::value>;
        // plan_exact: the query image or the merge lists, neither above kQueryImageMaxLds
        if (hipError_t e = ensure_instance_lds<kern>(p.lds_bytes, kQueryImageMaxLds); e != hipSuccess) return e;
        kern<<<dim3(p.nblk, p.nqtiles), p.threads, p.lds_bytes, s>>>(a, p.nblk);
        return hipGetLastError();
    });
}

hipError_t launch_exact_merge(const TopEntry* partial, int32_t nq_sel, const int32_t* nq_sel_dev, const int32_t* qsel,
                              int32_t nblk, int32_t k, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                              double* out_d64, hipStream_t s) {
    if (nq_sel <= 0) return hipSuccess;
    exact_merge_kernel<false><<<nq_sel, 256, 0, s>>>(partial, nq_sel_dev, qsel, nblk, k, out_labels, out_dist, out_counts,
                                                     out_d64);
    return hipGetLastError();
}

}  // namespace mlvdb
