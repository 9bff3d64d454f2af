// Distinct-by-attribute kNN (include/mlvdb_distinct.h): the nearest row of each of the k nearest groups, a group being one
// present value of an int64 attribute column.
//   distinct_pick_kernel   one wave per query over its ranked list from the plain search: the first entry of each group,
//                          until k groups are kept; queries whose list ends first are flagged for the grouped scan
//   distinct_scan_kernel   exact_scan_kernel with WaveTopKDistinct: the same accumulate_rows / finish_distance (a row's
//                          distance keeps the exact scan's bits), per-block partial lists that carry the group code
//   distinct_merge_kernel  the partial lists of a query folded by the same group-aware offer
// The merge is exact: a group among the k nearest has its best row in some block; fewer than k groups beat that row in
// the whole corpus, so fewer than k do in the block, and the block's list holds it.
#include <algorithm>

#include "internal.h"
#include "panel_walk.h"
#include "wave_topk_distinct.h"

namespace mlvdb {

__global__ __launch_bounds__(64) void distinct_pick_kernel(const int64_t* __restrict__ lab, const double* __restrict__ d64,
                                                           const int32_t* __restrict__ cnt, const int32_t L,
                                                           const int64_t* __restrict__ group, const int32_t k,
                                                           const int32_t k_eff, int32_t* __restrict__ qsel,
                                                           int32_t* __restrict__ nflag, int64_t* __restrict__ out_labels,
                                                           float* __restrict__ out_dist, int32_t* __restrict__ out_counts,
                                                           double* __restrict__ out_d64, int64_t* __restrict__ out_groups) {
    const int q = blockIdx.x;
    const int lane = threadIdx.x;
    const int n = min(cnt[q], L);  // valid entries of the list, ranked by (distance, label)
    const int64_t* ql = lab + (int64_t)q * L;
    const double* qd = d64 + (int64_t)q * L;
    int64_t kg = kNoGroup, kl = -1;  // lane i: the i-th kept entry
    double kd = __builtin_inf();
    int kept = 0;
    for (int base = 0; base < n && kept < k_eff; base += kWave) {
        const int i = base + lane;
        const int64_t label = i < n ? ql[i] : -1;
        const bool have = label >= 0;
        const int64_t cg = have ? group[label] : kNoGroup;
        const double cd = have ? qd[i] : __builtin_inf();
        unsigned long long m = __ballot(cg != kNoGroup);
        while (m && kept < k_eff) {
            const int src = __builtin_ctzll(m);
            const int64_t vg = lane_read(cg, src);
            m &= ~__ballot(cg == vg);  // the group's later entries of this chunk rank behind this one
            if (__ballot(lane < kept && kg == vg)) continue;
            const int64_t vl = lane_read(label, src);
            const double vd = lane_read(cd, src);
            if (lane == kept) {
                kg = vg;
                kl = vl;
                kd = vd;
            }
            ++kept;
        }
    }
    // fewer than L valid entries: the list holds every live allowed row, so what was kept is all there is
    const bool complete = kept == k_eff || n < L;
    if (!complete) {
        if (lane == 0) qsel[atomicAdd(nflag, 1)] = q;
        return;
    }
    if (lane < k) {
        const bool valid = lane < kept;
        const int64_t o = (int64_t)q * k + lane;
        out_labels[o] = valid ? kl : -1;
        out_dist[o] = valid ? (float)kd : __builtin_inff();
        out_d64[o] = valid ? kd : __builtin_inf();
        out_groups[o] = valid ? kg : kNoGroup;
    }
    if (lane == 0) out_counts[q] = kept;
}

template <int SPACE, int QT, int PW, int NW>
__global__ __launch_bounds__(NW * 64) void distinct_scan_kernel(const DistinctArgs a, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
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

    WaveTopKDistinct top[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) top[t].init();

    // panel_walk's loop, written out: through the shared function the eight-query l2 and ip instances come out at 224 and
    // 221 VGPRs instead of 166 and lose their third wave per SIMD (profiles/r16), whatever shape the sink is given.
    const int ld = a.ld, g = lane >> 4, r = lane & 15;
    const int64_t panel_end = (a.total + 15) >> 4;
    const int64_t ntasks = (panel_end + PW - 1) / PW;
    for (int64_t task = (int64_t)blockIdx.x * NW + wave; task < ntasks; task += (int64_t)nblk * NW) {
        const float* base[PW];
        int64_t panel[PW];
#pragma unroll
        for (int p = 0; p < PW; ++p) {
            panel[p] = task * PW + p;
            const int64_t pp = panel[p] < panel_end ? panel[p] : 0;  // keep the address valid
            base[p] = a.X + pp * (int64_t)(kPanelRows * ld) + lane_group_offset(lane);
        }
        double acc[PW][QT];
        double nx[PW];
        accumulate_rows<SPACE, QT, PW, (QT == 8 ? 1 : 0), /*NT=*/true>(base, qs, ld, g, acc, nx);  // (the exact scan's PF = 4 spills here: 8 lists carry 16 more VGPRs)
#pragma unroll
        for (int p = 0; p < PW; ++p) {
            const int64_t row = panel[p] * kPanelRows + r;
            bool live = panel_row_live(a.rn, row, lane < 16 && panel[p] < panel_end && row < a.total);
            int64_t grp = kNoGroup;
            if (live) {
                grp = a.group[row];
                live = grp != kNoGroup;  // an absent value belongs to no group
            }
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const double dist = finish_distance<SPACE>(acc[p][t], nx[p], qinv[t]);
                top[t].offer(live && qid[t] >= 0, dist, (int32_t)row, grp, a.k, lane);
            }
        }
    }

    // ---- block merge: the lists of all waves through LDS (aliases the query tile), GT queries at a time
    constexpr int GT = QT < 4 ? QT : 4;
    static_assert(GT <= NW, "one merging wave per query of a group");
    double* ld_d = reinterpret_cast<double*>(smem);                                                   // [NW][GT][64]
    int64_t* ld_g = reinterpret_cast<int64_t*>(smem + (size_t)NW * GT * 64 * sizeof(double));         // [NW][GT][64]
    int32_t* ld_l = reinterpret_cast<int32_t*>(smem + (size_t)NW * GT * 64 * 2 * sizeof(double));     // [NW][GT][64]
#pragma unroll
    for (int t0 = 0; t0 < QT; t0 += GT) {
        __syncthreads();  // the query tile / the previous group's lists are consumed
#pragma unroll
        for (int tt = 0; tt < GT; ++tt) {
            ld_d[(wave * GT + tt) * 64 + lane] = top[t0 + tt].d;
            ld_g[(wave * GT + tt) * 64 + lane] = top[t0 + tt].g;
            ld_l[(wave * GT + tt) * 64 + lane] = top[t0 + tt].l;
        }
        __syncthreads();
        if (wave < GT) {
            WaveTopKDistinct m;
            m.init();
            for (int w2 = 0; w2 < NW; ++w2) {
                const double cd = ld_d[(w2 * GT + wave) * 64 + lane];
                const int64_t cg = ld_g[(w2 * GT + wave) * 64 + lane];
                const int32_t cl = ld_l[(w2 * GT + wave) * 64 + lane];
                m.offer(lane < a.k && cl != kNoLabel, cd, cl, cg, a.k, lane);
            }
            const int sel = blockIdx.y * QT + t0 + wave;
            if (sel < nq_sel && lane < a.k) {
                DistinctEntry e;
                e.d = m.d;
                e.g = m.g;
                e.l = m.l;
                e.pad = 0;
                a.partial[((int64_t)sel * nblk + blockIdx.x) * a.k + lane] = e;
            }
        }
    }
}

// One block (4 waves) per selected query: each wave folds a quarter of the partial entries, wave 0 folds the four lists
// and writes the final answer.
__global__ __launch_bounds__(256) void distinct_merge_kernel(const DistinctEntry* __restrict__ partial,
                                                             const int32_t* nq_sel_dev, const int32_t* qsel, int32_t nblk,
                                                             int32_t k, int32_t k_eff, int64_t* out_labels, float* out_dist,
                                                             int32_t* out_counts, double* out_d64, int64_t* out_groups) {
    __shared__ double sd[4][64];
    __shared__ int64_t sg[4][64];
    __shared__ int32_t sl[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int sel = blockIdx.x;
    if (nq_sel_dev && sel >= *nq_sel_dev) return;
    const int q = qsel ? qsel[sel] : sel;
    const DistinctEntry* src = partial + (int64_t)sel * nblk * k;
    const int64_t n = (int64_t)nblk * k;
    WaveTopKDistinct m;
    m.init();
    for (int64_t i0 = (int64_t)wave * 64; i0 < n; i0 += 256) {
        const int64_t i = i0 + lane;
        DistinctEntry e;
        e.d = __builtin_inf();
        e.g = kNoGroup;
        e.l = kNoLabel;
        if (i < n) e = src[i];
        m.offer(e.l != kNoLabel, e.d, e.l, e.g, k, lane);
    }
    sd[wave][lane] = m.d;
    sg[wave][lane] = m.g;
    sl[wave][lane] = m.l;
    __syncthreads();
    if (wave != 0) return;
    WaveTopKDistinct f;
    f.init();
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
        const double cd = sd[w2][lane];
        const int64_t cg = sg[w2][lane];
        const int32_t cl = sl[w2][lane];
        f.offer(lane < k && cl != kNoLabel, cd, cl, cg, k, lane);
    }
    const bool valid = lane < k_eff && f.l != kNoLabel;  // k_eff < k: the caller's bound on the number of groups
    if (lane < k) {
        const int64_t o = (int64_t)q * k + lane;
        out_labels[o] = valid ? (int64_t)f.l : -1;
        out_dist[o] = valid ? (float)f.d : __builtin_inff();
        out_d64[o] = valid ? f.d : __builtin_inf();
        out_groups[o] = valid ? f.g : kNoGroup;
    }
    const int cnt = __popcll(__ballot(valid));
    if (lane == 0) out_counts[q] = cnt;
}

// ------------------------------------------------------------------------------ host side
hipError_t launch_distinct_pick(const int64_t* lab, const double* d64, const int32_t* cnt, int32_t nq, int32_t L,
                                const int64_t* group, int32_t k, int32_t k_eff, int32_t* qsel, int32_t* nflag,
                                int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_d64, int64_t* out_groups,
                                hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    distinct_pick_kernel<<<nq, 64, 0, s>>>(lab, d64, cnt, L, group, k, k_eff, qsel, nflag, out_labels, out_dist, out_counts,
                                           out_d64, out_groups);
    return hipGetLastError();
}

ExactPlan plan_distinct(int64_t nrows, int32_t ld, int32_t nq_sel, int32_t k) {
    ExactPlan p = plan_exact(nrows, ld, nq_sel, k);  // the exact scan's geometry; the merge lists carry 8 more bytes
    const int nw = p.threads / 64, gt = std::min(p.qt, 4);
    const size_t q_bytes = (size_t)p.qt * ld * sizeof(double);
    const size_t m_bytes = (size_t)nw * gt * 64 * (2 * sizeof(double) + sizeof(int32_t));
    p.lds_bytes = std::max(q_bytes, m_bytes);
    return p;
}

hipError_t launch_distinct_scan(const DistinctArgs& a, const ExactPlan& p, hipStream_t s) {
    if (a.nq_sel <= 0) return hipSuccess;
    return with_exact_tile(a.space, p.qt, [&](auto sp, auto qt, auto pw, auto nw) {
        constexpr auto kern = distinct_scan_kernel<decltype(sp)::value, decltype(qt)::value, decltype(pw)::value, decltype(nw)::value>;
        // plan_distinct: the query image or the merge lists, neither above kQueryImageMaxLds
        if (hipError_t e = ensure_instance_lds<kern>(p.lds_bytes, kQueryImageMaxLds); e != hipSuccess) return e;
        kern<<<dim3(p.nblk, p.nqtiles), p.threads, p.lds_bytes, s>>>(a, p.nblk);
        return hipGetLastError();
    });
}

hipError_t launch_distinct_merge(const DistinctEntry* partial, int32_t nq_sel, const int32_t* nq_sel_dev, const int32_t* qsel,
                                 int32_t nblk, int32_t k, int32_t k_eff, int64_t* out_labels, float* out_dist,
                                 int32_t* out_counts, double* out_d64, int64_t* out_groups, hipStream_t s) {
    if (nq_sel <= 0) return hipSuccess;
    distinct_merge_kernel<<<nq_sel, 256, 0, s>>>(partial, nq_sel_dev, qsel, nblk, k, k_eff, out_labels, out_dist, out_counts,
                                                 out_d64, out_groups);
    return hipGetLastError();
}

}  // namespace mlvdb
