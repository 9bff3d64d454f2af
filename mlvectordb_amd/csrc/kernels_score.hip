// Scored kNN (include/mlvdb_score.h): the exact top k of every query by a formula of the row's distance and its attributes.
//   scored_scan_kernel   exact_scan_kernel's shape, geometry and arithmetic -- plan_exact's tiles, gather_stage_queries,
//                        panel_walk, gather_block_merge; accumulate_rows / finish_distance give DIST the scans' bits -- with
//                        the score program between the distance and the selection lists.  Per row, once: its liveness, one
//                        bit per cond program (where_eval_with) and the value of every ATTR operand (8 coalesced bytes per
//                        row and operand, parked in the wave's own LDS slots).  Per (slot, row): score_eval, and the offer
//                        of (score, row) to the slot's WaveTopK unless the score is NaN -- the four lanes that hold a
//                        row's sums take a slot each, so the program runs once per four slots.
// Its partial lists hold (score, row) and go through launch_exact_merge like the exact scan's.
// LDS: [the query tile | the block merge's lists, as plan_exact sizes them][ScoreProgram][NW x kScoreMaxOperands x 16 values].
// Everything is fp64, one rounded operation per op (the library is built with -ffp-contract=off, restated below for this
// file).  No atomics, no scratch.
#include <algorithm>

#include "internal.h"
#include "panel_walk.h"
#include "where_common.h"

#pragma clang fp contract(off)

#include "score_common.h"

namespace mlvdb {

namespace {
// bytes of the region the query tile and the block merge's lists share (plan_exact's lds_bytes), rounded to the alignment
// of what follows it
__host__ __device__ constexpr size_t scored_base_bytes(int qt, int nw, int ld) {
    const size_t q_bytes = (size_t)qt * ld * sizeof(double);
    const size_t m_bytes = (size_t)nw * qt * 64 * (sizeof(double) + sizeof(int32_t));
    return ((q_bytes > m_bytes ? q_bytes : m_bytes) + 15) / 16 * 16;
}
constexpr size_t scored_lds_bytes(int qt, int nw, int ld) {
    return scored_base_bytes(qt, nw, ld) + sizeof(ScoreProgram) + (size_t)nw * kScoreMaxOperands * kPanelRows * sizeof(double);
}
// the most any launch asks for: a 64 KiB query image and 16 waves
constexpr int kScoredMaxLds = (int)scored_lds_bytes(1, 16, 8192);

// What the walk computes once per panel row
struct ScoredRow {
    bool live;      // a live row of the range (tombstones and the call's `where` mask both read as NaN norms)
    bool any_live;  // ... in some lane of the wave (uniform)
    uint32_t cond;  // bit c: the row matches cond c
};
}  // namespace

template <int SPACE, int QT, int PW, int NW>
__global__ __launch_bounds__(NW * 64) void scored_scan_kernel(const ScoredArgs a, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    const ScoreProgram* sp = reinterpret_cast<const ScoreProgram*>(smem + scored_base_bytes(QT, NW, a.ld));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // this lane's row of the wave's operand values: vals[slot * 16] (lanes 16 g + r share row r's slots)
    double* vals = reinterpret_cast<double*>(smem + scored_base_bytes(QT, NW, a.ld) + sizeof(ScoreProgram)) +
                   wave * (kScoreMaxOperands * kPanelRows) + (lane & 15);

    int qid[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int q = blockIdx.y * QT + t;
        qid[t] = q < a.nq ? q : -1;
    }
    {  // the programs, once per block (gather_stage_queries ends with the barrier)
        const int4* src = reinterpret_cast<const int4*>(a.prog);
        int4* dst = reinterpret_cast<int4*>(smem + scored_base_bytes(QT, NW, a.ld));
        for (int i = threadIdx.x; i < (int)(sizeof(ScoreProgram) / sizeof(int4)); i += NW * 64) dst[i] = src[i];
    }
    double qinv[QT];
    gather_stage_queries<QT, NW>(qs, a.Qpad, a.qaux, qid, a.ld, qinv);
    const int n_ops = sp->n_ops, n_operands = sp->n_operands, n_conds = sp->n_conds;

    WaveTopK top[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) top[t].init();

    // The four lanes 16 g + r of a row hold the same distances (accumulate_rows ends with the sums in all four), so they
    // share the row's slots: lane group g evaluates slots g, g + 4, ... and offers for them alone -- one pass of the
    // program per four slots instead of one per slot.  Which lane evaluates a pair changes no bit of its score.
    const int g = lane >> 4;
    double mine = 0.0;  // the distance of this lane group's slot among the current four
    panel_walk<SPACE, QT, PW, NW, (QT == 8 ? 4 : 0), /*NT=*/true>(
        a.X, a.ld, a.total, nblk, qs, qinv,
        [&](int64_t row, bool in) {
            ScoredRow st;
            // (the walk's `in` names one lane of the four; here all four report the row, each for its own slots: a row
            // of a panel past the end lies past the range too)
            st.live = panel_row_live(a.rn, row, row < a.total);
            st.any_live = __ballot(st.live) != 0;
            st.cond = 0;
            if (!st.any_live) return st;  // (wave-uniform)
            for (int c = 0; c < n_conds; ++c) {
                const bool m = where_eval_with(sp->cond_ops + sp->cond_off[c], sp->cond_off[c + 1] - sp->cond_off[c], a.set,
                                               [&](const WhereOp& o) {
                                                   return st.live ? static_cast<const int64_t*>(o.col)[row] : INT64_MIN;
                                               });
                st.cond |= m ? 1u << c : 0u;
            }
            for (int j = 0; j < n_operands; ++j) {
                const ScoreOperand od = sp->operands[j];
                if (in && st.live) vals[j * kPanelRows] = score_operand_value(od, od.col[row]);
            }
            return st;
        },
        [&](int t, const ScoredRow& st, double dist, int32_t row) {
            if ((t & 3) == g) mine = dist;
            if ((t & 3) != 3 && t != QT - 1) return;  // the last slot of a four, or of the tile: evaluate and offer
            if (qid[t & ~3] < 0 || !st.any_live) return;  // (wave-uniform: nothing to offer; the slots of a tile fill in order)
            const double sc = score_eval(sp->ops, n_ops, mine, st.cond, [&](int slot) { return vals[slot * kPanelRows]; });
            const bool ok = st.live && sc == sc;
            top[t].offer(ok && (t & 3) == g && qid[t] >= 0, sc, row, a.k, lane);
            if ((t & 3) >= 1) top[t - 1].offer(ok && ((t - 1) & 3) == g && qid[t - 1] >= 0, sc, row, a.k, lane);
            if ((t & 3) >= 2) top[t - 2].offer(ok && ((t - 2) & 3) == g && qid[t - 2] >= 0, sc, row, a.k, lane);
            if ((t & 3) >= 3) top[t - 3].offer(ok && ((t - 3) & 3) == g && qid[t - 3] >= 0, sc, row, a.k, lane);
        });
    gather_block_merge<QT, NW>(smem, top, qid, a.k, [&](int t) {
        return a.partial + ((int64_t)(blockIdx.y * QT + t) * nblk + blockIdx.x) * a.k;
    });
}

// ------------------------------------------------------------------------------ host side
ExactPlan plan_scored(int64_t nrows, int32_t ld, int32_t nq, int32_t k) {
    ExactPlan p = plan_exact(nrows, ld, nq, k);
    p.lds_bytes = scored_lds_bytes(p.qt, p.threads / 64, ld);
    return p;
}

hipError_t launch_scored_scan(const ScoredArgs& a, const ExactPlan& p, hipStream_t s) {
    if (a.nq <= 0) return hipSuccess;
    return with_exact_tile(a.space, p.qt, [&](auto sp, auto qt, auto pw, auto nw) {
        constexpr auto kern = scored_scan_kernel<decltype(sp)::value, decltype(qt)::value, decltype(pw)::value, decltype(nw)::value>;
        // plan_scored: plan_exact's region (within kQueryImageMaxLds), the programs and the operand values
        if (hipError_t e = ensure_instance_lds<kern>(p.lds_bytes, kScoredMaxLds); e != hipSuccess) return e;
        kern<<<dim3(p.nblk, p.nqtiles), p.threads, p.lds_bytes, s>>>(a, p.nblk);
        return hipGetLastError();
    });
}

}  // namespace mlvdb
