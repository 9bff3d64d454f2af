// Recommend / discover (include/mlvdb_examples.h): every row ranked against a bag of examples, each judged on its own.
//   examples_stage_kernel  one block per example: its stored row out of the panels (layout.h's addressing, as
//                          like_query_kernel reads it) or its uploaded raw vector -> one dense [examples, dim] batch, which
//                          launch_query_prep then treats as any queries.
//   examples_scan_kernel   exact_scan_kernel's shape, geometry and arithmetic -- plan_exact's tiles, gather_stage_queries,
//                          panel_walk; accumulate_rows / finish_distance give every d_j the scans' bits.  A block row works
//                          on ONE tile (ExamplesTile, cut on the host): up to QT examples of one query, a pair never split.
//                          panel_walk hands the sink the slots of a row back to back, so the reduction over the tile's
//                          examples runs in two registers (a, b) and a held POS distance, steered by the tile's role word
//                          (wave-uniform).  A bag of several tiles is walked by several launches: every tile but the first
//                          loads (a, b) of its (query, row) from the state workspace, every tile but the last stores it --
//                          one lane per row, 16 B, coalesced (24 B with tiles of one example, which carry a pair's POS
//                          distance too) -- and the last forms the key (tier, value), drops the query's
//                          own stored examples (their labels sit in LDS: at most 64 compares per row) and offers it to the
//                          wave's tiered list.  A bag of one tile touches no state.
//                          All four lanes 16 g + r of a row hold the same sums and run the same few fp64 operations per
//                          slot; lanes 0 .. 15 alone load, store and offer.  There is ONE list per tile where the exact
//                          scan keeps QT, so the admission test runs once per row, not once per (slot, row): the slots
//                          are already folded when it runs, which is all that sharing them over the four lanes could save.
//   examples_merge_kernel  one block per query: its last tile's per-block lists -> the answer.
// The folds are order-independent where the order is not fixed: a minimum does not depend on it (a distance is never -0.0:
// finish_distance returns a sum of squares or 1.0 - x), and CONTEXT's sum runs in pair order inside a tile and in tile order
// across launches, which one stream serialises.  Everything is fp64, one rounded operation per step (the library is built
// with -ffp-contract=off, restated below for this file).  No atomics, no scratch.
#include <algorithm>

#include "internal.h"
#include "panel_walk.h"
#include "wave_topk_tiered.h"

#pragma clang fp contract(off)

namespace mlvdb {

__global__ __launch_bounds__(256) void examples_stage_kernel(const float* __restrict__ X, const int32_t dim, const int32_t ld,
                                                             const int64_t* __restrict__ labels,
                                                             const int32_t* __restrict__ raw,
                                                             const float* __restrict__ vectors, float* __restrict__ out) {
    const int j = blockIdx.x;
    const int32_t rj = raw[j];
    if (rj >= 0) {  // (block-uniform)
        for (int c = threadIdx.x; c < dim; c += 256) out[(int64_t)j * dim + c] = vectors[(int64_t)rj * dim + c];
        return;
    }
    const float* row = X + layout_offset(labels[j], 0, ld);
    for (int c = threadIdx.x; c < dim; c += 256) out[(int64_t)j * dim + c] = row[(int64_t)(c >> 4) * kGroupFloats + (c & 15)];
}

hipError_t launch_examples_stage(const float* X, int32_t dim, int32_t ld, const int64_t* labels, const int32_t* raw,
                                 const float* vectors, int32_t n, float* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    examples_stage_kernel<<<n, 256, 0, s>>>(X, dim, ld, labels, raw, vectors, out);
    return hipGetLastError();
}

namespace {
// LDS: [the query tile | the block merge's lists][the query's exclusion labels]
__host__ __device__ constexpr size_t examples_base_bytes(int qt, int nw, int ld) {
    const size_t q_bytes = (size_t)qt * ld * sizeof(double);
    const size_t m_bytes = (size_t)nw * 64 * sizeof(TopEntry);
    return ((q_bytes > m_bytes ? q_bytes : m_bytes) + 15) / 16 * 16;
}
constexpr size_t examples_lds_bytes(int qt, int nw, int ld) { return examples_base_bytes(qt, nw, ld) + kExamplesMax * sizeof(int32_t); }
constexpr int kExamplesMaxLds = (int)examples_lds_bytes(1, 16, 8192);

// a minimum that keeps a NaN once it has met one: the result does not depend on the order
__device__ __forceinline__ double sticky_min(double m, double d) { return (d < m || d != d) && m == m ? d : m; }
}  // namespace

template <int SPACE, int QT, int PW, int NW>
__global__ __launch_bounds__(NW * 64) void examples_scan_kernel(const ExamplesArgs a, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]
    int32_t* excl = reinterpret_cast<int32_t*>(smem + examples_base_bytes(QT, NW, a.ld));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // The scalar registers are what this kernel runs out of (the role word and the flags steer scalar branches and have to
    // stay there), so whatever the walk needs per lane anyway is made per lane here, before it: the row's norm and state
    // through pointers that already carry the lane's row r, the block's partial list through one that carries the lane, and
    // cosine's 1 / |q| through the lanes' own copies.  Nothing of the 64-byte tile but two words outlives the staging.
    const ExamplesTile* const tp = a.tiles + blockIdx.y;  // (block-uniform)
    const int r = lane & 15;
    int qid[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) qid[t] = tp->ex[t];
    {
        const int n_stage = tp->n_excl, at = tp->excl_off;
        if ((int)threadIdx.x < n_stage) excl[threadIdx.x] = a.excl[at + threadIdx.x];
    }
    double qinv[QT];
    gather_stage_queries<QT, NW>(qs, a.Qpad, a.qaux, qid, a.ld, qinv);  // (ends with the barrier)
    if (SPACE == kSpaceCosine) {
#pragma unroll
        for (int t = 0; t < QT; ++t) qinv[t] = lane_read(qinv[t], lane);
    }

    const uint32_t flags = tp->flags, roles = tp->roles;
    const bool last = flags & kExLast;
    const int n_excl = last ? tp->n_excl : 0;
    const float* const rn_r = a.rn + r;
    ExamplesState* const state_r = a.state + (int64_t)(tp->state >= 0 ? tp->state : 0) * a.total + r;
    // a tile of one example (QT == 1: rows wider than 4096 columns) cannot keep a pair together: the held POS distance
    // travels beside the state
    double* const held_r = QT == 1 ? a.held + (int64_t)(tp->state >= 0 ? tp->state : 0) * a.total + r : nullptr;
    TopEntry* const out = a.partial + ((int64_t)tp->query * a.partial_stride + blockIdx.x) * a.k + lane;
    const int k = a.k;

    WaveTopKTiered top;
    top.init();
    double ra = 0.0, rb = 0.0, held = 0.0;
    // (no prefetch banks, unlike the exact scan's eight-query tile: their block counters and clamps are scalars, and with them
    // five instantiations spilled SGPRs; without them none does and three to four waves per SIMD hide the latency)
    panel_walk<SPACE, QT, PW, NW, 0, /*NT=*/true>(
        a.X, a.ld, a.total, nblk, qs, qinv,
        [&](int64_t row, bool in) {
            const bool live = panel_row_live(rn_r, row - r, in);
            // the state this tile starts from: the neutral element on a bag's first tile, what the tile before left otherwise
            ra = rb = (flags >> kExModeShift) & 3u ? 0.0 : __builtin_inf();  // (BEST is mode 0)
            if (!(flags & kExFirst) && live) {
                const ExamplesState st = state_r[row - r];
                ra = st.a;
                rb = st.b;
                if (QT == 1) held = held_r[row - r];
            }
            return live;
        },
        [&](int t, bool live, double dist, int32_t row) {
            switch ((roles >> (4 * t)) & 15u) {  // (wave-uniform; t is a constant once the walk is unrolled)
                case kExPosMin: ra = sticky_min(ra, dist); break;
                case kExNegMin: rb = sticky_min(rb, dist); break;
                case kExTarget: ra = dist; break;
                case kExPairPos: held = dist; break;
                case kExNegCount: rb = rb + (held < dist ? 0.0 : 1.0); break;
                case kExNegSum: ra = ra + (held > dist ? held - dist : 0.0); break;
                default: break;
            }
            if (t != QT - 1) return;
            if (!(flags & kExLast)) {  // (block-uniform)
                if (live) {
                    ExamplesState st;
                    st.a = ra;
                    st.b = rb;
                    state_r[row - r] = st;
                    if (QT == 1) held_r[row - r] = held;
                }
                return;
            }
            int32_t tier = 0;
            double value = ra;
            const uint32_t mode = (flags >> kExModeShift) & 3u;
            if (mode == MLVDB_EXAMPLES_BEST) {  // (block-uniform, like the tests of the flags below)
                bool liked = ra < rb;
                if (!(flags & kExHasNeg)) liked = true;
                if (!(flags & kExHasPos)) liked = false;
                tier = liked ? 0 : 1;
                value = liked ? ra : -rb;
            } else if (mode == MLVDB_EXAMPLES_DISCOVER) {
                tier = (int32_t)rb;
            }
            bool want = live && value == value;
            for (int e = 0; e < n_excl; ++e) want = want && excl[e] != row;
            top.offer(want, tier, value, row, k, lane);
        });
    if (!last) return;  // (block-uniform)

    // the waves' lists through LDS (aliasing the query tile, hence the barrier first) into the block's one
    __syncthreads();
    TopEntry* lists = reinterpret_cast<TopEntry*>(smem);  // [NW][64]
    lists[wave * 64 + lane] = top.entry();
    __syncthreads();
    if (wave != 0) return;
    WaveTopKTiered m;
    m.init();
    for (int w2 = 0; w2 < NW; ++w2) {
        const TopEntry e = lists[w2 * 64 + lane];
        m.offer(lane < k && e.l != kNoLabel, e, k, lane);
    }
    if (lane < k) *out = m.entry();
}

// One block (4 waves) per query: exact_merge_kernel's shape over the tiered entries.
__global__ __launch_bounds__(256) void examples_merge_kernel(const TopEntry* __restrict__ partial,
                                                             const int32_t* __restrict__ nblk_of, int32_t stride, int32_t k,
                                                             int64_t* out_labels, int32_t* out_tier, double* out_value,
                                                             int32_t* out_counts) {
    __shared__ TopEntry lists[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int q = blockIdx.x;
    const TopEntry* src = partial + (int64_t)q * stride * k;
    const int64_t n = (int64_t)nblk_of[q] * k;
    WaveTopKTiered m;
    m.init();
    for (int64_t i0 = (int64_t)wave * 64; i0 < n; i0 += 256) {
        const int64_t i = i0 + lane;
        TopEntry e;
        e.d = __builtin_inf();
        e.l = kNoLabel;
        e.pad = kNoTier;
        if (i < n) e = src[i];
        m.offer(e.l != kNoLabel, e, k, lane);
    }
    lists[wave][lane] = m.entry();
    __syncthreads();
    if (wave != 0) return;
    WaveTopKTiered f;
    f.init();
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
        const TopEntry e = lists[w2][lane];
        f.offer(lane < k && e.l != kNoLabel, e, k, lane);
    }
    const bool valid = lane < k && f.l != kNoLabel;
    if (lane < k) {
        out_labels[(int64_t)q * k + lane] = valid ? (int64_t)f.l : -1;
        out_tier[(int64_t)q * k + lane] = valid ? f.t : kNoTier;
        out_value[(int64_t)q * k + lane] = valid ? f.d : __builtin_inf();
    }
    const int cnt = __popcll(__ballot(valid));
    if (lane == 0) out_counts[q] = cnt;
}

// ------------------------------------------------------------------------------ host side
int32_t examples_tile_width(int32_t ld, int32_t most) {
    int32_t qt = most > 4 ? 8 : most > 2 ? 4 : most > 1 ? 2 : 1;
    while (qt > 1 && (size_t)qt * ld * sizeof(double) > 64 * 1024) qt >>= 1;
    return qt;
}

ExactPlan plan_examples(int64_t nrows, int32_t ld, int32_t qt, int32_t ntiles) {
    // plan_exact for ntiles tiles of qt queries each (its tile rule picks qt for a batch of exactly qt queries)
    ExactPlan p = plan_exact(nrows, ld, qt, 1);
    p.nqtiles = ntiles;
    const ExactTile tile = kExactTiles[exact_tile_index(p.qt)];
    const int64_t ntasks = ((nrows + 15) / 16 + tile.pw - 1) / tile.pw;
    int64_t nblk = (ntasks + tile.nw - 1) / tile.nw;
    const int64_t cap = std::max<int64_t>(8, std::min<int64_t>(256, 1024 / std::max(1, ntiles)));
    p.nblk = (int)std::max<int64_t>(1, std::min(nblk, cap));
    p.lds_bytes = examples_lds_bytes(p.qt, tile.nw, ld);
    return p;
}

hipError_t launch_examples_scan(const ExamplesArgs& a, const ExactPlan& p, hipStream_t s) {
    if (a.ntiles <= 0 || a.total <= 0) return hipSuccess;
    if (a.ntiles > 65535 || p.nblk > a.partial_stride) return hipErrorInvalidValue;
    return with_exact_tile(a.space, p.qt, [&](auto sp, auto qt, auto pw, auto nw) {
        constexpr auto kern = examples_scan_kernel<decltype(sp)::value, decltype(qt)::value, decltype(pw)::value, decltype(nw)::value>;
        // plan_examples: plan_exact's region (within kQueryImageMaxLds) and the exclusion labels
        if (hipError_t e = ensure_instance_lds<kern>(p.lds_bytes, kExamplesMaxLds); e != hipSuccess) return e;
        kern<<<dim3(p.nblk, a.ntiles), p.threads, p.lds_bytes, s>>>(a, p.nblk);
        return hipGetLastError();
    });
}

hipError_t launch_examples_merge(const TopEntry* partial, int32_t nq, const int32_t* nblk_of, int32_t stride, int32_t k,
                                 int64_t* out_labels, int32_t* out_tier, double* out_value, int32_t* out_counts, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    examples_merge_kernel<<<nq, 256, 0, s>>>(partial, nblk_of, stride, k, out_labels, out_tier, out_value, out_counts);
    return hipGetLastError();
}

}  // namespace mlvdb
