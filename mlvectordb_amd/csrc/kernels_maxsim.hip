// Late-interaction search (include/mlvdb_maxsim.h): the [token, document] reduction behind it.  One pass maps every row to
// the dense id of its document; the scan is the exact scan (kernels_exact.hip) with another sink -- instead of a top-k list
// per query, the minimum distance per (token, document) cell, kept as an order-preserving 64-bit key under atomicMin; the
// rank kernel sums a query's cells per document, in token order, and selects the k smallest (score, dense id).
//
// Nothing depends on the order in which the atomics arrive: a cell ends as the minimum of the keys offered to it, the keys
// order as the fp64 distances do, and the ranking's order is total.
#include <algorithm>

#include "group_table.h"
#include "internal.h"
#include "panel_walk.h"
#include "wave_peel.h"

namespace mlvdb {

namespace {

constexpr unsigned long long kSignBit = 0x8000000000000000ull;

// fp64 distance -> uint64 that orders as the distances do: the mapping kernels_order.hip uses for float columns.  0.0 is
// added first, so -0.0 and +0.0 share a key (and decode as +0.0).
__device__ __forceinline__ unsigned long long maxsim_key(double d) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(d + 0.0);
    return (u >> 63) ? ~u : (u ^ kSignBit);
}
// ... and back.  A cell nothing was offered to (kMaxsimEmpty, all ones) decodes as a NaN.
__device__ __forceinline__ double maxsim_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k ^ kSignBit) : ~k;
    return __longlong_as_double((long long)u);
}

}  // namespace

// row_doc[row] = the dense id of the row's document, or -1 for a tombstoned, masked-out or absent row.  Launch shape of
// where_eval_kernel: 256 threads, grid-stride, whole waves.
__global__ __launch_bounds__(256) void maxsim_slot_kernel(const float* __restrict__ rn, const int64_t* __restrict__ col,
                                                          int64_t total, const long long* __restrict__ keys, uint64_t mask,
                                                          const int32_t* __restrict__ dense, int32_t* __restrict__ row_doc) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int32_t slot = grouped_row_slot(rn, col, i, total, keys, mask);
        row_doc[i] = slot >= 0 ? dense[slot] : -1;
    }
}

hipError_t launch_maxsim_slot(const float* rn, const int64_t* col, int64_t total, const long long* keys, uint64_t slots,
                              const int32_t* dense, int32_t* row_doc, hipStream_t s) {
    if (total <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 256 * 16);
    maxsim_slot_kernel<<<(unsigned)blocks, 256, 0, s>>>(rn, col, total, keys, slots - 1, dense, row_doc);
    return hipGetLastError();
}

// exact_scan_kernel's shape, geometry and arithmetic (plan_exact; accumulate_rows / finish_distance unchanged: every distance
// has the exact scan's bits) over all rows, blockIdx.y selecting a tile of QT tokens of the chunk -- tokens of different
// queries may share a tile, the sink knows tokens only.  Sink: best[token][dense id] = min(key of the distance).  The lanes
// of a wave that hold rows of one document fold their minimum first (wave_peel_min: the 16 rows of a panel are adjacent
// rows, normally of one document), and a plain load skips an atomic that cannot lower the cell -- cells only ever
// decrease, so a stale read only costs a redundant atomic.
template <int SPACE, int QT, int PW, int NW>
__global__ __launch_bounds__(NW * 64) void maxsim_scan_kernel(const MaxsimArgs a, const int nblk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);  // [QT][ld]

    int qid[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int tok = blockIdx.y * QT + t;
        qid[t] = tok < a.ntok ? tok : -1;
    }
    double qinv[QT];
    gather_stage_queries<QT, NW>(qs, a.Qpad, a.qaux, qid, a.ld, qinv);
    // the exact scan's instance of the walk; every row is read once per launch
    panel_walk<SPACE, QT, PW, NW, (QT == 8 ? 4 : 0), /*NT=*/true>(
        a.X, a.ld, a.total, nblk, qs, qinv,
        [&](int64_t row, bool in) { return in ? a.row_doc[row] : -1; },  // -1: tombstoned, masked out or in no document
        [&](int t, int32_t doc, double dist, int32_t) {
            const bool want = doc >= 0 && qid[t] >= 0 && dist == dist;  // (a NaN is never a best distance)
            unsigned long long* const cells = a.best + (int64_t)(qid[t] >= 0 ? qid[t] : 0) * a.ndocs;
            wave_peel_min<16>(want, doc, maxsim_key(dist), [&](int32_t d, unsigned long long key) {
                unsigned long long* const cell = cells + d;
                if (__hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(cell, key);
            });
        });
}

hipError_t launch_maxsim_scan(const MaxsimArgs& a, const ExactPlan& p, hipStream_t s) {
    if (a.ntok <= 0 || a.total <= 0) return hipSuccess;
    if (p.nqtiles > 65535) return hipErrorInvalidValue;
    const size_t lds = (size_t)p.qt * a.ld * sizeof(double);  // the query tile alone: there is no block merge
    return with_exact_tile(a.space, p.qt, [&](auto sp, auto qt, auto pw, auto nw) {
        constexpr auto kern = maxsim_scan_kernel<decltype(sp)::value, decltype(qt)::value, decltype(pw)::value, decltype(nw)::value>;
        // plan_exact's halving keeps the image within kQueryImageMaxLds
        if (hipError_t e = ensure_instance_lds<kern>(lds, kQueryImageMaxLds); e != hipSuccess) return e;
        kern<<<dim3(p.nblk, p.nqtiles), p.threads, lds, s>>>(a, p.nblk);
        return hipGetLastError();
    });
}

// Grid (blocks per query, queries of the chunk), 4 waves.  A lane takes documents g, adjacent lanes adjacent g (the reads of
// best[t][.] coalesce), decodes and sums the query's tokens in the order given -- (((0.0 + b0) + b1) + ...), fp64 -- and
// offers (score, dense id) to its wave's list; a score that is NaN (a token without a best distance) is never admitted.
// The block's four lists are merged through LDS into partial[(query * gridDim.x + block) * k ..], which exact_merge_kernel
// folds.
__global__ __launch_bounds__(256) void maxsim_rank_kernel(const unsigned long long* __restrict__ best,
                                                          const int32_t* __restrict__ tok_off, int32_t ndocs, int32_t k,
                                                          TopEntry* __restrict__ partial) {
    __shared__ double sd[4][64];
    __shared__ int32_t sl[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int q = blockIdx.y;
    const int t0 = tok_off[q], t1 = tok_off[q + 1];
    WaveTopK top;
    top.init();
    // g0 is uniform over the block: every lane of a wave runs the same iterations (the list's shuffles need all of them)
    for (int64_t g0 = (int64_t)blockIdx.x * 256; g0 < ndocs; g0 += (int64_t)gridDim.x * 256) {
        const int64_t gd = g0 + threadIdx.x;
        const bool have = gd < ndocs;
        double score = 0.0;
        for (int t = t0; t < t1; ++t) {
            const unsigned long long key = have ? best[(int64_t)t * ndocs + gd] : ~0ull;
            score = score + maxsim_unkey(key);
        }
        top.offer(have, score, (int32_t)gd, k, lane);
    }
    sd[wave][lane] = top.d;
    sl[wave][lane] = top.l;
    __syncthreads();
    if (wave != 0) return;
    WaveTopK m;
    m.init();
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
        const double cd = sd[w2][lane];
        const int32_t cl = sl[w2][lane];
        m.offer(lane < k && cl != kNoLabel, cd, cl, k, lane);
    }
    if (lane < k) {
        TopEntry e;
        e.d = m.d;
        e.l = m.l;
        e.pad = 0;
        partial[((int64_t)q * gridDim.x + blockIdx.x) * k + lane] = e;
    }
}

int32_t maxsim_rank_blocks(int32_t ndocs) { return (int32_t)std::min<int64_t>(256, std::max<int64_t>(1, ((int64_t)ndocs + 255) / 256)); }

hipError_t launch_maxsim_rank(const unsigned long long* best, const int32_t* tok_off, int32_t nq, int32_t ndocs, int32_t k,
                              int32_t nblk, TopEntry* partial, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    if (k < 1 || k > kWave || nblk < 1 || nq > 65535) return hipErrorInvalidValue;
    maxsim_rank_kernel<<<dim3((unsigned)nblk, (unsigned)nq), 256, 0, s>>>(best, tok_off, ndocs, k, partial);
    return hipGetLastError();
}

}  // namespace mlvdb
