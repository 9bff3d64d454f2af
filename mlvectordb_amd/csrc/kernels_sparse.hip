// Sparse vector columns (include/mlvdb_sparse.h): the exact inner product of a batch of sparse queries with every live,
// present (and matching) row's sparse vector, and its top-k.  DESIGN.md 11.13.
//
// A tile is up to QT queries whose term union U (sorted, <= kSparseMaxUnion terms) and dense weights W[nu][QT] (0 where a
// query lacks the term) sit in LDS.  blockIdx.y is the tile, blockIdx.x strides over groups of 16 rows: 16 lanes per row,
// four rows per wave step.  Lane j of a row's group takes the row's elements j, j + 16, ... in that order; an element
// passes a one-read LDS bitmap of (term & (B - 1)) before U is searched; a hit at u is QT fma's into fp64 accumulators.
// The 16 partial sums are folded by a fixed butterfly (xor 1, 2, 4, 8 as DPP row operations: fp addition commutes, so every
// lane ends with the same bits), and each query's WaveTopK is offered (-score, row) by lane 0 of each group.
//
// A pair's score is a pure function of the two vectors: the element -> lane assignment and both summation orders depend on
// the row's own element order alone, and a term another query of the tile brought into U adds fma(w, 0, acc), which leaves
// acc as it is (acc is never -0: it starts at +0 and x + (-0) == x).
#include "internal.h"
#include "panel_walk.h"  // exact_merge_kernel
#include "sparse_dpp.h"  // the bitmap's size and the 16-lane fold, shared with the gathered scorer (kernels_hybrid.hip)

namespace mlvdb {

namespace {
constexpr int kSparseLoads = 4;  // elements a lane loads before it looks any of them up: 64 elements of a row per round
}  // namespace

template <int QT>
__global__ __launch_bounds__(256) void sparse_scan_kernel(const int64_t* __restrict__ slots, const int64_t* __restrict__ pool,
                                                          const float* __restrict__ rn, const uint8_t* __restrict__ mask,
                                                          int64_t total, const SparseTile* __restrict__ tiles,
                                                          const int32_t* __restrict__ U, const float* __restrict__ W, int32_t k,
                                                          TopEntry* __restrict__ partial) {
    static_assert(QT == 8, "the weight rows are read as two float4");
    __shared__ int32_t sU[kSparseMaxUnion];
    __shared__ __attribute__((aligned(16))) float sW[kSparseMaxUnion * QT];
    __shared__ unsigned int sB[kSparseBitmapWords];
    __shared__ double sd[4][64];
    __shared__ int32_t sl[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int j = lane & 15;
    const SparseTile tile = tiles[blockIdx.y];
    const int nu = tile.nu;
    for (int c = threadIdx.x; c < kSparseBitmapWords; c += 256) sB[c] = 0u;
    for (int c = threadIdx.x; c < nu; c += 256) sU[c] = U[tile.u0 + c];
    for (int c = threadIdx.x; c < nu * QT; c += 256) sW[c] = W[(int64_t)tile.u0 * QT + c];
    __syncthreads();
    for (int c = threadIdx.x; c < nu; c += 256) {
        const unsigned int t = (unsigned int)sU[c] & (kSparseBitmapBits - 1);
        atomicOr(&sB[t >> 5], 1u << (t & 31));
    }
    __syncthreads();

    WaveTopK top[QT];
#pragma unroll
    for (int i = 0; i < QT; ++i) top[i].init();

    // The slot of `row` if the row is a candidate (live, in the mask, with a vector), else INT64_MIN.
    auto candidate_slot = [&](int64_t row) -> int64_t {
        if (row >= total) return INT64_MIN;
        const float n = rn[row];
        if (n != n || (mask && mask[row] == 0)) return INT64_MIN;
        return slots[row];
    };

    // r0 is uniform over the block: every lane of a wave runs the same iterations (the lists' shuffles need all of them).
    // The next step's slot is loaded before this step's elements, and a lane's elements four at a time before any of them
    // is looked up: the walk is a chain of dependent loads (slot -> element -> LDS), and what hides it is loads in flight.
    const int64_t stride = (int64_t)gridDim.x * 16;
    int64_t slot_next = candidate_slot((int64_t)blockIdx.x * 16 + wave * 4 + g);
    for (int64_t r0 = (int64_t)blockIdx.x * 16; r0 < total; r0 += stride) {
        const int64_t row = r0 + wave * 4 + g;
        const int64_t slot = slot_next;
        slot_next = r0 + stride < total ? candidate_slot(row + stride) : INT64_MIN;
        const bool have = slot != INT64_MIN;
        const int len = have ? (int)(slot & 0xff) : 0;
        const int64_t* src = pool + (slot >> 8);  // (never read when len == 0)
        double acc[QT];
#pragma unroll
        for (int i = 0; i < QT; ++i) acc[i] = 0.0;
        for (int e0 = j; e0 < len; e0 += 16 * kSparseLoads) {
            int64_t els[kSparseLoads];
#pragma unroll
            for (int u = 0; u < kSparseLoads; ++u) els[u] = e0 + 16 * u < len ? src[e0 + 16 * u] : 0;
#pragma unroll
            for (int u = 0; u < kSparseLoads; ++u) {  // in ascending element order: the order of a lane's additions is fixed
                if (e0 + 16 * u >= len) continue;
                const int64_t el = els[u];
                const int32_t term = (int32_t)(el >> 32);
                const unsigned int t = (unsigned int)term & (kSparseBitmapBits - 1);
                if (!((sB[t >> 5] >> (t & 31)) & 1u)) continue;
                int lo = 0, hi = nu;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sU[mid] < term) lo = mid + 1; else hi = mid;
                }
                if (lo >= nu || sU[lo] != term) continue;
                const double w = (double)__int_as_float((int32_t)(el & 0xffffffffll));
                const float4 w0 = *reinterpret_cast<const float4*>(&sW[lo * QT]);
                const float4 w1 = *reinterpret_cast<const float4*>(&sW[lo * QT + 4]);
                acc[0] = fma(w, (double)w0.x, acc[0]);
                acc[1] = fma(w, (double)w0.y, acc[1]);
                acc[2] = fma(w, (double)w0.z, acc[2]);
                acc[3] = fma(w, (double)w0.w, acc[3]);
                acc[4] = fma(w, (double)w1.x, acc[4]);
                acc[5] = fma(w, (double)w1.y, acc[5]);
                acc[6] = fma(w, (double)w1.z, acc[6]);
                acc[7] = fma(w, (double)w1.w, acc[7]);
            }
        }
#pragma unroll
        for (int i = 0; i < QT; ++i) {
            if (i < tile.nq) {  // (uniform)
                const double score = row16_sum(acc[i]);
                top[i].offer(have && j == 0, -score, (int32_t)row, k, lane);
            }
        }
    }

    // the block's four lists of each query -> partial[((q0 + i) * gridDim.x + block) * k ..], the input of exact_merge_kernel<true>
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        if (i >= tile.nq) break;  // (uniform)
        sd[wave][lane] = top[i].d;
        sl[wave][lane] = top[i].l;
        __syncthreads();
        if (wave == 0) {
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
                partial[((int64_t)(tile.q0 + i) * gridDim.x + blockIdx.x) * k + lane] = e;
            }
        }
        __syncthreads();
    }
}

int32_t sparse_scan_blocks(int64_t total, int64_t nq, int32_t k) {
    // <= 64 MiB of partial entries, <= 1024 blocks per tile (four per CU), one block per 16 rows at the most
    const int64_t by_mem = (int64_t)(64u << 20) / (std::max<int64_t>(nq, 1) * k * (int64_t)sizeof(TopEntry));
    const int64_t by_rows = (total + 15) / 16;
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>({kSparseMaxBlocks, by_mem, by_rows}));
}

hipError_t launch_sparse_scan(const int64_t* slots, const int64_t* pool, const float* rn, const uint8_t* mask, int64_t total,
                              const SparseTile* tiles, int32_t ntiles, const int32_t* U, const float* W, int32_t k,
                              int32_t nblk, TopEntry* partial, hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    if (k < 1 || k > kWave || nblk < 1 || ntiles > 65535 || total <= 0 || total > INT32_MAX) return hipErrorInvalidValue;
    sparse_scan_kernel<kSparseQT><<<dim3((unsigned)nblk, (unsigned)ntiles), 256, 0, s>>>(slots, pool, rn, mask, total, tiles, U,
                                                                                       W, k, partial);
    return hipGetLastError();
}

hipError_t launch_sparse_merge(const TopEntry* partial, int32_t nq, int32_t nblk, int32_t k, int64_t* out_labels,
                               float* out_score, int32_t* out_counts, double* out_s64, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    // the exact scan's merge with the signs turned back (panel_walk.h); every query of the pass is selected
    exact_merge_kernel<true><<<(unsigned)nq, 256, 0, s>>>(partial, nullptr, nullptr, nblk, k, out_labels, out_score, out_counts,
                                                          out_s64);
    return hipGetLastError();
}

}  // namespace mlvdb
