// Row moments (include/mlvdb_moments.h): the column sums and the Gram matrix X^T X of the candidate rows, in fp64.
//   moments_tile_kernel   a register-blocked fp64 tile kernel that reduces over ROWS (every other tile kernel here reduces over
//                         columns and keeps rows apart).  A workgroup of 4 waves owns one pair (I, J), I <= J, of column tiles
//                         of kMomentsTile = 128 and one slab of kMomentsSlab = 4096 rows.  Thread (ti, tj) = (tid / 16, tid % 16)
//                         holds acc[8][8]: the entries (i, j) with i in {4 ti .. 4 ti + 3} u {64 + 4 ti ..} of strip I and j in
//                         {4 tj .. 4 tj + 3} u {64 + 4 tj ..} of strip J -- 64 accumulators, each of which meets the slab's rows
//                         in ascending label, one FMA per row: the header's order, with no cross-lane step at all.  (The
//                         products are exact in fp64, so the FMA rounds as multiply-then-add does.)
//                         The rows go through LDS as fp32, a chunk of one panel (16 rows) at a time: the two strips are 8
//                         column groups each, 8 contiguous 1 KiB blocks of the panel layout, and a thread moves two float4 of
//                         each.  The candidate test is applied once, there: a row that is no candidate is stored as zeros
//                         (selected, never multiplied).  Two buffers: the global loads of chunk c + 1 are issued before the FMAs
//                         of chunk c and stored behind them, one barrier per chunk.  A row of a strip is 144 floats apart, so
//                         the staging stores of a wave (16 rows x 64 B) spread over all banks; a thread reads its row values as
//                         four float4 (two of them a broadcast within 16 lanes, two contiguous over 16 lanes) for 64 FMAs: 1 B
//                         of LDS per FMA and lane, and 16 conversions.  fp64 in LDS would save the conversions and read 2 B per
//                         FMA, which is the whole LDS rate at the full FMA rate.  A diagonal pair stages one strip and also
//                         keeps the slab's column sums of its strip: thread tid < 128 adds column tid of the staged chunk, row
//                         after row, into one more accumulator.  The tile goes to the batch's partials; no atomics.
//   moments_fold_kernel   one thread per entry of the upper triangle of tiles: the batch's slab partials are added in
//                         ascending slab order into gram[i][j], and the same value is written to gram[j][i]; blockIdx.y ==
//                         npairs folds the column sums.  The first batch starts from +0.0, so nothing is cleared beforehand.
// The library is built with -ffp-contract=off, restated below for this file.  No scratch.
#include "internal.h"

#pragma clang fp contract(off)

namespace mlvdb {

namespace {
constexpr int kT = kMomentsTile;
constexpr int kThreads = 256;
constexpr int kChunkRows = kPanelRows;       // rows per staged chunk: one panel
constexpr int kStripGroups = kT / 16;        // column groups per strip
constexpr int kRowStride = kT + 16;          // floats between two rows of a strip in LDS (64 B past a multiple of 256 B)
constexpr int kFoldBlocks = kT * kT / kThreads;
static_assert(kT == 128 && kThreads == 256 && kStripGroups == 8, "thread (ti, tj) owns 8 x 8 entries; a thread stages 2 float4 per strip");
static_assert(kMomentsSlab % kChunkRows == 0, "a slab is whole panels");
static_assert(MLVDB_MOMENTS_MAX_DIM <= kFoldBlocks * kThreads, "the fold's sums row has one thread per column");
static_assert((size_t)(MLVDB_MOMENTS_MAX_DIM / kT) * (MLVDB_MOMENTS_MAX_DIM / kT + 1) / 2 * kT * kT * sizeof(double) <= kMomentsPartialBytes,
              "one slab's tiles fit the bound");

// pair p of the upper triangle, numbered row by row -> (I, J), I <= J
__device__ __forceinline__ void moments_pair(int p, const int tiles, int& I, int& J) {
    I = 0;
    while (p >= tiles - I) {
        p -= tiles - I;
        ++I;
    }
    J = I + p;
}

// entry k of a thread's eight along one side of the tile, for its index t along that side
__device__ __forceinline__ int moments_entry(int t, int k) { return (k < 4 ? 0 : kT / 2 - 4) + 4 * t + k; }

struct MomentsChunk {
    float4 v[4];  // strip I groups g, g + 4; strip J groups g, g + 4
    bool cand;
};
}  // namespace

__global__ __launch_bounds__(kThreads) void moments_tile_kernel(const MomentsArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[2][2][kChunkRows][kRowStride];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int pair = blockIdx.x % a.npairs, slab_local = blockIdx.x / a.npairs;
    int I, J;
    moments_pair(pair, a.tiles, I, J);
    const bool diag = I == J;
    const int64_t row0 = (a.slab0 + slab_local) * (int64_t)kMomentsSlab;  // (< total: the host launches no slab beyond it)
    const int64_t left = a.total - row0;
    const int nchunks = (int)((left < kMomentsSlab ? left : kMomentsSlab) + kChunkRows - 1) / kChunkRows;
    const int ld = a.ld, nkb = ld >> 4;

    // staging: thread -> row sr of the panel, float4 sq of column groups sg and sg + 4 of each strip
    const int sg = tid >> 6, sr = (tid & 63) >> 2, sq = tid & 3;
    const float* const src = a.X + (row0 >> 4) * (int64_t)(kPanelRows * ld) + (tid & 63) * 4;
    auto fetch = [&](int c, MomentsChunk& ch) __attribute__((always_inline)) {
        const float* p = src + (int64_t)c * (kPanelRows * ld);  // (a panel below ceil(total / 16): inside the capacity)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int kb = (k < 2 ? I : J) * kStripGroups + sg + 4 * (k & 1);
            ch.v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kb < nkb && (k < 2 || !diag)) ch.v[k] = *reinterpret_cast<const float4*>(p + (int64_t)kb * kGroupFloats);
        }
        const int64_t row = row0 + c * kChunkRows + sr;
        ch.cand = false;
        if (row < a.total) {
            const float nrm = a.rn[row];
            ch.cand = nrm == nrm && (!a.mask || a.mask[row] != 0);
        }
    };
    auto stash = [&](int buf, const MomentsChunk& ch) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < 2 || !diag) {
                const float4 v = ch.v[k];  // a row that is no candidate is selected to zero: its bytes may be anything
                *reinterpret_cast<float4*>(&xs[buf][k >> 1][sr][(sg + 4 * (k & 1)) * 16 + sq * 4]) =
                    make_float4(ch.cand ? v.x : 0.f, ch.cand ? v.y : 0.f, ch.cand ? v.z : 0.f, ch.cand ? v.w : 0.f);
            }
    };

    double acc[8][8], sum = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.0;
    const bool sums = diag && tid < kT;  // (wave-uniform) thread tid < 128 of a diagonal pair: column tid of the strip

    MomentsChunk next;
    fetch(0, next);
    stash(0, next);
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const bool more = c + 1 < nchunks;
        if (more) fetch(c + 1, next);
        const float* const pa = &xs[c & 1][0][0][4 * ti];
        const float* const pb = &xs[c & 1][diag ? 0 : 1][0][4 * tj];
#pragma unroll 4
        for (int r = 0; r < kChunkRows; ++r) {
            const float4 a0 = *reinterpret_cast<const float4*>(pa + r * kRowStride);
            const float4 a1 = *reinterpret_cast<const float4*>(pa + r * kRowStride + kT / 2);
            const float4 b0 = *reinterpret_cast<const float4*>(pb + r * kRowStride);
            const float4 b1 = *reinterpret_cast<const float4*>(pb + r * kRowStride + kT / 2);
            const double xa[8] = {(double)a0.x, (double)a0.y, (double)a0.z, (double)a0.w, (double)a1.x, (double)a1.y, (double)a1.z, (double)a1.w};
            const double xb[8] = {(double)b0.x, (double)b0.y, (double)b0.z, (double)b0.w, (double)b1.x, (double)b1.y, (double)b1.z, (double)b1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_fma(xa[i], xb[j], acc[i][j]);
        }
        if (sums) {
#pragma unroll
            for (int r = 0; r < kChunkRows; ++r) sum += (double)xs[c & 1][0][r][tid];
        }
        if (more) stash((c + 1) & 1, next);
        __syncthreads();  // chunk c + 1 is staged; buffer c & 1 is free for chunk c + 2
    }

    double* const out = a.part + ((int64_t)slab_local * a.npairs + pair) * (kT * kT);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double* const o = out + moments_entry(ti, i) * kT + 4 * tj;
        *reinterpret_cast<double2*>(o) = make_double2(acc[i][0], acc[i][1]);
        *reinterpret_cast<double2*>(o + 2) = make_double2(acc[i][2], acc[i][3]);
        *reinterpret_cast<double2*>(o + kT / 2) = make_double2(acc[i][4], acc[i][5]);
        *reinterpret_cast<double2*>(o + kT / 2 + 2) = make_double2(acc[i][6], acc[i][7]);
    }
    if (sums) a.part_sums[(int64_t)slab_local * (a.tiles * kT) + I * kT + tid] = sum;
}

// grid (kFoldBlocks, npairs + 1)
__global__ __launch_bounds__(kThreads) void moments_fold_kernel(const MomentsArgs a, const bool first) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if ((int)blockIdx.y == a.npairs) {  // the column sums
        if (e >= a.dim) return;
        double acc = first ? 0.0 : a.sums[e];
        for (int s = 0; s < a.nslabs; ++s) acc += a.part_sums[(int64_t)s * (a.tiles * kT) + e];
        a.sums[e] = acc;
        return;
    }
    int I, J;
    moments_pair(blockIdx.y, a.tiles, I, J);
    const int i = I * kT + (e >> 7), j = J * kT + (e & (kT - 1));
    if (i >= a.dim || j >= a.dim) return;
    double* const g = a.gram + (int64_t)i * a.dim + j;
    double acc = first ? 0.0 : *g;
    const double* p = a.part + (int64_t)blockIdx.y * (kT * kT) + e;
    for (int s = 0; s < a.nslabs; ++s) acc += p[(int64_t)s * a.npairs * (kT * kT)];
    *g = acc;
    if (I != J) a.gram[(int64_t)j * a.dim + i] = acc;  // (a diagonal tile holds both of its halves, with the same bits)
}

// ------------------------------------------------------------------------------ host side
namespace {
bool moments_args_ok(const MomentsArgs& a) {
    return a.total > 0 && a.ld > 0 && a.ld % 16 == 0 && a.dim > 0 && a.dim <= a.ld && a.dim <= MLVDB_MOMENTS_MAX_DIM &&
           a.tiles == moments_tiles(a.ld) && a.npairs == moments_pairs(a.tiles) && a.slab0 >= 0 && a.nslabs >= 1 &&
           a.nslabs <= moments_batch(a.npairs) && (a.slab0 + a.nslabs - 1) * (int64_t)kMomentsSlab < a.total && a.X && a.rn &&
           a.part && a.part_sums && a.gram && a.sums;
}
}  // namespace

hipError_t launch_moments_tiles(const MomentsArgs& a, hipStream_t s) {
    if (!moments_args_ok(a)) return hipErrorInvalidValue;
    moments_tile_kernel<<<(unsigned)(a.npairs * a.nslabs), kThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_moments_fold(const MomentsArgs& a, bool first, hipStream_t s) {
    if (!moments_args_ok(a)) return hipErrorInvalidValue;
    moments_fold_kernel<<<dim3(kFoldBlocks, (unsigned)(a.npairs + 1)), kThreads, 0, s>>>(a, first);
    return hipGetLastError();
}

}  // namespace mlvdb
