// Bit codes from the stored rows (include/mlvdb_project.h): bit j of a row = proj(planes[j], row) > thresholds[j].
//   project_planes_kernel   a register-blocked fp64 tile kernel.  A workgroup of 8 waves owns kProjectRowBlock = 128 rows
//                           (8 panels) and kProjectPlaneTile = 64 planes, one code word.  All waves hold the same 128 rows --
//                           lane 16g + r of a wave has slice g of row r of each panel, the panel's float4 per column group,
//                           converted to fp64 once -- and wave w owns planes 8w .. 8w + 7 of the tile: acc[8 rows][8 planes]
//                           per lane, 64 accumulators.  The plane tile goes through LDS as fp64 in chunks of two column
//                           groups (64 planes x 32 columns = 16 KiB), converted on the way in, two buffers: the global loads
//                           of chunk c + 1 are issued before the FMAs of chunk c and stored behind them, one barrier per
//                           chunk.  A 16-byte LDS read (two plane values) feeds 16 FMAs: 1 B of LDS per FMA and lane, where
//                           accumulate_group with PW rows reads 8 / PW.  The summation order is the header's: per accumulator
//                           the columns of its slice ascending, then (S0 + S1) + (S2 + S3) by xor-16 / xor-32.  Each wave
//                           leaves one byte per row in LDS; thread i < 128 reads row i's eight bytes as the code word and
//                           writes it with one store; the workgroup of plane tile 0 writes the slot.  No atomics.
//   project_sign_kernel     sign mode, bandwidth-bound: one lane per (row, word), 16 rows x 4 words per wave; a lane reads its
//                           row's four 64-byte pieces and packs 64 compares by shifts.
//   project_vectors_kernel  the same function of given vectors (row-major), plain: one wave per vector, one lane per plane,
//                           the four slice sums in the stated order, the word by ballot.
// The library is built with -ffp-contract=off, restated below for this file.  No scratch.
#include "internal.h"

#pragma clang fp contract(off)

namespace mlvdb {

namespace {
constexpr int kPW = kProjectRowBlock / kPanelRows;  // panels per workgroup, each lane one row of each
constexpr int kNP = 8;                              // planes per wave
constexpr int kNW = kProjectPlaneTile / kNP;        // waves per workgroup
constexpr int kChunkCols = 32;                      // columns per staged chunk: two column groups
constexpr int kBlocksPerSlab = 4096;                // row blocks per grid.y step
static_assert(kPW == 8 && kNW == 8, "a row's eight wave bytes are read back as one 64-bit word, thread i < 128 owns row i");
static_assert(kTileRows % kProjectRowBlock == 0, "a row block never reaches past the capacity");

__device__ __forceinline__ bool project_candidate(const ProjectArgs& a, int64_t row) {
    const float nrm = a.rn[row];
    return nrm == nrm && (!a.mask || a.mask[row] != 0);
}

// row < total: the word `w` of its code -> the pool (zeros for a row that is no candidate); word 0 also writes the slot
__device__ __forceinline__ void project_store(const ProjectArgs& a, int64_t row, int w, uint64_t word) {
    const bool cand = project_candidate(a, row);
    const int64_t off = a.base + row * a.words;
    a.pool[off + w] = cand ? (int64_t)word : 0;
    if (w == 0 && cand) a.slots[row] = (off << 8) | a.words;
}
}  // namespace

__global__ __launch_bounds__(kNW * 64) void project_planes_kernel(const ProjectArgs a, const float* __restrict__ Ppad,
                                                                  const int64_t nblocks) {
    __shared__ __attribute__((aligned(16))) double ps[2][kProjectPlaneTile][kChunkCols];
    __shared__ __attribute__((aligned(8))) uint8_t code[kProjectRowBlock][kNW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const int tile = blockIdx.x % a.words;
    const int64_t block = (int64_t)blockIdx.y * kBlocksPerSlab + blockIdx.x / a.words;
    if (block >= nblocks) return;  // (block-uniform, before any barrier)
    const int ld = a.ld, nkb = ld >> 4, nchunks = (nkb + 1) >> 1;

    // staging: thread -> plane tid / 8 of the tile, float4 tid % 8 of the chunk's 32 columns
    const int sp = tid >> 3, sc = (tid & 7) * 4;
    const float* const psrc = Ppad + (int64_t)(tile * kProjectPlaneTile + sp) * ld + sc;
    auto fetch = [&](int c) __attribute__((always_inline)) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c * kChunkCols + sc < ld) v = *reinterpret_cast<const float4*>(psrc + c * kChunkCols);
        return v;
    };
    auto stash = [&](int buf, const float4& v) __attribute__((always_inline)) {
        *reinterpret_cast<double2*>(&ps[buf][sp][sc]) = make_double2((double)v.x, (double)v.y);
        *reinterpret_cast<double2*>(&ps[buf][sp][sc + 2]) = make_double2((double)v.z, (double)v.w);
    };

    // (capacity is a multiple of kTileRows, hence of the row block: all eight panels lie inside X)
    const float* const base = a.X + block * (int64_t)(kProjectRowBlock * ld) + lane_group_offset(lane);
    const int64_t pstride = (int64_t)kPanelRows * ld;
    double acc[kPW][kNP];
#pragma unroll
    for (int p = 0; p < kPW; ++p)
#pragma unroll
        for (int t = 0; t < kNP; ++t) acc[p][t] = 0.0;

    stash(0, fetch(0));
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const bool more = c + 1 < nchunks;
        float4 next = make_float4(0.f, 0.f, 0.f, 0.f);
        if (more) next = fetch(c + 1);
        const double(*q)[kChunkCols] = ps[c & 1] + wave * kNP;
        const int ng = nkb - 2 * c < 2 ? 1 : 2;
#pragma unroll 1
        for (int kk = 0; kk < ng; ++kk) {
            float4 x[kPW];
#pragma unroll
            for (int p = 0; p < kPW; ++p) x[p] = *reinterpret_cast<const float4*>(base + p * pstride + (int64_t)(2 * c + kk) * kGroupFloats);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                double xa[kPW], xb[kPW];
#pragma unroll
                for (int p = 0; p < kPW; ++p) {
                    xa[p] = (double)(half ? x[p].z : x[p].x);
                    xb[p] = (double)(half ? x[p].w : x[p].y);
                }
#pragma unroll
                for (int t = 0; t < kNP; ++t) {
                    const double2 pv = *reinterpret_cast<const double2*>(&q[t][kk * 16 + g * 4 + half * 2]);
#pragma unroll
                    for (int p = 0; p < kPW; ++p) acc[p][t] = __builtin_fma(pv.x, xa[p], acc[p][t]);
#pragma unroll
                    for (int p = 0; p < kPW; ++p) acc[p][t] = __builtin_fma(pv.y, xb[p], acc[p][t]);
                }
            }
        }
        if (more) stash((c + 1) & 1, next);
        __syncthreads();  // chunk c + 1 is staged; buffer c & 1 is free for chunk c + 2
    }

    // the four slices of a row meet, (S0 + S1) + (S2 + S3); eight compares -> this wave's byte of the row's word
    double thr[kNP];
#pragma unroll
    for (int t = 0; t < kNP; ++t) thr[t] = a.thr[tile * kProjectPlaneTile + wave * kNP + t];
#pragma unroll
    for (int p = 0; p < kPW; ++p) {
        uint32_t b = 0;
#pragma unroll
        for (int t = 0; t < kNP; ++t) {
            double v = acc[p][t];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            b |= (v > thr[t] ? 1u : 0u) << t;  // (a NaN compares false)
        }
        if (g == 0) code[p * kPanelRows + r][wave] = (uint8_t)b;
    }
    __syncthreads();
    if (tid < kProjectRowBlock) {
        const int64_t row = block * kProjectRowBlock + tid;
        if (row < a.total) project_store(a, row, tile, *reinterpret_cast<const uint64_t*>(code[tid]));
    }
}

// grid (ceil(words / 4), ceil(panels / 4)); wave = one panel x four words, lane 16 q + r = row r, word 4 blockIdx.x + q
__global__ __launch_bounds__(256) void project_sign_kernel(const ProjectArgs a, const int64_t panel0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, w = blockIdx.x * 4 + (lane >> 4);
    const int64_t panel = panel0 + (int64_t)blockIdx.y * 4 + wave;
    const int64_t row = panel * kPanelRows + r;
    if (w >= a.words || row >= a.total) return;  // (no barrier below)
    const int nkb = a.ld >> 4;
    uint64_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int kb = w * 4 + k;
        if (kb >= nkb) break;
        const float* src = a.X + panel * (int64_t)(kPanelRows * a.ld) + (int64_t)kb * kGroupFloats + r * 16;
        float v[16];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 f = *reinterpret_cast<const float4*>(src + 4 * i);
            v[4 * i] = f.x, v[4 * i + 1] = f.y, v[4 * i + 2] = f.z, v[4 * i + 3] = f.w;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = kb * 16 + j;
            if (c < a.dim && (double)v[j] > a.thr[c]) word |= 1ull << (k * 16 + j);
        }
    }
    project_store(a, row, w, word);
}

// grid (n): one wave per vector, lane = plane 64 w + lane of word w
__global__ __launch_bounds__(64) void project_vectors_kernel(const float* __restrict__ vectors, const int32_t dim,
                                                             const float* __restrict__ planes, const double* __restrict__ thr,
                                                             const int32_t words, uint64_t* __restrict__ out) {
    const int lane = threadIdx.x;
    const float* x = vectors + (int64_t)blockIdx.x * dim;
    for (int w = 0; w < words; ++w) {
        const int j = w * 64 + lane;
        bool bit;
        if (planes) {
            const float* p = planes + (int64_t)j * dim;
            double S[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c0 = 0; c0 < dim; c0 += 16) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = c0 + 4 * g + i;
                        if (c < dim) S[g] = __builtin_fma((double)p[c], (double)x[c], S[g]);
                    }
            }
            bit = (S[0] + S[1]) + (S[2] + S[3]) > thr[j];
        } else {
            bit = j < dim && (double)x[j] > thr[j];
        }
        const uint64_t word = __ballot(bit);
        if (lane == 0) out[(int64_t)blockIdx.x * words + w] = word;
    }
}

// ------------------------------------------------------------------------------ host side
namespace {
bool project_args_ok(const ProjectArgs& a) {
    return a.total > 0 && a.ld > 0 && a.ld % 16 == 0 && a.dim > 0 && a.dim <= a.ld && a.words >= 1 && a.words <= MLVDB_BITS_MAX_WORDS &&
           a.X && a.rn && a.thr && a.pool && a.slots && a.base >= 0;
}
}  // namespace

hipError_t launch_project_planes(const ProjectArgs& a, const float* Ppad, hipStream_t s) {
    if (!project_args_ok(a) || !Ppad) return hipErrorInvalidValue;
    const int64_t nblocks = (a.total + kProjectRowBlock - 1) / kProjectRowBlock;
    const int64_t per_slab = nblocks < kBlocksPerSlab ? nblocks : kBlocksPerSlab;
    const dim3 grid((unsigned)(per_slab * a.words), (unsigned)((nblocks + kBlocksPerSlab - 1) / kBlocksPerSlab));
    project_planes_kernel<<<grid, kNW * 64, 0, s>>>(a, Ppad, nblocks);
    return hipGetLastError();
}

hipError_t launch_project_sign(const ProjectArgs& a, hipStream_t s) {
    if (!project_args_ok(a) || (a.dim + 63) / 64 != a.words) return hipErrorInvalidValue;
    const int64_t groups = (((a.total + 15) >> 4) + 3) / 4;  // workgroups of four panels
    for (int64_t g0 = 0; g0 < groups; g0 += 65535) {
        const dim3 grid((unsigned)((a.words + 3) / 4), (unsigned)(groups - g0 < 65535 ? groups - g0 : 65535));
        project_sign_kernel<<<grid, 256, 0, s>>>(a, g0 * 4);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_project_vectors(const float* vectors, int64_t n, int32_t dim, const float* planes, const double* thr,
                                  int32_t words, uint64_t* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!vectors || !thr || !out || dim < 1 || words < 1 || words > MLVDB_BITS_MAX_WORDS || n > (1 << 24)) return hipErrorInvalidValue;
    project_vectors_kernel<<<(unsigned)n, 64, 0, s>>>(vectors, dim, planes, thr, words, out);
    return hipGetLastError();
}

}  // namespace mlvdb
