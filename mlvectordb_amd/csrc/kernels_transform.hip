// Linear maps of the stored rows (include/mlvdb_transform.h): out[i][j] = (float)(proj(matrix[j], row_i) - shift[j]).
//   transform_tile_kernel     a register-blocked fp64 tile kernel over a *list* of rows.  A workgroup of 8 waves owns
//                             kTransformRowBlock = 128 consecutive candidates of the ascending label list and kTransformColTile
//                             = 64 output columns.  All waves hold the same 128 candidates -- lane 16g + r of a wave has slice g
//                             of candidate 16p + r for p = 0..7, addressed by its label the way gather_walk addresses a row, so
//                             a slice is still one aligned float4 per column group -- and wave w owns columns 8w .. 8w + 7 of
//                             the tile: acc[8 candidates][8 columns] per lane, 64 accumulators.  A selective filter costs its
//                             matches, and the result is dense in candidate order without a second pass.  The matrix tile goes
//                             through LDS as fp64 in chunks of 32 columns (64 x 32 x 8 B = 16 KiB), converted on the way in, two
//                             buffers: the global loads of chunk c + 1 are issued before the FMAs of chunk c and stored behind
//                             them, one barrier per chunk.  A 16-byte LDS read feeds 16 FMAs: 1 B of LDS per FMA and lane.  The
//                             summation order is the header's: per accumulator the columns of its slice ascending, then
//                             (S0 + S1) + (S2 + S3) by xor-16 / xor-32.  Epilogue: subtract the shift, convert, test isfinite
//                             (a failure stores 1 to the flag word: every writer stores the same value, no atomic); the
//                             128 x 64 fp32 tile goes through LDS over the two matrix buffers (float4 index xor row, so neither
//                             side conflicts) and leaves as 256-byte pieces of the row-major result.  Slots beyond `matched`
//                             read label 0 and are neither tested nor written; columns >= out_dim are not written.  For
//                             out_dim < 64 the tile computes padded zero columns.
//   transform_vectors_kernel  the same function of given vectors (row-major), plain: one wave per vector, lanes over the output
//                             columns, the four slice sums in the stated order.
// The library is built with -ffp-contract=off, restated below for this file.  No scratch, no atomics.
#include "internal.h"

#pragma clang fp contract(off)

namespace mlvdb {

namespace {
constexpr int kPW = kTransformRowBlock / kPanelRows;  // candidates per lane
constexpr int kNP = 8;                                // output columns per wave
constexpr int kNW = kTransformColTile / kNP;          // waves per workgroup
constexpr int kChunkCols = 32;                        // columns per staged chunk: two column groups
constexpr int kBlocksPerSlab = 4096;                  // candidate blocks per grid.y step
constexpr int kQuads = kTransformColTile / 4;         // float4 per row of the output tile
static_assert(kPW == 8 && kNW == 8 && kQuads == 16, "lane group g stores candidates 2g, 2g + 1; 16 threads write one 256-byte row piece");
static_assert(2 * kTransformColTile * kChunkCols * sizeof(double) == kTransformRowBlock * kTransformColTile * sizeof(float),
              "the output tile lies exactly over the two matrix buffers");
}  // namespace

__global__ __launch_bounds__(kNW * 64) void transform_tile_kernel(const TransformArgs a, const int64_t nblocks, const int32_t tiles) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kTransformColTile * kChunkCols * sizeof(double)];
    double(*ps)[kTransformColTile][kChunkCols] = reinterpret_cast<double(*)[kTransformColTile][kChunkCols]>(smem);
    float4* const ot = reinterpret_cast<float4*>(smem);  // [128][16], quad q of row i at i * 16 + (q ^ (i & 15))
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const int tile = blockIdx.x % tiles;
    const int64_t block = (int64_t)blockIdx.y * kBlocksPerSlab + blockIdx.x / tiles;
    if (block >= nblocks) return;  // (block-uniform, before any barrier)
    const int ld = a.ld, nkb = ld >> 4, nchunks = (nkb + 1) >> 1;

    // staging: thread -> matrix row tid / 8 of the tile, float4 tid % 8 of the chunk's 32 columns
    const int sp = tid >> 3, sc = (tid & 7) * 4;
    const float* const msrc = a.Mpad + (int64_t)(tile * kTransformColTile + sp) * ld + sc;
    auto fetch = [&](int c) __attribute__((always_inline)) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c * kChunkCols + sc < ld) v = *reinterpret_cast<const float4*>(msrc + c * kChunkCols);
        return v;
    };
    auto stash = [&](int buf, const float4& v) __attribute__((always_inline)) {
        *reinterpret_cast<double2*>(&ps[buf][sp][sc]) = make_double2((double)v.x, (double)v.y);
        *reinterpret_cast<double2*>(&ps[buf][sp][sc + 2]) = make_double2((double)v.z, (double)v.w);
    };

    // this lane's slice of its eight candidates (a slot beyond the list reads row 0, which exists: matched > 0)
    const int64_t cand0 = block * kTransformRowBlock;
    int32_t lab[kPW];
#pragma unroll
    for (int p = 0; p < kPW; ++p) {
        const int64_t i = cand0 + p * kPanelRows + r;
        lab[p] = i < a.matched ? (a.labels ? a.labels[i] : (int32_t)i) : 0;
    }
    const float* const xg = a.X + g * 4;
    const int pstride = kPanelRows * ld;  // (ld <= 8192)
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
            for (int p = 0; p < kPW; ++p) x[p] = *reinterpret_cast<const float4*>(xg + (int64_t)(lab[p] >> 4) * pstride + ((lab[p] & 15) * 16 + (2 * c + kk) * kGroupFloats));
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
                    const double2 mv = *reinterpret_cast<const double2*>(&q[t][kk * 16 + g * 4 + half * 2]);
#pragma unroll
                    for (int p = 0; p < kPW; ++p) acc[p][t] = __builtin_fma(mv.x, xa[p], acc[p][t]);
#pragma unroll
                    for (int p = 0; p < kPW; ++p) acc[p][t] = __builtin_fma(mv.y, xb[p], acc[p][t]);
                }
            }
        }
        if (more) stash((c + 1) & 1, next);
        __syncthreads();  // chunk c + 1 is staged; buffer c & 1 is free for chunk c + 2 (after the last chunk: for the output tile)
    }

    // the four slices of a candidate meet, (S0 + S1) + (S2 + S3); then the shift, the conversion and the finiteness test.
    // Every lane of a group of four holds the same sums: lane group g keeps candidates 2g and 2g + 1 for the tile.
    const int col0 = tile * kTransformColTile + wave * kNP;
    double sh[kNP];
#pragma unroll
    for (int t = 0; t < kNP; ++t) sh[t] = a.shift[col0 + t];
    bool bad = false;
#pragma unroll
    for (int p = 0; p < kPW; ++p) {
        float f[kNP];
#pragma unroll
        for (int t = 0; t < kNP; ++t) {
            double v = acc[p][t];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            f[t] = (float)(v - sh[t]);
        }
        if ((p >> 1) == g) {
            const int i = p * kPanelRows + r;
            if (cand0 + i < a.matched) {
#pragma unroll
                for (int t = 0; t < kNP; ++t) bad |= col0 + t < a.out_dim && !__builtin_isfinite(f[t]);
            }
            ot[i * kQuads + ((2 * wave) ^ r)] = make_float4(f[0], f[1], f[2], f[3]);
            ot[i * kQuads + ((2 * wave + 1) ^ r)] = make_float4(f[4], f[5], f[6], f[7]);
        }
    }
    if (bad) *a.flag = 1u;
    __syncthreads();

    // 16 threads per 256-byte piece of a result row, 32 rows per step
    const int qd = tid & 15;
    const int col = tile * kTransformColTile + qd * 4;
    const bool whole = (a.out_dim & 3) == 0;  // then every row is 16-byte aligned and col < out_dim covers the float4
#pragma unroll
    for (int step = 0; step < kTransformRowBlock / 32; ++step) {
        const int i = step * 32 + (tid >> 4);
        const int64_t cand = cand0 + i;
        if (cand >= a.matched || col >= a.out_dim) continue;
        const float4 v = ot[i * kQuads + (qd ^ (i & 15))];
        float* const dst = a.out + cand * a.out_dim + col;
        if (whole) {
            *reinterpret_cast<float4*>(dst) = v;
        } else {
            dst[0] = v.x;
            if (col + 1 < a.out_dim) dst[1] = v.y;
            if (col + 2 < a.out_dim) dst[2] = v.z;
            if (col + 3 < a.out_dim) dst[3] = v.w;
        }
    }
}

// grid (n): one wave per vector, lane = output column 64 w + lane of step w
__global__ __launch_bounds__(64) void transform_vectors_kernel(const float* __restrict__ vectors, const int32_t dim,
                                                               const float* __restrict__ matrix, const double* __restrict__ shift,
                                                               const int32_t out_dim, float* __restrict__ out,
                                                               uint32_t* __restrict__ flag) {
    const int lane = threadIdx.x;
    const float* x = vectors + (int64_t)blockIdx.x * dim;
    for (int j = lane; j < out_dim; j += 64) {
        const float* m = matrix + (int64_t)j * dim;
        double S[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c0 = 0; c0 < dim; c0 += 16) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = c0 + 4 * g + i;
                    if (c < dim) S[g] = __builtin_fma((double)m[c], (double)x[c], S[g]);
                }
        }
        const float f = (float)(((S[0] + S[1]) + (S[2] + S[3])) - shift[j]);
        if (!__builtin_isfinite(f)) *flag = 1u;
        out[(int64_t)blockIdx.x * out_dim + j] = f;
    }
}

// ------------------------------------------------------------------------------ host side
hipError_t launch_transform_tiles(const TransformArgs& a, hipStream_t s) {
    if (a.matched <= 0) return hipSuccess;
    if (!a.X || !a.Mpad || !a.shift || !a.out || !a.flag || a.ld <= 0 || a.ld % 16 != 0 || a.out_dim < 1 ||
        a.out_dim > MLVDB_TRANSFORM_MAX_OUT || a.matched > INT32_MAX)
        return hipErrorInvalidValue;
    const int32_t tiles = (a.out_dim + kTransformColTile - 1) / kTransformColTile;
    const int64_t nblocks = (a.matched + kTransformRowBlock - 1) / kTransformRowBlock;
    const int64_t per_slab = nblocks < kBlocksPerSlab ? nblocks : kBlocksPerSlab;
    const dim3 grid((unsigned)(per_slab * tiles), (unsigned)((nblocks + kBlocksPerSlab - 1) / kBlocksPerSlab));
    transform_tile_kernel<<<grid, kNW * 64, 0, s>>>(a, nblocks, tiles);
    return hipGetLastError();
}

hipError_t launch_transform_vectors(const float* vectors, int64_t n, int32_t dim, const float* matrix, const double* shift,
                                    int32_t out_dim, float* out, uint32_t* flag, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!vectors || !matrix || !shift || !out || !flag || dim < 1 || out_dim < 1 || out_dim > MLVDB_TRANSFORM_MAX_OUT || n > (1 << 24))
        return hipErrorInvalidValue;
    transform_vectors_kernel<<<(unsigned)n, 64, 0, s>>>(vectors, dim, matrix, shift, out_dim, out, flag);
    return hipGetLastError();
}

}  // namespace mlvdb
