// Binary vector columns (include/mlvdb_bits.h): the exact Hamming or Jaccard distance of a batch of bit codes to every live,
// (matching) row that holds a code of the same width, and its top-k.  DESIGN.md 11.17.
//
// A tile is up to kBitsQT consecutive queries of the pass.  blockIdx.y is the tile, blockIdx.x strides over groups of
// 256 / L rows: L lanes per row (the smallest power of two >= words / 2, at most 16), 64 / L rows per wave step.  Lane j of a
// row's group takes the row's words 2j and 2j + 1 -- for a code of more than 32 words again at 32, 64, ... further on -- and a
// word the code does not have is 0 on both sides, which adds nothing to any count.  Up to 32 words a lane keeps its two words
// of every query of the tile in registers; wider codes read the tile's queries from LDS.  Per word and query the work is one
// `and` and one popcount into an int32, i = popcount(q & x); the row's own popcount px is counted once per row and the
// query's pq comes from the host, so both metrics read the same three integers: Hamming is pq + px - 2i, Jaccard's union
// pq + px - i.  The L partial counts are folded by __shfl_xor (integer addition commutes: every lane ends with the same sum),
// and each query's WaveTopK is offered (distance, row) by lane 0 of each group.
//
// The distances are integers (Hamming) or one fp64 division of two integers (Jaccard): a pair's distance is a pure function of
// the two codes.  The block's lists leave as launch_exact_merge's input.
#include "internal.h"

namespace mlvdb {

namespace {
// two adjacent words of a code: a code starts wherever the pool's append left it, so 8-byte alignment is all there is
struct __attribute__((packed, aligned(8))) WordPair {
    uint64_t a, b;
};
}  // namespace

template <int L, bool LDSQ>
__global__ __launch_bounds__(256) void bits_scan_kernel(const int64_t* __restrict__ slots, const int64_t* __restrict__ pool,
                                                        const float* __restrict__ rn, const uint8_t* __restrict__ mask,
                                                        int64_t total, const uint64_t* __restrict__ queries,
                                                        const int32_t* __restrict__ qpop, int32_t nq, int32_t words, int32_t metric,
                                                        int32_t k, TopEntry* __restrict__ partial) {
    constexpr int QT = kBitsQT;
    constexpr int RW = 64 / L;  // rows per wave step
    static_assert(L == 1 || L == 2 || L == 4 || L == 8 || L == 16, "a group is a power of two of lanes inside a row of 16");
    extern __shared__ __attribute__((aligned(16))) uint64_t sQ[];  // LDSQ: [QT][words]
    __shared__ double sd[4][64];
    __shared__ int32_t sl[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane / L;
    const int j = lane % L;
    const int q0 = blockIdx.y * QT;
    const int tnq = min(QT, nq - q0);

    // the tile's queries: this lane's two words of each in registers, or all of them in LDS (absent queries and words are 0)
    uint64_t qa[QT], qb[QT];
    if constexpr (LDSQ) {
        for (int c = threadIdx.x; c < QT * words; c += 256) sQ[c] = c < tnq * words ? queries[(int64_t)q0 * words + c] : 0ull;
        __syncthreads();
    } else {
#pragma unroll
        for (int i = 0; i < QT; ++i) {
            const uint64_t* q = queries + (int64_t)(q0 + i) * words;
            qa[i] = i < tnq && 2 * j < words ? q[2 * j] : 0ull;
            qb[i] = i < tnq && 2 * j + 1 < words ? q[2 * j + 1] : 0ull;
        }
    }

    WaveTopK top[QT];
#pragma unroll
    for (int i = 0; i < QT; ++i) top[i].init();

    // The slot of `row` if the row is a candidate (live, in the mask, with a code of `words` words), else INT64_MIN.
    auto candidate_slot = [&](int64_t row) -> int64_t {
        if (row >= total) return INT64_MIN;
        const float n = rn[row];
        if (n != n || (mask && mask[row] == 0)) return INT64_MIN;
        const int64_t slot = slots[row];
        return (slot & 0xff) == words ? slot : INT64_MIN;  // (INT64_MIN itself has length 0, and words >= 1)
    };
    // words w and w + 1 of a candidate's code (0 where the code ends, or without a candidate)
    auto load_pair = [&](bool have, const uint64_t* src, int w, uint64_t& xa, uint64_t& xb) {
        xa = xb = 0ull;
        if (have && w + 1 < words) {
            const WordPair p = *reinterpret_cast<const WordPair*>(src + w);
            xa = p.a;
            xb = p.b;
        } else if (have && w < words) {
            xa = src[w];
        }
    };
    auto count = [](uint64_t x, uint64_t q) -> int32_t { return __popcll(x & q); };

    // r0 is uniform over the block: every lane of a wave runs the same iterations (the lists' shuffles need all of them).
    // The next step's slot is loaded before this step's words.
    constexpr int64_t step = 4 * RW;
    const int64_t stride = (int64_t)gridDim.x * step;
    int64_t slot_next = candidate_slot((int64_t)blockIdx.x * step + wave * RW + g);
    for (int64_t r0 = (int64_t)blockIdx.x * step; r0 < total; r0 += stride) {
        const int64_t row = r0 + wave * RW + g;
        const int64_t slot = slot_next;
        slot_next = r0 + stride < total ? candidate_slot(row + stride) : INT64_MIN;
        const bool have = slot != INT64_MIN;
        const uint64_t* src = reinterpret_cast<const uint64_t*>(pool) + (slot >> 8);  // (never read without a candidate)
        int32_t acc[QT];
#pragma unroll
        for (int i = 0; i < QT; ++i) acc[i] = 0;
        int32_t px = 0;  // the popcount of the row's code
        if constexpr (LDSQ) {
            for (int c = 0; c < words; c += 32) {
                const int w = c + 2 * j;
                uint64_t xa, xb;
                load_pair(have, src, w, xa, xb);
                px += __popcll(xa) + __popcll(xb);
#pragma unroll
                for (int i = 0; i < QT; ++i) {
                    const uint64_t a = w < words ? sQ[i * words + w] : 0ull;
                    const uint64_t b = w + 1 < words ? sQ[i * words + w + 1] : 0ull;
                    acc[i] += count(xa, a) + count(xb, b);
                }
            }
        } else {
            uint64_t xa, xb;
            load_pair(have, src, 2 * j, xa, xb);
            px = __popcll(xa) + __popcll(xb);
#pragma unroll
            for (int i = 0; i < QT; ++i) acc[i] = count(xa, qa[i]) + count(xb, qb[i]);
        }
#pragma unroll
        for (int m = 1; m < L; m <<= 1) px += __shfl_xor(px, m);
#pragma unroll
        for (int i = 0; i < QT; ++i) {
            if (i < tnq) {  // (uniform)
                int32_t c = acc[i];
#pragma unroll
                for (int m = 1; m < L; m <<= 1) c += __shfl_xor(c, m);
                const int32_t u = qpop[q0 + i] + px - c;  // popcount(q | x)
                double d = (double)(u - c);               // popcount(q ^ x)
                if (metric == MLVDB_BITS_JACCARD) d = u == 0 ? 0.0 : d / (double)u;  // (uniform)
                top[i].offer(have && j == 0, d, (int32_t)row, k, lane);
            }
        }
    }

    // the block's four lists of each query -> partial[((q0 + i) * gridDim.x + block) * k ..], the input of exact_merge_kernel
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        if (i < tnq) {  // (uniform over the block: the barriers inside are met by all of it or by none)
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
                    partial[((int64_t)(q0 + i) * gridDim.x + blockIdx.x) * k + lane] = e;
                }
            }
            __syncthreads();
        }
    }
}

int bits_lanes(int32_t words) {
    int l = 1;
    while (l < 16 && 2 * l < words) l *= 2;
    return l;
}

int32_t bits_scan_blocks(int64_t total, int64_t nq, int32_t k, int32_t words) {
    // kBitsMaxBlocks blocks over all tiles of the pass -- what the card holds at once at two waves per SIMD -- and one block
    // per 256 / L rows at the most.  A wave's list costs its k (ln(rows / k) + 1) insertions whatever the grid is, so every
    // further wave per query adds that much serial work and shortens nothing but the cheap walk: 1,024 blocks per tile were
    // measured at 9.8 ms per 256 queries over 1M 256-bit codes.  The 64 MiB bound of the partial entries stays
    // as the last word; at k <= 64 the first bound keeps them below 8 MiB.
    const int64_t ntiles = (std::max<int64_t>(nq, 1) + kBitsQT - 1) / kBitsQT;
    const int64_t by_tiles = std::max<int64_t>(1, kBitsMaxBlocks / ntiles);
    const int64_t by_mem = (int64_t)(64u << 20) / (std::max<int64_t>(nq, 1) * k * (int64_t)sizeof(TopEntry));
    const int64_t rows = 256 / bits_lanes(words);
    const int64_t by_rows = (total + rows - 1) / rows;
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>({by_tiles, by_mem, by_rows}));
}

hipError_t launch_bits_scan(const int64_t* slots, const int64_t* pool, const float* rn, const uint8_t* mask, int64_t total,
                            const uint64_t* queries, const int32_t* qpop, int32_t nq, int32_t words, int32_t metric, int32_t k,
                            int32_t nblk, TopEntry* partial, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    const int32_t ntiles = (nq + kBitsQT - 1) / kBitsQT;
    if (k < 1 || k > kWave || nblk < 1 || ntiles > 65535 || total <= 0 || total > INT32_MAX || words < 1 ||
        words > MLVDB_BITS_MAX_WORDS || (metric != MLVDB_BITS_HAMMING && metric != MLVDB_BITS_JACCARD))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nblk, (unsigned)ntiles);
    const size_t lds = words > 32 ? (size_t)kBitsQT * words * sizeof(uint64_t) : 0;
#define MLVDB_BITS_LAUNCH(L, LDSQ) \
    bits_scan_kernel<L, LDSQ><<<grid, 256, lds, s>>>(slots, pool, rn, mask, total, queries, qpop, nq, words, metric, k, partial)
    if (words > 32) MLVDB_BITS_LAUNCH(16, true);
    else switch (bits_lanes(words)) {
        case 1: MLVDB_BITS_LAUNCH(1, false); break;
        case 2: MLVDB_BITS_LAUNCH(2, false); break;
        case 4: MLVDB_BITS_LAUNCH(4, false); break;
        case 8: MLVDB_BITS_LAUNCH(8, false); break;
        default: MLVDB_BITS_LAUNCH(16, false); break;
    }
#undef MLVDB_BITS_LAUNCH
    return hipGetLastError();
}

}  // namespace mlvdb
