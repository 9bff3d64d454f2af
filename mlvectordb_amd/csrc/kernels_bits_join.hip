// Similarity join over a binary vector column (include/mlvdb_bits_join.h): the rows within a Hamming or Jaccard radius of
// thousands to millions of stored rows -- a popcount "GEMM", not the streaming walk of kernels_bits_range.hip.  DESIGN.md 11.23.
//
// bits_join_gather_kernel copies a wave of left codes through the slot column into a dense [rows][words] buffer with their
// popcounts (-1: the label holds no code of this width or is dead), the `queries` / `qpop` shape bits_range_sort_kernel
// takes; run over all rows with a mask and without a buffer it gives the popcount of every candidate row (-1: none).
// bits_join_kernel walks tiles of 128 left x 128 right rows with 256 threads: thread (ty, tx) = (t / 16, t % 16) owns the
// pairs (ty + 16 i, tx + 16 j), i, j < 8 -- 64 integer accumulators.  Both sides are staged in chunks of KC = 8 words into
// LDS rows of KC + 1 words, double-buffered: chunk c + 1 is in flight from HBM while chunk c is XORed and counted, one
// barrier per chunk.  The accumulators hold Hamming distances; Jaccard's integers follow from them and the two popcounts.
// After each chunk but the last a pair whose partial sum exceeds the tile's bound B (hit => ham <= B) is dead, and a tile
// without a live pair drops its remaining chunks: the waves' ballots meet in LDS and are read behind the next barrier.
// The bound only prunes: the final test of a pair is bits_range_kernel's own.
//   FILL = false  counts: a thread's hits of a left row -> one LDS atomic -> one global atomicAdd per (tile, left row) with
//                 a non-zero sum.
//   FILL = true   collects: a hit takes a position from the left row's cursor and writes the key of bits_range_key.h.
// bits_join_plan_kernel is the exclusive scan of a wave's segment lengths (0 above `capacity`) by one workgroup.
#include "bits_range_key.h"
#include "internal.h"

namespace mlvdb {

namespace {
constexpr int T = kBitsJoinTile;
constexpr int KC = kBitsJoinKC;
constexpr int LD = KC + 1;  // LDS row stride in words: 18 dwords, so 16 consecutive rows start in 16 different bank pairs
constexpr int kGatherLanes = 8;
static_assert(T == 128 && KC == 8, "256 threads stage 128 rows x 8 words in four steps and own 8 x 8 pairs each");

// acc + popcount(x) in the one instruction that has the addend: left to itself the compiler counts both halves of a word
// against zero and joins them with a three-operand add, five VALU operations per 64-bit word and pair instead of four
__device__ __forceinline__ int32_t popc_add(uint32_t x, int32_t acc) {
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(x));
    return acc;
}
}  // namespace

__global__ __launch_bounds__(256) void bits_join_gather_kernel(const int64_t* __restrict__ slots, const int64_t* __restrict__ pool,
                                                               const float* __restrict__ rn, const uint8_t* __restrict__ mask,
                                                               const int64_t* __restrict__ labels, int64_t n, int32_t words,
                                                               uint64_t* __restrict__ dense, int32_t* __restrict__ pop) {
    const int j = threadIdx.x % kGatherLanes;
    const int64_t i = (int64_t)blockIdx.x * (256 / kGatherLanes) + threadIdx.x / kGatherLanes;
    const bool in = i < n;
    int64_t slot = INT64_MIN;
    if (in) {
        const int64_t row = labels ? labels[i] : i;
        const float nn = rn[row];
        if (nn == nn && (!mask || mask[row] != 0)) {
            const int64_t sl = slots[row];
            if ((sl & 0xff) == words) slot = sl;  // (an absent row's INT64_MIN has length 0, and words >= 1)
        }
    }
    const bool have = slot != INT64_MIN;
    const uint64_t* src = reinterpret_cast<const uint64_t*>(pool) + (have ? slot >> 8 : 0);
    int32_t p = 0;
    for (int w = j; w < words; w += kGatherLanes) {
        const uint64_t v = have ? src[w] : 0ull;
        p += __popcll(v);
        if (dense && in) dense[i * words + w] = v;
    }
#pragma unroll
    for (int m = 1; m < kGatherLanes; m <<= 1) p += __shfl_xor(p, m);  // (every lane of the wave is here)
    if (in && j == 0) pop[i] = have ? p : -1;
}

template <bool JACCARD, bool FILL>
__global__ __launch_bounds__(256) void bits_join_kernel(const int64_t* __restrict__ slots, const int64_t* __restrict__ pool,
                                                        const int32_t* __restrict__ rpop, int64_t total,
                                                        const int64_t* __restrict__ labels, const uint64_t* __restrict__ lq,
                                                        const int32_t* __restrict__ lpop, int32_t n,
                                                        const int64_t* __restrict__ tile_begin, int64_t items, int32_t words,
                                                        int32_t mode, int32_t ham_max, double radius, double radius_up,
                                                        int32_t* __restrict__ cnt, const int64_t* __restrict__ off,
                                                        int32_t* __restrict__ cursor, uint64_t* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) uint64_t sL[2][T * LD];
    __shared__ __attribute__((aligned(16))) uint64_t sR[2][T * LD];
    __shared__ int64_t sRoff[T];                       // a right row's first word in the pool, -1: no candidate
    __shared__ int32_t sRp[T], sLp[T], sLab[T], sCnt[T];  // popcounts (-1: none), left labels, FILL = false: the tile's counts
    __shared__ int32_t sMax[4], sAlive[2][4];
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int ty = t >> 4, tx = t & 15;
    const int srow = t >> 3, sw = t & 7;  // staging: rows srow + 32 k, word sw of the chunk
    const int32_t nlt = (n + T - 1) / T;
    const int64_t nrt = (total + T - 1) / T;
    const int nch = (words + KC - 1) / KC;
    const uint64_t* pool64 = reinterpret_cast<const uint64_t*>(pool);

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {  // (uniform over the block)
        int32_t lt = 0, hi = nlt;  // the left tile of the item: the last one that begins at or before it
        while (hi - lt > 1) {
            const int32_t mid = (lt + hi) >> 1;
            if (tile_begin[mid] <= item) lt = mid;
            else hi = mid;
        }
        const int64_t rt = nrt - (tile_begin[lt + 1] - tile_begin[lt]) + (item - tile_begin[lt]);
        const int32_t l0 = lt * T;
        const int64_t r0 = rt * T;

        // the tile's rows: candidates are marked once, here
        int32_t m;
        if (t < T) {
            const int64_t row = r0 + t;
            m = row < total ? rpop[row] : -1;
            sRp[t] = m;
            sRoff[t] = m >= 0 ? slots[row] >> 8 : -1;
        } else {
            const int32_t li = l0 + t - T;
            m = li < n ? lpop[li] : -1;
            sLp[t - T] = m;
            sLab[t - T] = li < n ? (int32_t)labels[li] : -1;
            if constexpr (!FILL) sCnt[t - T] = 0;  // (the thread that sent the last tile's sum away, below)
        }
        if constexpr (JACCARD) {
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) m = max(m, __shfl_xor(m, s));
            if (lane == 0) sMax[wave] = m;  // waves 0, 1: the right rows, waves 2, 3: the left rows
        }
        __syncthreads();
        int32_t bound = ham_max;
        if constexpr (JACCARD) {
            // hit => ham <= u * radius_up (the walk's first test) and u <= pa + pb <= the tile's two maxima
            const double x = (double)(max(sMax[0], sMax[1]) + max(sMax[2], sMax[3])) * radius_up;
            bound = !(x == x) || x >= 2147483647.0 ? INT32_MAX : x < 0 ? -1 : (int32_t)x;
        }
        const bool prune = bound != INT32_MAX && nch > 1;

        int32_t acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0;
        uint64_t vl[4], vr[4];
        auto load = [&](int c0) {
            const int w = c0 + sw;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = srow + 32 * k;
                const int64_t ro = sRoff[row];
                vr[k] = ro >= 0 && w < words ? pool64[ro + w] : 0ull;
                const int32_t li = l0 + row;
                vl[k] = li < n && w < words ? lq[(int64_t)li * words + w] : 0ull;
            }
        };
        auto store = [&](int b) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sL[b][(srow + 32 * k) * LD + sw] = vl[k];
                sR[b][(srow + 32 * k) * LD + sw] = vr[k];
            }
        };
        load(0);
        store(0);
        bool dropped = false;
        for (int c = 0; c < nch; ++c) {
            const bool more = c + 1 < nch;
            if (more) load((c + 1) * KC);  // in flight during this chunk's arithmetic
            __syncthreads();               // chunk c is in LDS, and nobody reads the other buffer any more
            if (prune && c > 0 && !(sAlive[(c - 1) & 1][0] | sAlive[(c - 1) & 1][1] | sAlive[(c - 1) & 1][2] | sAlive[(c - 1) & 1][3])) {
                dropped = true;  // (the same four words for every thread)
                break;
            }
            const uint64_t* pl = &sL[c & 1][ty * LD];
            const uint64_t* pr = &sR[c & 1][tx * LD];
            const int len = min(KC, words - c * KC);
            for (int w = 0; w < len; ++w) {
                uint64_t a[8], b[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    a[i] = pl[i * 16 * LD + w];
                    b[i] = pr[i * 16 * LD + w];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const uint64_t x = a[i] ^ b[j];
                        acc[i][j] = popc_add((uint32_t)x, acc[i][j]);
                        acc[i][j] = popc_add((uint32_t)(x >> 32), acc[i][j]);
                    }
            }
            if (more) {
                if (prune) {
                    bool alive = false;
#pragma unroll
                    for (int i = 0; i < 8; ++i)
#pragma unroll
                        for (int j = 0; j < 8; ++j) alive |= acc[i][j] <= bound;
                    const bool any = __ballot(alive) != 0;
                    if (lane == 0) sAlive[c & 1][wave] = any;
                }
                store((c + 1) & 1);
            }
        }

        // a wave none of whose pairs is within the bound has no hit to test (hit => ham <= bound): most waves of most tiles
        bool live = false;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) live |= acc[i][j] <= bound;
        if (!dropped && __ballot(live) != 0) {
            int32_t rp[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) rp[j] = sRp[tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int li = ty + 16 * i;
                const int32_t pa = sLp[li];
                const int32_t lab = sLab[li];
                int32_t nh = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int64_t row = r0 + tx + 16 * j;
                    const int32_t ham = acc[i][j];
                    bool hit = pa >= 0 && rp[j] >= 0 && (mode == MLVDB_JOIN_LATER ? row > lab : row != lab);
                    double d = (double)ham;
                    if constexpr (JACCARD) {
                        const int32_t u = (pa + rp[j] + ham) >> 1;  // popcount(a | b): pa + pb = u + i and ham = u - i
                        // bits_range_kernel's test: the multiply drops no hit, the one division decides
                        hit = hit && !((double)ham > (double)u * radius_up);
                        if (hit) {
                            d = u == 0 ? 0.0 : d / (double)u;
                            hit = d <= radius;
                        }
                    } else {
                        hit = hit && ham <= ham_max;
                    }
                    if (hit) {
                        if constexpr (!FILL) {
                            ++nh;
                        } else {
                            const int64_t lo = off[l0 + li];  // (pa >= 0: the left row exists)
                            const int32_t len = (int32_t)(off[l0 + li + 1] - lo);  // 0: the row is over capacity
                            if (len > 0) {
                                const int32_t pos = atomicAdd(&cursor[l0 + li], 1);
                                if (pos < len) keys[lo + pos] = range_key(JACCARD ? MLVDB_BITS_JACCARD : MLVDB_BITS_HAMMING, ham, d, row);
                            }
                        }
                    }
                }
                if constexpr (!FILL)
                    if (nh) atomicAdd(&sCnt[li], nh);
            }
        }
        __syncthreads();  // the tile is done: its rows, buffers and counters may be overwritten
        if constexpr (!FILL) {
            if (t >= T) {  // (the thread that clears the counter for the next tile)
                const int32_t s = sCnt[t - T];
                if (s != 0) atomicAdd(&cnt[l0 + t - T], s);
            }
        }
    }
}

// One workgroup: thread t scans the rows [t * per, (t + 1) * per) of the wave.  len[i] = cnt[i] if it is <= capacity, else
// 0; off[0 .. n] = the exclusive scan of len; *over = some row is over capacity.
__global__ __launch_bounds__(1024) void bits_join_plan_kernel(const int32_t* __restrict__ cnt, int32_t n, int32_t capacity,
                                                              int64_t* __restrict__ off, int32_t* __restrict__ over) {
    __shared__ int64_t s[1024];
    __shared__ int32_t any_over;
    const int t = threadIdx.x;
    const int32_t per = (n + 1023) / 1024;
    const int32_t lo = min(n, t * per), hi = min(n, lo + per);
    if (t == 0) any_over = 0;
    __syncthreads();
    int64_t sum = 0;
    for (int32_t i = lo; i < hi; ++i) {
        const int32_t c = cnt[i];
        if (c <= capacity) sum += c;
        else any_over = 1;  // (every writer writes 1)
    }
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // inclusive scan
        const int64_t v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    int64_t run = s[t] - sum;
    for (int32_t i = lo; i < hi; ++i) {
        const int32_t c = cnt[i];
        off[i] = run;
        run += c <= capacity ? c : 0;
    }
    if (t == 1023) off[n] = s[t];
    if (t == 0) *over = any_over;
}

int64_t bits_join_wave_rows(int32_t words, int32_t budget_mb) {
    const int64_t fit = ((int64_t)std::max(budget_mb, 1) << 20) / ((int64_t)words * (int64_t)sizeof(uint64_t));
    return std::min<int64_t>(std::max<int64_t>(fit / T * T, T), kBitsSortMaxSegments);
}

int32_t bits_join_blocks(int64_t items, int32_t cus) {
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(items, (int64_t)std::max(cus, 1) * kBitsJoinBlocksPerCU));
}

hipError_t launch_bits_join_gather(const int64_t* slots, const int64_t* pool, const float* rn, const uint8_t* mask,
                                   const int64_t* labels, int64_t n, int32_t words, uint64_t* dense, int32_t* pop, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    constexpr int64_t rows = 256 / kGatherLanes;
    if (n > INT32_MAX || words < 1 || words > MLVDB_BITS_MAX_WORDS || !pop) return hipErrorInvalidValue;
    bits_join_gather_kernel<<<(unsigned)((n + rows - 1) / rows), 256, 0, s>>>(slots, pool, rn, mask, labels, n, words, dense, pop);
    return hipGetLastError();
}

hipError_t launch_bits_join_walk(bool fill, const int64_t* slots, const int64_t* pool, const int32_t* rpop, int64_t total,
                                 const int64_t* labels, const uint64_t* lq, const int32_t* lpop, int32_t n,
                                 const int64_t* tile_begin, int64_t items, int32_t words, int32_t metric, int32_t mode,
                                 double radius, int32_t nblk, int32_t* cnt, const int64_t* off, int32_t* cursor,
                                 uint64_t* keys, hipStream_t s) {
    if (n <= 0 || items <= 0) return hipSuccess;
    if (nblk < 1 || total <= 0 || total > INT32_MAX || n > kBitsSortMaxSegments || words < 1 || words > MLVDB_BITS_MAX_WORDS ||
        radius != radius || (metric != MLVDB_BITS_HAMMING && metric != MLVDB_BITS_JACCARD) ||
        (mode != MLVDB_JOIN_OTHERS && mode != MLVDB_JOIN_LATER) || (fill ? !off || !cursor || !keys : !cnt))
        return hipErrorInvalidValue;
    // the two constants of launch_bits_range_walk: d <= radius on integers, and the multiplier of Jaccard's first test
    const int32_t ham_max = radius < 0 ? -1 : radius >= 64.0 * MLVDB_BITS_MAX_WORDS ? 64 * MLVDB_BITS_MAX_WORDS : (int32_t)radius;
    const double radius_up = radius * 1.0000001;
#define MLVDB_BITS_JOIN_LAUNCH(JACCARD, FILL)                                                                              \
    bits_join_kernel<JACCARD, FILL><<<(unsigned)nblk, 256, 0, s>>>(slots, pool, rpop, total, labels, lq, lpop, n, tile_begin, \
                                                                   items, words, mode, ham_max, radius, radius_up, cnt, off, \
                                                                   cursor, keys)
    if (metric == MLVDB_BITS_JACCARD) {
        if (fill) MLVDB_BITS_JOIN_LAUNCH(true, true);
        else MLVDB_BITS_JOIN_LAUNCH(true, false);
    } else {
        if (fill) MLVDB_BITS_JOIN_LAUNCH(false, true);
        else MLVDB_BITS_JOIN_LAUNCH(false, false);
    }
#undef MLVDB_BITS_JOIN_LAUNCH
    return hipGetLastError();
}

hipError_t launch_bits_join_plan(const int32_t* cnt, int32_t n, int32_t capacity, int64_t* off, int32_t* over, hipStream_t s) {
    if (n < 1 || n > kBitsSortMaxSegments || capacity < 1 || capacity > MLVDB_BITS_RANGE_MAX_HITS) return hipErrorInvalidValue;
    bits_join_plan_kernel<<<1, 1024, 0, s>>>(cnt, n, capacity, off, over);
    return hipGetLastError();
}

}  // namespace mlvdb
