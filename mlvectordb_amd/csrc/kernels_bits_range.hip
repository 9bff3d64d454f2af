// Range search over a binary vector column (include/mlvdb_bits_range.h): every candidate row within a Hamming or Jaccard
// radius of each query of a pass, counted exactly, then collected and sorted.  DESIGN.md 11.22.
//
// bits_range_kernel is a streaming walk with the candidate rule, the loads and the three integers (pq, px, i) of
// bits_scan_kernel (kernels_bits.hip) and none of its lists: a hit is a test against one scalar.  A tile is kBitsRangeQT = 32
// consecutive queries (the registers the sixteen WaveTopK held now hold query words), blockIdx.y is the tile, blockIdx.x
// strides over groups of 256 / L rows.  The test is an integer compare for Hamming; for Jaccard one fp64 multiply rules out
// what cannot be a hit and the division -- the one the reported distance is -- decides the few rows that are left.
//   FILL = false  counts: a wave's hits of a query are the popcount of its ballot, summed in a wave-uniform register; the
//                 block's four sums meet in LDS and leave as one integer atomicAdd per (block, query) with a non-zero sum.
//   FILL = true   collects: lane 0 of a hit's group takes a position from the query's cursor and writes the 64-bit key
//                 (distance << 32 | row) into the query's segment, for the queries whose segment is not empty.
// bits_range_plan_kernel turns a pass's counts into segment lengths (0 above `capacity`), their exclusive scan and the
// over-capacity flag.  bits_range_sort_kernel is one workgroup per non-empty segment: keys into LDS, bitonic sort, labels
// out, and every hit's distance computed again from the row's code and the query -- the key orders, it reports nothing.
#include "bits_range_key.h"
#include "internal.h"

namespace mlvdb {

namespace {
// two adjacent words of a code: a code starts wherever the pool's append left it, so 8-byte alignment is all there is
struct __attribute__((packed, aligned(8))) WordPair {
    uint64_t a, b;
};

// words w and w + 1 of a candidate's code (0 where the code ends, or without a candidate)
__device__ __forceinline__ void load_pair(bool have, const uint64_t* src, int w, int words, uint64_t& xa, uint64_t& xb) {
    xa = xb = 0ull;
    if (have && w + 1 < words) {
        const WordPair p = *reinterpret_cast<const WordPair*>(src + w);
        xa = p.a;
        xb = p.b;
    } else if (have && w < words) {
        xa = src[w];
    }
}
}  // namespace

template <int L, bool LDSQ, bool FILL>
__global__ __launch_bounds__(256) void bits_range_kernel(const int64_t* __restrict__ slots, const int64_t* __restrict__ pool,
                                                         const float* __restrict__ rn, const uint8_t* __restrict__ mask,
                                                         int64_t total, const uint64_t* __restrict__ queries,
                                                         const int32_t* __restrict__ qpop, int32_t nq, int32_t words,
                                                         int32_t metric, int32_t ham_max, double radius, double radius_up,
                                                         int32_t* __restrict__ cnt, const int64_t* __restrict__ off,
                                                         int32_t* __restrict__ cursor, uint64_t* __restrict__ keys) {
    constexpr int QT = kBitsRangeQT;
    constexpr int RW = 64 / L;  // rows per wave step
    static_assert(L == 1 || L == 2 || L == 4 || L == 8 || L == 16, "a group is a power of two of lanes inside a row of 16");
    extern __shared__ __attribute__((aligned(16))) uint64_t sQ[];  // LDSQ: [QT][words]
    __shared__ int32_t sc[4][QT];
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
    int32_t hits[QT];  // FILL = false: this wave's hits of each query (wave-uniform)
#pragma unroll
    for (int i = 0; i < QT; ++i) hits[i] = 0;

    // The slot of `row` if the row is a candidate (live, in the mask, with a code of `words` words), else INT64_MIN.
    auto candidate_slot = [&](int64_t row) -> int64_t {
        if (row >= total) return INT64_MIN;
        const float n = rn[row];
        if (n != n || (mask && mask[row] == 0)) return INT64_MIN;
        const int64_t slot = slots[row];
        return (slot & 0xff) == words ? slot : INT64_MIN;  // (INT64_MIN itself has length 0, and words >= 1)
    };
    // Query i of the tile against the row of this lane's group: c = popcount(q & x) summed over the group.
    auto test = [&](int i, int32_t c, int32_t px, bool lead, int64_t row) {
        const int32_t u = qpop[q0 + i] + px - c;  // popcount(q | x)
        const int32_t ham = u - c;                // popcount(q ^ x)
        double d = (double)ham;
        bool hit = lead;
        if (metric == MLVDB_BITS_JACCARD) {  // (uniform)
            // fl(ham / u) <= radius implies ham <= u * radius * (1 + 2^-52) < fl(u * radius_up): the multiply drops no hit
            // (written as a negation: u == 0 with an infinite radius gives a NaN product, and d = 0.0 is a hit then)
            hit = hit && !((double)ham > (double)u * radius_up);
            if (hit) {
                d = u == 0 ? 0.0 : d / (double)u;
                hit = d <= radius;
            }
        } else {
            hit = hit && ham <= ham_max;  // ham_max = floor(radius), -1 for a negative one: the same test on integers
        }
        if constexpr (!FILL) {
            hits[i] += __popcll(__ballot(hit));
        } else if (hit) {
            const int64_t lo = off[q0 + i];
            const int32_t len = (int32_t)(off[q0 + i + 1] - lo);  // 0: the query is over capacity (or has no hit)
            if (len > 0) {
                const int32_t pos = atomicAdd(&cursor[q0 + i], 1);
                if (pos < len) keys[lo + pos] = range_key(metric, ham, d, row);  // (the counts are exact: never false)
            }
        }
    };

    // r0 is uniform over the block: every lane of a wave runs the same iterations (the shuffles and ballots need all of
    // them).  The next step's slot is loaded before this step's words.
    constexpr int64_t step = 4 * RW;
    const int64_t stride = (int64_t)gridDim.x * step;
    int64_t slot_next = candidate_slot((int64_t)blockIdx.x * step + wave * RW + g);
    for (int64_t r0 = (int64_t)blockIdx.x * step; r0 < total; r0 += stride) {
        const int64_t row = r0 + wave * RW + g;
        const int64_t slot = slot_next;
        slot_next = r0 + stride < total ? candidate_slot(row + stride) : INT64_MIN;
        const bool have = slot != INT64_MIN;
        const bool lead = have && j == 0;
        const uint64_t* src = reinterpret_cast<const uint64_t*>(pool) + (slot >> 8);  // (never read without a candidate)
        int32_t px = 0;  // the popcount of the row's code
        if constexpr (LDSQ) {
            int32_t acc[QT];
#pragma unroll
            for (int i = 0; i < QT; ++i) acc[i] = 0;
            for (int c = 0; c < words; c += 32) {
                const int w = c + 2 * j;
                uint64_t xa, xb;
                load_pair(have, src, w, words, xa, xb);
                px += __popcll(xa) + __popcll(xb);
#pragma unroll
                for (int i = 0; i < QT; ++i) {
                    const uint64_t a = w < words ? sQ[i * words + w] : 0ull;
                    const uint64_t b = w + 1 < words ? sQ[i * words + w + 1] : 0ull;
                    acc[i] += __popcll(xa & a) + __popcll(xb & b);
                }
            }
#pragma unroll
            for (int m = 1; m < L; m <<= 1) px += __shfl_xor(px, m);
#pragma unroll
            for (int i = 0; i < QT; ++i) {
                if (i < tnq) {  // (uniform)
                    int32_t c = acc[i];
#pragma unroll
                    for (int m = 1; m < L; m <<= 1) c += __shfl_xor(c, m);
                    test(i, c, px, lead, row);
                }
            }
        } else {
            uint64_t xa, xb;
            load_pair(have, src, 2 * j, words, xa, xb);
            px = __popcll(xa) + __popcll(xb);
#pragma unroll
            for (int m = 1; m < L; m <<= 1) px += __shfl_xor(px, m);
#pragma unroll
            for (int i = 0; i < QT; ++i) {
                if (i < tnq) {  // (uniform)
                    int32_t c = __popcll(xa & qa[i]) + __popcll(xb & qb[i]);
#pragma unroll
                    for (int m = 1; m < L; m <<= 1) c += __shfl_xor(c, m);
                    test(i, c, px, lead, row);
                }
            }
        }
    }

    if constexpr (!FILL) {
        // the four waves' sums of each query -> one atomicAdd per (block, query) with a hit; integer addition commutes
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < QT; ++i) sc[wave][i] = hits[i];
        }
        __syncthreads();
        if (threadIdx.x < tnq) {
            const int32_t s = sc[0][threadIdx.x] + sc[1][threadIdx.x] + sc[2][threadIdx.x] + sc[3][threadIdx.x];
            if (s) atomicAdd(&cnt[q0 + threadIdx.x], s);
        }
    }
}

// One block per pass of n <= kBitsChunk queries: len[q] = cnt[q] if it is <= capacity, else 0; off[0 .. n] = the exclusive
// scan of len (off[n] = the entries the pass needs, at most 256 x 16,384); *over = some query is over capacity.
__global__ __launch_bounds__(kBitsChunk) void bits_range_plan_kernel(const int32_t* __restrict__ cnt, int32_t n, int32_t capacity,
                                                                     int64_t* __restrict__ off, int32_t* __restrict__ over) {
    __shared__ int32_t s[kBitsChunk];
    __shared__ int32_t any_over;
    const int t = threadIdx.x;
    if (t == 0) any_over = 0;
    __syncthreads();
    const int32_t c = t < n ? cnt[t] : 0;
    const int32_t len = c <= capacity ? c : 0;
    if (c > capacity) any_over = 1;  // (every writer writes 1)
    s[t] = len;
    __syncthreads();
    for (int d = 1; d < kBitsChunk; d <<= 1) {  // inclusive scan
        const int32_t v = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    if (t < n) off[t] = (int64_t)(s[t] - len);
    if (t == n - 1) off[n] = (int64_t)s[t];
    if (t == 0) *over = any_over;
}

// One workgroup per query of the pass; a query with an empty segment returns at once.  `lanes` = the L of the walk: L lanes
// per hit compute its distance again, lane j from the words 2j and 2j + 1 (+ 32, 64, ...) of the row's code and the query.
__global__ __launch_bounds__(1024) void bits_range_sort_kernel(const int64_t* __restrict__ slots, const int64_t* __restrict__ pool,
                                                               const uint64_t* __restrict__ queries,
                                                               const int32_t* __restrict__ qpop, int32_t words, int32_t metric,
                                                               int32_t lanes, const int64_t* __restrict__ off,
                                                               const uint64_t* __restrict__ keys, int64_t* __restrict__ out_lab,
                                                               float* __restrict__ out_dist, double* __restrict__ out_d64) {
    extern __shared__ __attribute__((aligned(16))) uint64_t sk[];  // the segment, padded to a power of two
    const int q = blockIdx.x;
    const int64_t lo = off[q];
    const int32_t len = (int32_t)(off[q + 1] - lo);
    if (len <= 0) return;  // (uniform over the block)
    int32_t np = 1;
    while (np < len) np <<= 1;
    const int t = threadIdx.x, nt = blockDim.x;
    for (int e = t; e < np; e += nt) sk[e] = e < len ? keys[lo + e] : UINT64_MAX;
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int e = t; e < np; e += nt) {
                const int p = e ^ jj;
                if (p > e) {
                    const uint64_t a = sk[e], b = sk[p];
                    if ((a > b) == ((e & k) == 0)) {
                        sk[e] = b;
                        sk[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // every hit's distance from the same integers and the same division as the walk's: the same 64 bits
    const uint64_t* qw = queries + (int64_t)q * words;
    const int32_t pq = qpop[q];
    const int j = t % lanes;
    const int per = nt / lanes;  // hits per round (lanes <= 16 divides the block and the wave)
    for (int e0 = 0; e0 < len; e0 += per) {  // (uniform: the shuffles below need every lane of the wave)
        const int e = e0 + t / lanes;
        const bool have = e < len;
        const int64_t row = have ? (int64_t)(sk[e] & 0xffffffffull) : 0;
        const uint64_t* src = reinterpret_cast<const uint64_t*>(pool) + (have ? slots[row] >> 8 : 0);
        int32_t px = 0, c = 0;
        for (int w0 = 0; w0 < words; w0 += 32) {
            const int w = w0 + 2 * j;
            uint64_t xa, xb;
            load_pair(have, src, w, words, xa, xb);
            px += __popcll(xa) + __popcll(xb);
            const uint64_t a = w < words ? qw[w] : 0ull;
            const uint64_t b = w + 1 < words ? qw[w + 1] : 0ull;
            c += __popcll(xa & a) + __popcll(xb & b);
        }
        for (int m = 1; m < lanes; m <<= 1) {
            px += __shfl_xor(px, m);
            c += __shfl_xor(c, m);
        }
        if (have && j == 0) {
            const int32_t u = pq + px - c;
            double d = (double)(u - c);
            if (metric == MLVDB_BITS_JACCARD) d = u == 0 ? 0.0 : d / (double)u;
            out_lab[lo + e] = row;
            out_dist[lo + e] = (float)d;
            out_d64[lo + e] = d;
        }
    }
}

int32_t bits_range_blocks(int64_t total, int64_t nq, int32_t words, int32_t cus) {
    // One resident set of blocks over all tiles of the pass -- per compute unit what the resource table lets
    // the instantiation keep: 7 blocks of the one-lane-per-row walk (39 VGPRs), kBitsRangeBlocksPerCU of every other (161 to
    // 188) -- and one block per 256 / L rows at the most: nothing is warmed per block here, so a block costs its launch and
    // 32 atomics at the most.
    const int64_t ntiles = (std::max<int64_t>(nq, 1) + kBitsRangeQT - 1) / kBitsRangeQT;
    const int64_t per_cu = words <= 2 ? 7 : kBitsRangeBlocksPerCU;
    const int64_t resident = std::max<int64_t>(1, (int64_t)std::max(cus, 1) * per_cu / ntiles);
    const int64_t rows = 256 / bits_lanes(words);
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(resident, (total + rows - 1) / rows));
}

hipError_t launch_bits_range_walk(bool fill, const int64_t* slots, const int64_t* pool, const float* rn, const uint8_t* mask,
                                  int64_t total, const uint64_t* queries, const int32_t* qpop, int32_t nq, int32_t words,
                                  int32_t metric, double radius, int32_t nblk, int32_t* cnt, const int64_t* off, int32_t* cursor,
                                  uint64_t* keys, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    const int32_t ntiles = (nq + kBitsRangeQT - 1) / kBitsRangeQT;
    if (nblk < 1 || ntiles > 65535 || total <= 0 || total > INT32_MAX || words < 1 || words > MLVDB_BITS_MAX_WORDS ||
        radius != radius || (metric != MLVDB_BITS_HAMMING && metric != MLVDB_BITS_JACCARD))
        return hipErrorInvalidValue;
    // Hamming: d <= radius on integers (no distance exceeds 64 x 255 bits); Jaccard: the multiplier of the first test
    const int32_t ham_max = radius < 0 ? -1 : radius >= 64.0 * MLVDB_BITS_MAX_WORDS ? 64 * MLVDB_BITS_MAX_WORDS : (int32_t)radius;
    const double radius_up = radius * 1.0000001;
    const dim3 grid((unsigned)nblk, (unsigned)ntiles);
    const size_t lds = words > 32 ? (size_t)kBitsRangeQT * words * sizeof(uint64_t) : 0;
    hipError_t e = hipSuccess;
#define MLVDB_BITS_RANGE_LAUNCH(L, LDSQ, FILL)                                                                             \
    do {                                                                                                                   \
        e = ensure_instance_lds<bits_range_kernel<L, LDSQ, FILL>>(lds, kBitsRangeQT * MLVDB_BITS_MAX_WORDS * 8);           \
        if (e != hipSuccess) return e;                                                                                     \
        bits_range_kernel<L, LDSQ, FILL><<<grid, 256, lds, s>>>(slots, pool, rn, mask, total, queries, qpop, nq, words,   \
                                                                metric, ham_max, radius, radius_up, cnt, off, cursor, keys); \
    } while (0)
#define MLVDB_BITS_RANGE_WALK(FILL)                                      \
    do {                                                                 \
        if (words > 32) MLVDB_BITS_RANGE_LAUNCH(16, true, FILL);         \
        else switch (bits_lanes(words)) {                                \
            case 1: MLVDB_BITS_RANGE_LAUNCH(1, false, FILL); break;      \
            case 2: MLVDB_BITS_RANGE_LAUNCH(2, false, FILL); break;      \
            case 4: MLVDB_BITS_RANGE_LAUNCH(4, false, FILL); break;      \
            case 8: MLVDB_BITS_RANGE_LAUNCH(8, false, FILL); break;      \
            default: MLVDB_BITS_RANGE_LAUNCH(16, false, FILL); break;    \
        }                                                                \
    } while (0)
    if (fill) MLVDB_BITS_RANGE_WALK(true);
    else MLVDB_BITS_RANGE_WALK(false);
#undef MLVDB_BITS_RANGE_WALK
#undef MLVDB_BITS_RANGE_LAUNCH
    return hipGetLastError();
}

hipError_t launch_bits_range_plan(const int32_t* cnt, int32_t n, int32_t capacity, int64_t* off, int32_t* over, hipStream_t s) {
    if (n < 1 || n > kBitsChunk || capacity < 1 || capacity > MLVDB_BITS_RANGE_MAX_HITS) return hipErrorInvalidValue;
    bits_range_plan_kernel<<<1, kBitsChunk, 0, s>>>(cnt, n, capacity, off, over);
    return hipGetLastError();
}

hipError_t launch_bits_range_sort(const int64_t* slots, const int64_t* pool, const uint64_t* queries, const int32_t* qpop,
                                  int32_t n, int32_t words, int32_t metric, int32_t longest, const int64_t* off,
                                  const uint64_t* keys, int64_t* out_lab, float* out_dist, double* out_d64, hipStream_t s) {
    if (n < 1 || n > kBitsSortMaxSegments || longest < 1 || longest > MLVDB_BITS_RANGE_MAX_HITS || words < 1 ||
        words > MLVDB_BITS_MAX_WORDS)
        return hipErrorInvalidValue;
    size_t np = 1;
    while (np < (size_t)longest) np <<= 1;
    const size_t lds = np * sizeof(uint64_t);
    const hipError_t e = ensure_instance_lds<bits_range_sort_kernel>(lds, MLVDB_BITS_RANGE_MAX_HITS * 8);
    if (e != hipSuccess) return e;
    // a long segment has 8 compare-exchanges per thread and step at 1,024 threads; a short one leaves no wave idle at 256
    const unsigned threads = np >= 4096 ? 1024 : 256;
    bits_range_sort_kernel<<<(unsigned)n, threads, lds, s>>>(slots, pool, queries, qpop, words, metric, bits_lanes(words), off,
                                                             keys, out_lab, out_dist, out_d64);
    return hipGetLastError();
}

}  // namespace mlvdb
