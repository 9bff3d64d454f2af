// Attribute statistics (include/mlvdb_stats.h): rows, count, min, max and a 128-bit sum of one column per distinct value of
// a second one.  Launch shape and predicate of the facet kernels (kernels_facet.hip): 256 threads, grid-stride, one row per
// thread and pass, i0 uniform over the block so that every ballot sees whole waves; the program is evaluated here, nothing
// is written per row.  Everything that accumulates is an integer atomic that commutes -- add, unsigned min / max on
// order-preserving images, and the two adds of a 128-bit sum -- so the table after a kernel does not depend on the order in
// which lanes, waves and blocks arrive.
#include <algorithm>

#include "internal.h"
#include "where_common.h"

namespace mlvdb {

namespace {

constexpr unsigned long long kStatsEmpty = 0x8000000000000000ull;  // INT64_MIN: never a present value of `by`

// What a lane, a wave or a block adds under one key.  hi:lo is two's complement in 128 bits.
struct StatsAcc {
    uint32_t rows, count;
    unsigned long long mn, mx, lo, hi;
};

__device__ __forceinline__ StatsAcc stats_none() { return StatsAcc{0, 0, ~0ull, 0, 0, 0}; }

__device__ __forceinline__ void acc_add128(StatsAcc& a, unsigned long long lo, unsigned long long hi) {
    a.lo += lo;
    a.hi += hi + (a.lo < lo ? 1 : 0);
}

// a += one present value: its image for min / max, its term q for the sum
__device__ __forceinline__ void acc_value(StatsAcc& a, unsigned long long image, int64_t q) {
    a.count += 1;
    a.mn = image < a.mn ? image : a.mn;
    a.mx = image > a.mx ? image : a.mx;
    acc_add128(a, (unsigned long long)q, q < 0 ? ~0ull : 0);
}

// lo += alo, and the carry out of the low word joins ahi: both adds commute, so hi:lo is the exact sum mod 2^128 in whatever
// order the adds of different lanes land (LDS or HBM)
__device__ __forceinline__ void atomic_add128(unsigned long long* lo, unsigned long long* hi, unsigned long long alo,
                                              unsigned long long ahi) {
    if (!(alo | ahi)) return;
    const unsigned long long old = atomicAdd(lo, alo);
    ahi += old + alo < old ? 1 : 0;
    if (ahi) atomicAdd(hi, ahi);
}

// The peel of wave_peel_add with a folded payload: the lanes that hold the first active lane's key fold what they add in a
// masked butterfly (the other lanes feed it the neutral element), and the leading lane hands the fold to put(key, fold) --
// one call per key instead of one per lane, for at most kFacetPeelRounds leading keys; a round that found its key on a single
// lane ends the peel.  MINMAX / SUM: the parts of the payload the caller uses (rows and count always fold).  Every lane of
// the wave must call this; put runs at one call site after the rounds (a lane leads at most once).
template <bool MINMAX, bool SUM, class Put>
__device__ __forceinline__ void stats_peel(bool has, int64_t key, StatsAcc mine, Put&& put) {
    const int lane = threadIdx.x & 63;
    bool puts = false;
    for (int r = 0; r < kFacetPeelRounds; ++r) {
        const unsigned long long active = __ballot(has);
        if (!active) break;
        const int leader = __ffsll((long long)active) - 1;
        const uint32_t klo = __builtin_amdgcn_readlane((int)(uint32_t)key, leader);
        const uint32_t khi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)key >> 32), leader);
        const bool same = has && key == (int64_t)(((uint64_t)khi << 32) | klo);
        const int n = __popcll(__ballot(same));
        if (n > 1) {
            StatsAcc f = same ? mine : stats_none();
#pragma unroll
            for (int x = 1; x < 64; x <<= 1) {
                f.rows += (uint32_t)__shfl_xor((int)f.rows, x);
                f.count += (uint32_t)__shfl_xor((int)f.count, x);
                if (MINMAX) {
                    const unsigned long long a = (unsigned long long)__shfl_xor((long long)f.mn, x);
                    const unsigned long long b = (unsigned long long)__shfl_xor((long long)f.mx, x);
                    f.mn = a < f.mn ? a : f.mn;
                    f.mx = b > f.mx ? b : f.mx;
                }
                if (SUM) {  // a (hi, lo) pair: 64 terms of 2^62 do not fit one word
                    const unsigned long long olo = (unsigned long long)__shfl_xor((long long)f.lo, x);
                    const unsigned long long ohi = (unsigned long long)__shfl_xor((long long)f.hi, x);
                    acc_add128(f, olo, ohi);
                }
            }
            if (lane == leader) mine = f;
        }
        if (lane == leader) puts = true;
        has = has && !same;
        if (n == 1) break;
    }
    if (puts || has) put(key, mine);
}

// The block's table in LDS: open addressing, linear probing, the key claimed by a 64-bit compare-and-swap -> its slot, or -1
// after kFacetLdsProbes probes (the caller then goes to the global table)
template <int SLOTS>
__device__ __forceinline__ int lds_claim(unsigned long long* keys, int64_t key) {
    uint32_t s = (uint32_t)facet_hash(key) & (SLOTS - 1);
    for (int p = 0; p < kFacetLdsProbes; ++p) {
        const unsigned long long prev = atomicCAS(&keys[s], kStatsEmpty, (unsigned long long)key);
        if (prev == kStatsEmpty || prev == (unsigned long long)key) return (int)s;
        s = (s + 1) & (SLOTS - 1);
    }
    return -1;
}

// ... in HBM, as global_insert of the facet kernels: whoever claims an empty slot counts one more distinct key (exact while
// the table is not full).  Once more than max_groups are counted the call is an overflow whatever follows, so further
// inserts are dropped; a full table flags the overflow itself.
template <bool SUM>
__device__ __forceinline__ void global_put(const StatsTable& t, int64_t key, const StatsAcc& a) {
    if (__hip_atomic_load(&t.ctr[kFacetDistinct], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > t.max_groups) return;
    uint64_t s = facet_hash(key) & t.mask;
    for (uint64_t p = 0; p <= t.mask; ++p) {
        const unsigned long long prev = atomicCAS(&t.keys[s], kStatsEmpty, (unsigned long long)key);
        if (prev == kStatsEmpty) atomicAdd(&t.ctr[kFacetDistinct], 1ull);
        if (prev == kStatsEmpty || prev == (unsigned long long)key) {
            atomicAdd(&t.rows[s], (unsigned long long)a.rows);
            if (a.count) {
                atomicAdd(&t.count[s], (unsigned long long)a.count);
                atomicMin(&t.mn[s], a.mn);
                atomicMax(&t.mx[s], a.mx);
                if (SUM) atomic_add128(&t.lo[s], &t.hi[s], a.lo, a.hi);
            }
            return;
        }
        s = (s + 1) & t.mask;
    }
    atomicOr(&t.ctr[kFacetOverflow], 1ull);
}

// the slot of key in the final table, or -1 (the probe is bounded: an overflowed table may be full)
__device__ __forceinline__ int64_t global_find(const StatsTable& t, int64_t key) {
    uint64_t s = facet_hash(key) & t.mask;
    for (uint64_t p = 0; p <= t.mask; ++p) {
        const unsigned long long k = t.keys[s];
        if (k == (unsigned long long)key) return (int64_t)s;
        if (k == kStatsEmpty) return -1;
        s = (s + 1) & t.mask;
    }
    return -1;
}

// row i: live and matching -> hit; its group key (0 when by == nullptr, INT64_MIN = no value of `by`) and, when it has a
// group, its value of `col` -- both only loaded for a hit
__device__ __forceinline__ bool stats_row(const WhereOp* sp, int32_t n_ops, const int64_t* __restrict__ set,
                                          const float* __restrict__ rn, const int64_t* __restrict__ by,
                                          const int64_t* __restrict__ col, int64_t i, int64_t total, int64_t& key, int64_t& raw) {
    const bool in = i < total;
    const bool live = in && rn[i] == rn[i];  // tombstoned rows (NaN norm) never count
    const bool hit = live && (n_ops == 0 || where_eval_row(sp, n_ops, set, i, live));
    key = !hit ? INT64_MIN : by ? by[i] : 0;
    raw = key != INT64_MIN ? col[i] : INT64_MIN;
    return hit;
}

// a double's bits: a present value (not NaN)
__device__ __forceinline__ bool f64_present(int64_t raw) { return ((uint64_t)raw & 0x7FFFFFFFFFFFFFFFull) <= 0x7FF0000000000000ull; }

// rint(v * 2^(61 - E)), half to even, of a finite double by its bits, in integers: |v| < 2^(E + 1), so |term| <= 2^62
__device__ __forceinline__ int64_t stats_term(uint64_t bits, int E) {
    const int ef = (int)((bits >> 52) & 0x7FF);
    const uint64_t mant = (bits & 0xFFFFFFFFFFFFFull) | (ef ? 1ull << 52 : 0);
    const int sh = (ef ? ef : 1) - 1075 + 61 - E;  // v = mant * 2^(ef - 1075): the term is mant * 2^sh, sh <= 61
    uint64_t q = 0;
    if (sh >= 0) {
        q = mant << sh;
    } else if (sh >= -54) {  // (below, mant * 2^sh < 1/2)
        const int r = -sh;
        const uint64_t rem = mant & ((1ull << r) - 1), half = 1ull << (r - 1);
        q = mant >> r;
        q += (rem > half || (rem == half && (q & 1))) ? 1 : 0;
    }
    return (bits >> 63) ? -(int64_t)q : (int64_t)q;
}

}  // namespace

// Pass 1.  GROUPED: the keys of a wave's rows are peeled and folded, then put into the block's table.  Otherwise every thread
// keeps its own partial across the grid-stride loop and the wave folds once at the end (one key: the peel's first round);
// the block's table then holds that one key and is kStatsLdsSlotsOne slots small, which leaves the occupancy to the VGPRs.
template <bool F64, bool GROUPED>
__global__ __launch_bounds__(256) void stats_pass1_kernel(const WhereOp* __restrict__ prog, int32_t n_ops,
                                                          const int64_t* __restrict__ set, const float* __restrict__ rn,
                                                          const int64_t* __restrict__ by, const int64_t* __restrict__ col,
                                                          int64_t total, StatsTable t) {
    constexpr bool SUM = !F64;
    constexpr int SLOTS = GROUPED ? kStatsLdsSlots : kStatsLdsSlotsOne;
    __shared__ WhereOp sp[kWhereMaxOps];
    __shared__ unsigned long long lkeys[SLOTS], lmn[SLOTS], lmx[SLOTS];
    __shared__ unsigned long long llo[SUM ? SLOTS : 1], lhi[SUM ? SLOTS : 1];
    __shared__ uint32_t lrows[SLOTS], lcount[SLOTS];
    __shared__ unsigned long long block_matched, block_absent;
    if ((int)threadIdx.x < n_ops) sp[threadIdx.x] = prog[threadIdx.x];
    for (int s = threadIdx.x; s < SLOTS; s += blockDim.x) {
        lkeys[s] = kStatsEmpty;
        lmn[s] = ~0ull;
        lmx[s] = 0;
        lrows[s] = lcount[s] = 0;
        if (SUM) llo[s] = lhi[s] = 0;
    }
    if (threadIdx.x == 0) block_matched = block_absent = 0;
    __syncthreads();
    auto put = [&](int64_t key, const StatsAcc& a) {
        const int s = lds_claim<SLOTS>(lkeys, key);
        if (s < 0) return global_put<SUM>(t, key, a);
        atomicAdd(&lrows[s], a.rows);
        if (a.count) {
            atomicAdd(&lcount[s], a.count);
            atomicMin(&lmn[s], a.mn);
            atomicMax(&lmx[s], a.mx);
            if (SUM) atomic_add128(&llo[s], &lhi[s], a.lo, a.hi);
        }
    };
    const int lane = threadIdx.x & 63;
    unsigned long long wave_matched = 0, wave_absent = 0;
    StatsAcc own = stats_none();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        int64_t key, raw;
        const bool hit = stats_row(sp, n_ops, set, rn, by, col, i0 + threadIdx.x, total, key, raw);
        const bool has = hit && key != INT64_MIN;
        const bool present = has && (F64 ? f64_present(raw) : raw != INT64_MIN);
        const unsigned long long image = F64 ? stats_image_f64((uint64_t)raw) : stats_image_i64(raw);
        if (GROUPED) {
            const unsigned long long bh = __ballot(hit), ba = __ballot(hit && !has);
            if (lane == 0) {
                wave_matched += __popcll(bh);
                wave_absent += __popcll(ba);
            }
            StatsAcc a = stats_none();
            a.rows = 1;
            if (present) acc_value(a, image, SUM ? raw : 0);
            stats_peel<true, SUM>(has, key, a, put);
        } else {
            own.rows += has ? 1 : 0;
            if (present) acc_value(own, image, SUM ? raw : 0);
        }
    }
    if (!GROUPED) stats_peel<true, SUM>(own.rows != 0, 0, own, put);  // (matched: the table's rows, at the flush)
    if (lane == 0 && wave_matched) atomicAdd(&block_matched, wave_matched);
    if (lane == 0 && wave_absent) atomicAdd(&block_absent, wave_absent);
    __syncthreads();
    for (int s = threadIdx.x; s < SLOTS; s += blockDim.x) {
        if (lkeys[s] == kStatsEmpty) continue;
        const StatsAcc a{lrows[s], lcount[s], lmn[s], lmx[s], SUM ? llo[s] : 0, SUM ? lhi[s] : 0};
        global_put<SUM>(t, (int64_t)lkeys[s], a);
        if (!GROUPED) atomicAdd(&t.ctr[kFacetMatched], (unsigned long long)a.rows);
    }
    if (threadIdx.x == 0 && block_matched) atomicAdd(&t.ctr[kFacetMatched], block_matched);
    if (threadIdx.x == 0 && block_absent) atomicAdd(&t.ctr[kFacetAbsent], block_absent);
}

hipError_t launch_stats_pass1(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* by,
                              const int64_t* col, bool f64, int64_t total, const StatsTable& t, hipStream_t s) {
    if (total == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 16);
    if (f64 && by)
        stats_pass1_kernel<true, true><<<blocks, 256, 0, s>>>(prog, n_ops, set, rn, by, col, total, t);
    else if (f64)
        stats_pass1_kernel<true, false><<<blocks, 256, 0, s>>>(prog, n_ops, set, rn, by, col, total, t);
    else if (by)
        stats_pass1_kernel<false, true><<<blocks, 256, 0, s>>>(prog, n_ops, set, rn, by, col, total, t);
    else
        stats_pass1_kernel<false, false><<<blocks, 256, 0, s>>>(prog, n_ops, set, rn, by, col, total, t);
    return hipGetLastError();
}

// Pass 2 (float64 columns): every row finds its group's slot in the final table by probing, takes E from the slot's min and
// max and adds its term.  The block's table is keyed by the slot; the terms of one slot fold as the keys of pass 1 do.
template <bool GROUPED>
__global__ __launch_bounds__(256) void stats_pass2_kernel(const WhereOp* __restrict__ prog, int32_t n_ops,
                                                          const int64_t* __restrict__ set, const float* __restrict__ rn,
                                                          const int64_t* __restrict__ by, const int64_t* __restrict__ col,
                                                          int64_t total, StatsTable t) {
    constexpr int SLOTS = GROUPED ? kStatsLdsSlots : kStatsLdsSlotsOne;
    __shared__ WhereOp sp[kWhereMaxOps];
    __shared__ unsigned long long lkeys[SLOTS], llo[SLOTS], lhi[SLOTS];
    // an overflowed pass 1: the arrays are unspecified, and keys may be missing from the table (uniform over the grid: pass 1
    // has ended)
    if (t.ctr[kFacetOverflow] || t.ctr[kFacetDistinct] > t.max_groups) return;
    if ((int)threadIdx.x < n_ops) sp[threadIdx.x] = prog[threadIdx.x];
    for (int s = threadIdx.x; s < SLOTS; s += blockDim.x) {
        lkeys[s] = kStatsEmpty;
        llo[s] = lhi[s] = 0;
    }
    __syncthreads();
    auto put = [&](int64_t slot, const StatsAcc& a) {
        const int s = lds_claim<SLOTS>(lkeys, slot);
        if (s < 0) return atomic_add128(&t.lo[slot], &t.hi[slot], a.lo, a.hi);
        atomic_add128(&llo[s], &lhi[s], a.lo, a.hi);
    };
    // the exponent of a slot: false when its sum stays 0 (an infinity in the group, or nothing but zeros)
    auto exponent = [&](int64_t slot, int* E) {
        return stats_exponent(stats_bits_f64(t.mn[slot]), stats_bits_f64(t.mx[slot]), E);
    };
    StatsAcc own = stats_none();
    int E0 = 0;
    const int64_t slot0 = GROUPED ? -1 : global_find(t, 0);
    const bool sums0 = slot0 >= 0 && t.count[slot0] && exponent(slot0, &E0);
    if (!GROUPED && !sums0) return;  // (uniform over the grid)
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        int64_t key, raw;
        const bool hit = stats_row(sp, n_ops, set, rn, by, col, i0 + threadIdx.x, total, key, raw);
        const bool finite = hit && key != INT64_MIN && ((uint64_t)raw & 0x7FFFFFFFFFFFFFFFull) < 0x7FF0000000000000ull;
        if (GROUPED) {
            const int64_t slot = finite ? global_find(t, key) : -1;
            int E = 0;
            const bool sums = slot >= 0 && exponent(slot, &E);
            StatsAcc a = stats_none();
            if (sums) acc_value(a, 0, stats_term((uint64_t)raw, E));
            stats_peel<false, true>(sums, slot, a, put);
        } else if (finite) {
            acc_value(own, 0, stats_term((uint64_t)raw, E0));
        }
    }
    if (!GROUPED) stats_peel<false, true>(own.count != 0, slot0, own, put);
    __syncthreads();
    for (int s = threadIdx.x; s < SLOTS; s += blockDim.x)
        if (lkeys[s] != kStatsEmpty) atomic_add128(&t.lo[lkeys[s]], &t.hi[lkeys[s]], llo[s], lhi[s]);
}

hipError_t launch_stats_pass2(const WhereOp* prog, int32_t n_ops, const int64_t* set, const float* rn, const int64_t* by,
                              const int64_t* col, int64_t total, const StatsTable& t, hipStream_t s) {
    if (total == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 16);
    if (by)
        stats_pass2_kernel<true><<<blocks, 256, 0, s>>>(prog, n_ops, set, rn, by, col, total, t);
    else
        stats_pass2_kernel<false><<<blocks, 256, 0, s>>>(prog, n_ops, set, rn, by, col, total, t);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void stats_collect_kernel(StatsTable t, unsigned long long* __restrict__ out) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = t.keys[s];
        if (key == kStatsEmpty) continue;
        const unsigned long long at = atomicAdd(&t.ctr[kFacetCursor], 1ull);
        if (at < t.max_groups) {  // (an overflowed table may hold more: its arrays are unspecified, never out of bounds)
            unsigned long long* rec = out + at * kStatsRecord;
            rec[0] = key;
            rec[1] = t.rows[s];
            rec[2] = t.count[s];
            rec[3] = t.mn[s];
            rec[4] = t.mx[s];
            rec[5] = t.hi[s];
            rec[6] = t.lo[s];
            rec[7] = 0;
        }
    }
}

hipError_t launch_stats_collect(const StatsTable& t, unsigned long long* out, hipStream_t s) {
    const int64_t blocks = std::min<int64_t>(((int64_t)t.mask + 256) / 256, 256 * 16);
    stats_collect_kernel<<<(unsigned)blocks, 256, 0, s>>>(t, out);
    return hipGetLastError();
}

}  // namespace mlvdb
