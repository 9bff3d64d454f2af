// Ordered metadata queries (include/mlvdb_order.h): the rows of ranks [offset, offset + limit) by an attribute column.
// mlvdb_geo_nearest (include/mlvdb_geo.h) is the same chain with another key source (kGeo): hav of the row's point from the
// call's centre, as geo_common.h defines it, in place of the value.
// Every candidate has a unique 96-bit composite key (order-preserving image of its value : label), so the N-th smallest
// composite, N = min(offset + limit, candidates), bounds exactly N rows and ties need no second mechanism.  It is found by
// most-significant-digit histogram passes (order_hist_kernel + the one-block order_scan_kernel per digit); the passes end as
// soon as the selected bucket and everything below it hold <= kOrderMaxRows rows, which order_collect_kernel then gathers
// and the one-workgroup order_sort_kernel ranks in LDS.  The kernels pass their state through OrderState on the device: the
// host enqueues the whole chain without reading anything back, and the launches behind a finished selection return at once.
// Launch shape of the passes over the index: where_eval_kernel's (256 threads, grid-stride, one row per thread and step, i0
// uniform over the block so that every ballot sees whole waves), over at most kOrderMaxBlocks blocks.
#include <algorithm>

#include "geo_common.h"
#include "internal.h"
#include "wave_peel.h"

namespace mlvdb {

namespace {

constexpr unsigned long long kSignBit = 0x8000000000000000ull;

// value bits -> uint64 that orders as the values do (int64: as integers; float64: as IEEE doubles, -0.0 folded onto 0.0)
__device__ __forceinline__ unsigned long long order_key(int64_t raw, bool f64, bool descending) {
    unsigned long long u = (unsigned long long)raw;
    if (f64) {
        if (u == kSignBit) u = 0;  // -0.0 ties with 0.0
        u = (u >> 63) ? ~u : (u ^ kSignBit);
    } else {
        u ^= kSignBit;
    }
    return descending ? ~u : u;
}

// The centre of a geo call as every thread holds it (uniform): its halves and its cosine, computed once per thread.
struct GeoCentre {
    int32_t lat, lon;
    double cos_lat;
};
template <bool kGeo>
__device__ __forceinline__ GeoCentre geo_centre(int64_t centre) {
    if constexpr (kGeo) return GeoCentre{geo_lat(centre), geo_lon(centre), geo_cos_lat(geo_lat(centre))};
    return GeoCentre{0, 0, 0.0};
}

// row i: a candidate -> its key; hit = live and matching (whatever its value).  kGeo: the key is hav from `c` (ascending: the
// bits of a double >= 0), and f64 / descending are not read.
template <bool kGeo>
__device__ __forceinline__ bool order_row(const uint8_t* __restrict__ mask, const float* __restrict__ rn,
                                          const int64_t* __restrict__ col, bool f64, bool descending, const GeoCentre& c,
                                          int64_t i, int64_t total, bool& hit, unsigned long long& key) {
    const bool in = i < total;
    hit = in && (mask ? mask[i] != 0 : rn[i] == rn[i]);  // (the mask of a program holds live rows only)
    const int64_t raw = hit ? col[i] : 0;
    if constexpr (kGeo) {
        const bool has = hit && raw != INT64_MIN;
        key = has ? order_key(__double_as_longlong(geo_hav(raw, c.lat, c.lon, c.cos_lat)), true, false) : 0;
        return has;
    }
    const double dv = __longlong_as_double(raw);
    const bool has = hit && (f64 ? dv == dv : raw != INT64_MIN);
    key = order_key(raw, f64, descending);
    return has;
}

// the digit of `pass`: bits [shift, shift + 11) of key:label, the last one its low 8 bits (pass uniform over the launch)
__device__ __forceinline__ uint32_t order_digit(unsigned long long key, uint32_t label, int pass) {
    const int shift = order_shift(pass);
    const unsigned long long lo = (key << 32) | label, hi = key >> 32;
    const unsigned long long v = shift >= 64 ? hi >> (shift - 64) : shift == 0 ? lo : (lo >> shift) | (hi << (64 - shift));
    return (uint32_t)v & (pass < kOrderPasses - 1 ? kOrderBins - 1 : 0xff);
}

// key:label >> low_bits (0 <= low_bits <= 96; 0 after the last digit: the whole composite) compared with the same of the bucket: -1 below, 0 inside, +1 above
__device__ __forceinline__ int order_side(unsigned long long key, uint32_t label, unsigned long long bkey, uint32_t blabel,
                                          uint32_t low_bits) {
    if (low_bits >= 96) return 0;
    if (low_bits >= 32) {
        const unsigned long long a = key >> (low_bits - 32), b = bkey >> (low_bits - 32);
        return a < b ? -1 : a > b ? 1 : 0;
    }
    if (key != bkey) return key < bkey ? -1 : 1;
    const uint32_t a = label >> low_bits, b = blabel >> low_bits;
    return a < b ? -1 : a > b ? 1 : 0;
}

}  // namespace

template <bool kGeo>
__global__ __launch_bounds__(256) void order_hist_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ rn,
                                                         const int64_t* __restrict__ col, int32_t f64, int32_t descending,
                                                         int64_t centre, int64_t total, int32_t pass,
                                                         unsigned long long* __restrict__ hist, OrderState* __restrict__ st) {
    __shared__ uint32_t lh[kOrderBins];
    __shared__ unsigned long long block_matched, block_absent;
    if (st->done) return;  // (uniform: written by an earlier launch)
    const unsigned long long bkey = st->key;
    const uint32_t blabel = st->label, low_bits = pass == 0 ? 96 : st->low_bits;  // (every candidate is in the first bucket)
    for (int s = threadIdx.x; s < kOrderBins; s += blockDim.x) lh[s] = 0;
    if (threadIdx.x == 0) block_matched = block_absent = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const GeoCentre c = geo_centre<kGeo>(centre);
    unsigned long long wave_matched = 0, wave_absent = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < total; i0 += stride) {
        const int64_t i = i0 + threadIdx.x;
        bool hit;
        unsigned long long key;
        const bool has = order_row<kGeo>(mask, rn, col, f64 != 0, descending != 0, c, i, total, hit, key);
        if (pass == 0) {
            const unsigned long long bh = __ballot(hit), ba = __ballot(hit && !has);
            if (lane == 0) {
                wave_matched += __popcll(bh);
                wave_absent += __popcll(ba);
            }
        }
        const bool inside = has && order_side(key, (uint32_t)i, bkey, blabel, low_bits) == 0;
        // all-equal and two-valued columns are the normal case (bool, year): their lanes share a bin, and one add serves them
        wave_peel_add(inside, (int64_t)order_digit(key, (uint32_t)i, pass),
                      [&](int64_t b, uint32_t n) { atomicAdd(&lh[b], n); });
    }
    if (lane == 0 && wave_matched) atomicAdd(&block_matched, wave_matched);
    if (lane == 0 && wave_absent) atomicAdd(&block_absent, wave_absent);
    __syncthreads();
    for (int s = threadIdx.x; s < kOrderBins; s += blockDim.x)
        if (lh[s]) atomicAdd(&hist[s], (unsigned long long)lh[s]);
    if (threadIdx.x == 0 && block_matched) atomicAdd(&st->matched, block_matched);
    if (threadIdx.x == 0 && block_absent) atomicAdd(&st->absent, block_absent);
}

hipError_t launch_order_hist(const uint8_t* mask, const float* rn, const int64_t* col, int32_t type, int32_t descending,
                             int64_t centre, int64_t total, int32_t pass, unsigned long long* hist, OrderState* st,
                             hipStream_t s) {
    if (total == 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, kOrderMaxBlocks);
    if (type == MLVDB_ATTR_GEO)
        order_hist_kernel<true><<<(unsigned)blocks, 256, 0, s>>>(mask, rn, col, 0, 0, centre, total, pass, hist, st);
    else
        order_hist_kernel<false><<<(unsigned)blocks, 256, 0, s>>>(mask, rn, col, type == MLVDB_ATTR_FLOAT64, descending, 0, total,
                                                                  pass, hist, st);
    return hipGetLastError();
}

// One block of 256 threads, 8 bins each: an inclusive scan of the threads' sums (a thread's own sum subtracted gives what
// lies before its bins), then the thread whose bins hold the rank walks them.  Thread 0 reads the state into LDS before the
// last barrier; after it only the one owner touches *st, so no thread can read what the owner has already updated.
// Invariant between the passes: st->below <= st->want - 1 < st->below + (rows in the selected bucket).
__global__ __launch_bounds__(256) void order_scan_kernel(const unsigned long long* __restrict__ hist, int32_t pass,
                                                         int64_t offset, int64_t limit, OrderState* __restrict__ st) {
    constexpr int kPer = kOrderBins / 256;
    __shared__ unsigned long long sums[256];
    __shared__ unsigned long long want_s, below_s, key_s;
    __shared__ uint32_t label_s;
    if (st->done) return;
    const int t = threadIdx.x;
    unsigned long long mine[kPer], sum = 0;
    for (int j = 0; j < kPer; ++j) {
        mine[j] = hist[t * kPer + j];
        sum += mine[j];
    }
    sums[t] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive scan
        const unsigned long long add = t >= d ? sums[t - d] : 0;
        __syncthreads();
        sums[t] += add;
        __syncthreads();
    }
    if (t == 0) {
        unsigned long long want = st->want;
        if (pass == 0) {  // every candidate is in the first bucket: their number fixes the rank
            const unsigned long long candidates = sums[255];
            want = (unsigned long long)(offset + limit) < candidates ? (unsigned long long)(offset + limit) : candidates;
            st->want = want;
            if (want <= (unsigned long long)offset) {  // nothing to return (n_collect stays 0)
                want = 0;
                st->done = 1;
            }
        }
        want_s = want;
        below_s = st->below;
        key_s = st->key;
        label_s = st->label;
    }
    __syncthreads();
    const unsigned long long want = want_s;
    if (want == 0) return;
    const unsigned long long r = want - 1 - below_s;  // rank inside the bucket, 0-based
    unsigned long long before = sums[t] - sum;
    if (r < before || r >= before + sum) return;  // exactly one thread goes on (the bucket holds rank `want`)
    int g = 0;
    for (; g < kPer - 1 && r >= before + mine[g]; ++g) before += mine[g];
    const uint32_t digit = (uint32_t)(t * kPer + g);
    const int shift = order_shift(pass);
    unsigned long long key = key_s;
    uint32_t label = label_s;
    if (shift >= 32) {
        key |= (unsigned long long)digit << (shift - 32);
    } else {
        key |= (unsigned long long)digit >> (32 - shift);  // (only the digit that straddles key and label has bits here)
        label |= digit << shift;
    }
    const unsigned long long below = below_s + before, n = below + mine[g];
    st->key = key;
    st->label = label;
    st->low_bits = (uint32_t)shift;
    st->below = below;
    st->passes = (uint32_t)pass + 1;
    if (n <= (unsigned long long)kOrderMaxRows) {  // (the last pass leaves one row in the bucket: n == want)
        st->n_collect = (uint32_t)n;
        st->done = 1;
    }
}

hipError_t launch_order_scan(const unsigned long long* hist, int32_t pass, int64_t offset, int64_t limit, OrderState* st,
                             hipStream_t s) {
    order_scan_kernel<<<1, 256, 0, s>>>(hist, pass, offset, limit, st);
    return hipGetLastError();
}

template <bool kGeo>
__global__ __launch_bounds__(256) void order_collect_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ rn,
                                                            const int64_t* __restrict__ col, int32_t f64, int32_t descending,
                                                            int64_t centre, int64_t total, OrderState* __restrict__ st,
                                                            unsigned long long* __restrict__ keys,
                                                            uint32_t* __restrict__ labels) {
    if (st->n_collect == 0) return;
    const unsigned long long bkey = st->key;
    const uint32_t blabel = st->label, low_bits = st->low_bits;
    const GeoCentre c = geo_centre<kGeo>(centre);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        bool hit;
        unsigned long long key;
        if (!order_row<kGeo>(mask, rn, col, f64 != 0, descending != 0, c, i, total, hit, key)) continue;
        if (order_side(key, (uint32_t)i, bkey, blabel, low_bits) > 0) continue;
        const uint32_t at = atomicAdd(&st->cursor, 1u);
        if (at < (uint32_t)kOrderMaxRows) {
            keys[at] = key;
            labels[at] = (uint32_t)i;
        } else {
            atomicOr(&st->overflow, 1u);  // the selection and this pass disagree: MLVDB_ERR_INTERNAL, never a store out of bounds
        }
    }
}

hipError_t launch_order_collect(const uint8_t* mask, const float* rn, const int64_t* col, int32_t type, int32_t descending,
                                int64_t centre, int64_t total, OrderState* st, unsigned long long* keys, uint32_t* labels,
                                hipStream_t s) {
    if (total == 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, kOrderMaxBlocks);
    if (type == MLVDB_ATTR_GEO)
        order_collect_kernel<true><<<(unsigned)blocks, 256, 0, s>>>(mask, rn, col, 0, 0, centre, total, st, keys, labels);
    else
        order_collect_kernel<false><<<(unsigned)blocks, 256, 0, s>>>(mask, rn, col, type == MLVDB_ATTR_FLOAT64, descending, 0,
                                                                     total, st, keys, labels);
    return hipGetLastError();
}

// Bitonic sort of the collected (key, label) pairs in LDS (48 KiB), padded to a power of two with pairs above every real one
// (a real label is below 2^31), then ranks [offset, want) out.  kGeo: also the rows' distances in metres, from the same hav.
template <bool kGeo>
__global__ __launch_bounds__(1024) void order_sort_kernel(const unsigned long long* __restrict__ keys,
                                                          const uint32_t* __restrict__ labels, const int64_t* __restrict__ col,
                                                          int64_t centre, int64_t total, int64_t offset,
                                                          OrderState* __restrict__ st, int64_t* __restrict__ out_labels,
                                                          int64_t* __restrict__ out_values, double* __restrict__ out_dist) {
    __shared__ unsigned long long sk[kOrderMaxRows];
    __shared__ uint32_t sl[kOrderMaxRows];
    const uint32_t n = st->cursor < (uint32_t)kOrderMaxRows ? st->cursor : (uint32_t)kOrderMaxRows;
    if (st->n_collect == 0 || n == 0) return;
    uint32_t m = 2;
    while (m < n) m <<= 1;  // <= kOrderMaxRows
    for (uint32_t s = threadIdx.x; s < m; s += blockDim.x) {
        sk[s] = s < n ? keys[s] : ~0ull;
        sl[s] = s < n ? labels[s] : ~0u;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < m / 2; t += blockDim.x) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long ka = sk[lo], kb = sk[hi];
                const uint32_t la = sl[lo], lb = sl[hi];
                const bool b_first = kb < ka || (kb == ka && lb < la);
                if (b_first == ((lo & k) == 0)) {
                    sk[lo] = kb;
                    sk[hi] = ka;
                    sl[lo] = lb;
                    sl[hi] = la;
                }
            }
            __syncthreads();
        }
    }
    const unsigned long long want = st->want < n ? st->want : n;
    const GeoCentre c = geo_centre<kGeo>(centre);
    for (unsigned long long r = (unsigned long long)offset + threadIdx.x; r < want; r += blockDim.x) {
        const uint32_t label = sl[r];
        if ((int64_t)label >= total) continue;  // (never: a collected label is a row)
        out_labels[r - offset] = (int64_t)label;
        const int64_t raw = col[label];
        out_values[r - offset] = raw;  // the stored bits, not the key's image of them
        if constexpr (kGeo) out_dist[r - offset] = geo_dist_m(geo_hav(raw, c.lat, c.lon, c.cos_lat));
    }
    if (threadIdx.x == 0) st->n_out = want > (unsigned long long)offset ? (uint32_t)(want - offset) : 0;
}

hipError_t launch_order_sort(const unsigned long long* keys, const uint32_t* labels, const int64_t* col, int32_t type,
                             int64_t centre, int64_t total, int64_t offset, OrderState* st, int64_t* out_labels,
                             int64_t* out_values, double* out_dist, hipStream_t s) {
    if (type == MLVDB_ATTR_GEO)
        order_sort_kernel<true><<<1, 1024, 0, s>>>(keys, labels, col, centre, total, offset, st, out_labels, out_values, out_dist);
    else
        order_sort_kernel<false><<<1, 1024, 0, s>>>(keys, labels, col, 0, total, offset, st, out_labels, out_values, nullptr);
    return hipGetLastError();
}

}  // namespace mlvdb
