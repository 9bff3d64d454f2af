// Search by stored examples (include/mlvdb_like.h): the two kernels around the plain device search.
//   like_query_kernel   one 256-thread block per query.  Phase 1 leaves each example's factor t_j and the offset of its row
//                       in LDS; on a cosine index t_j = weight_j * inv_j with inv_j formed as the query prep forms it (the
//                       column walk c = t, t + 256, ... over the padded ld, query_norm_wave_sum, query_aux_from_sums), so
//                       the bits are those launch_query_prep gives the row's values.  Phase 2: thread t owns the columns
//                       c = t, t + 256, ...; per column it walks the examples in order -- acc = acc + t_j * x_j[c], one
//                       rounded fp64 product and one rounded fp64 addition -- and writes (float)acc to the dense [n, dim]
//                       batch search_device_impl takes.  A row is a sequence of whole 64-byte pieces 1 KiB apart
//                       (layout.h); lanes 16a .. 16a + 15 of a wave hold the 16 columns of one piece, so every load of a
//                       wave is four whole pieces.
//   like_strip_kernel   one wavefront per query (four per block).  Lane e holds example label e (<= 64 of them); the ranked
//                       list of F entries is walked in chunks of 64, each lane tests its entry against the examples, and a
//                       ballot with a prefix popcount gives every kept entry its output position behind a running base:
//                       the order is kept.  The first k kept entries go to the outputs, the tail is padded; entries beyond
//                       the list's count are never read.
// Everything is fp64 (the library is built with -ffp-contract=off, restated below for this file).  No atomics, no scratch.
#include "internal.h"
#include "query_norm.h"

#pragma clang fp contract(off)

namespace mlvdb {

template <bool COSINE>
__global__ __launch_bounds__(256) void like_query_kernel(const float* __restrict__ X, const int32_t dim, const int32_t ld,
                                                         const int64_t* __restrict__ ex_labels,
                                                         const double* __restrict__ ex_weights,
                                                         const int64_t* __restrict__ ex_offsets,
                                                         const float* __restrict__ base, float* __restrict__ out) {
    __shared__ double tj[kLikeMaxExamples];        // the factor of example j
    __shared__ int64_t row_at[kLikeMaxExamples];   // float offset of (row of example j, column 0)
    __shared__ double sums[kLikeMaxExamples][4];   // cosine: the four wave sums of example j's squared norm
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e0 = ex_offsets[q];
    const int m = (int)min((int64_t)kLikeMaxExamples, max((int64_t)0, ex_offsets[q + 1] - e0));  // (the entry point checked it)
    if ((int)threadIdx.x < m) row_at[threadIdx.x] = layout_offset(ex_labels[e0 + threadIdx.x], 0, ld);
    __syncthreads();
    if (COSINE) {
        for (int j = 0; j < m; ++j) {
            const float* row = X + row_at[j];
            double s = 0.0;
            for (int c = threadIdx.x; c < ld; c += 256) {
                const float v = c < dim ? row[(int64_t)(c >> 4) * kGroupFloats + (c & 15)] : 0.f;
                s = __builtin_fma((double)v, (double)v, s);
            }
            s = query_norm_wave_sum(s);
            if (lane == 0) sums[j][wave] = s;
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < m) {
        const double w = ex_weights[e0 + threadIdx.x];
        tj[threadIdx.x] = COSINE ? w * query_aux_from_sums(sums[threadIdx.x], kSpaceCosine) : w;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < dim; c += 256) {
        const int64_t at = (int64_t)(c >> 4) * kGroupFloats + (c & 15);
        double acc = base ? (double)base[(int64_t)q * dim + c] : 0.0;
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
            const double p = tj[j] * (double)X[row_at[j] + at];
            acc = acc + p;
        }
        out[(int64_t)q * dim + c] = (float)acc;
    }
}

__global__ __launch_bounds__(256) void like_strip_kernel(const int64_t* __restrict__ l_lab, const float* __restrict__ l_dist,
                                                         const double* __restrict__ l_d64, const int32_t* __restrict__ l_cnt,
                                                         const int32_t F, const int64_t* __restrict__ ex_labels,
                                                         const int64_t* __restrict__ ex_offsets, const int32_t exclude,
                                                         const int32_t nq, const int32_t k, int64_t* __restrict__ out_labels,
                                                         float* __restrict__ out_dist, int32_t* __restrict__ out_counts,
                                                         double* __restrict__ out_d64) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;  // (wave-uniform; no barrier follows)
    const int64_t e0 = ex_offsets[q];
    const int m = exclude ? (int)min((int64_t)kLikeMaxExamples, max((int64_t)0, ex_offsets[q + 1] - e0)) : 0;
    const long long mine = lane < m ? (long long)ex_labels[e0 + lane] : -1;  // (a valid entry never holds a negative label)
    const int cnt = min(max(l_cnt[q], 0), F);
    const int64_t l0 = (int64_t)q * F, o0 = (int64_t)q * k;
    int kept = 0;  // entries kept so far: the running base of the compaction
    for (int i0 = 0; i0 < cnt && kept < k; i0 += 64) {
        const int i = i0 + lane;
        const bool have = i < cnt;
        const long long lab = have ? (long long)l_lab[l0 + i] : -2;
        bool is_example = false;
        for (int e = 0; e < m; ++e) is_example |= lab == __shfl(mine, e);
        const bool keep = have && !is_example;
        const unsigned long long votes = __ballot(keep);
        const int pos = kept + __popcll(votes & ((1ull << lane) - 1ull));
        if (keep && pos < k) {
            out_labels[o0 + pos] = lab;
            out_dist[o0 + pos] = l_dist[l0 + i];
            out_d64[o0 + pos] = l_d64[l0 + i];
        }
        kept += __popcll(votes);
    }
    kept = min(kept, k);
    for (int t = kept + lane; t < k; t += 64) {
        out_labels[o0 + t] = -1;
        out_dist[o0 + t] = __builtin_inff();
        out_d64[o0 + t] = __builtin_inf();
    }
    if (lane == 0) out_counts[q] = kept;
}

hipError_t launch_like_query(const float* X, int32_t dim, int32_t ld, int32_t space, const int64_t* ex_labels,
                             const double* ex_weights, const int64_t* ex_offsets, const float* base, int32_t nq, float* out,
                             hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    if (space == kSpaceCosine)
        like_query_kernel<true><<<nq, 256, 0, s>>>(X, dim, ld, ex_labels, ex_weights, ex_offsets, base, out);
    else
        like_query_kernel<false><<<nq, 256, 0, s>>>(X, dim, ld, ex_labels, ex_weights, ex_offsets, base, out);
    return hipGetLastError();
}

hipError_t launch_like_strip(const int64_t* l_lab, const float* l_dist, const double* l_d64, const int32_t* l_cnt, int32_t nq,
                             int32_t fetch, const int64_t* ex_labels, const int64_t* ex_offsets, int32_t exclude, int32_t k,
                             int64_t* out_labels, float* out_dist, int32_t* out_counts, double* out_d64, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    like_strip_kernel<<<(nq + 3) / 4, 256, 0, s>>>(l_lab, l_dist, l_d64, l_cnt, fetch, ex_labels, ex_offsets, exclude, nq, k,
                                                   out_labels, out_dist, out_counts, out_d64);
    return hipGetLastError();
}

}  // namespace mlvdb
