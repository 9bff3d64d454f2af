// Diversified kNN (include/mlvdb_mmr.h): greedy maximal-marginal-relevance selection over the ranked candidate list the
// plain device search left for each query.
//   mmr_select_kernel   one 256-thread block per query.  LDS: the picked row as fp64 [ld] (the `qs` of accumulate_rows),
//                       dq[F] (candidate-to-query distances, the list's own bits), mind[F] (distance to the nearest pick so
//                       far) and the picked flags [F] -- ld x 8 + F x 20 bytes.  Per step: block-wide argmin of
//                       obj = lambda dq - (1 - lambda) mind in the (objective, position) order, thread 0 writes the step's
//                       outputs, the block loads the picked row from its panel and forms its norm term as the query prep
//                       does, and each wave scores 16 candidates per iteration with pair_distance_kernel's addressing --
//                       D(s, i) has the bits mlvdb_pair_distances gives (values of row c_s, label c_i).
// Everything is fp64; the objective is two rounded products and one rounded subtraction (the library is built with
// -ffp-contract=off, restated below for this file).  No atomics, no scratch.
#include "internal.h"
#include "query_norm.h"
#include "scan_common.h"

#pragma clang fp contract(off)

namespace mlvdb {

namespace {
constexpr int32_t kMmrNone = 0x7fffffff;  // "no candidate": loses to every position

// (objective, position) order, ties to the lower position.  A NaN objective compares neither way, so the position decides:
// some unpicked candidate always wins.
__device__ __forceinline__ bool mmr_better(double ao, int32_t ai, double bo, int32_t bi) {
    return ai != kMmrNone && (bi == kMmrNone || ao < bo || (!(bo < ao) && ai < bi));
}
}  // namespace

template <int SPACE>
__global__ __launch_bounds__(256) void mmr_select_kernel(const float* __restrict__ X, const int32_t dim, const int32_t ld,
                                                         const int64_t* __restrict__ l_lab, const float* __restrict__ l_dist,
                                                         const double* __restrict__ l_d64, const int32_t* __restrict__ l_cnt,
                                                         const int32_t F, const int32_t k, const double lambda,
                                                         const double one_minus_lambda, int64_t* __restrict__ out_labels,
                                                         float* __restrict__ out_dist, int32_t* __restrict__ out_counts,
                                                         double* __restrict__ out_d64, int32_t* __restrict__ out_rank,
                                                         double* __restrict__ out_obj) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* qs = reinterpret_cast<double*>(smem);       // [ld]  the picked row
    double* dq = qs + ld;                               // [F]
    double* mind = dq + F;                              // [F]
    int32_t* picked = reinterpret_cast<int32_t*>(mind + F);  // [F]
    __shared__ double red[4];
    __shared__ double wbest_o[4];
    __shared__ int32_t wbest_i[4];
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, r = lane & 15;
    const int m = min(max(l_cnt[q], 0), F);  // valid entries of the list, ranked by (distance, label)
    const int npick = min(k, m);
    const int64_t* lab = l_lab + (int64_t)q * F;
    const int64_t o0 = (int64_t)q * k;
    for (int i = threadIdx.x; i < F; i += 256) {
        dq[i] = i < m ? l_d64[(int64_t)q * F + i] : __builtin_inf();
        mind[i] = __builtin_inf();
        picked[i] = 0;
    }
    // the padded tail of the outputs
    for (int t = npick + (int)threadIdx.x; t < k; t += 256) {
        out_labels[o0 + t] = -1;
        out_dist[o0 + t] = __builtin_inff();
        out_d64[o0 + t] = __builtin_inf();
        out_rank[o0 + t] = -1;
        out_obj[o0 + t] = __builtin_inf();
    }
    if (threadIdx.x == 0) out_counts[q] = npick;
    __syncthreads();

    for (int step = 0; step < npick; ++step) {
        // (a) the pick: position 0 first, then the block-wide argmin of the objective over the unpicked candidates
        int32_t s = 0;
        double so = lambda * dq[0];
        if (step > 0) {
            double bo = __builtin_inf();
            int32_t bi = kMmrNone;
            for (int i = threadIdx.x; i < m; i += 256) {
                if (picked[i]) continue;
                const double rel = lambda * dq[i];
                const double div = one_minus_lambda * mind[i];
                const double o = rel - div;
                if (mmr_better(o, i, bo, bi)) {
                    bo = o;
                    bi = i;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double oo = __shfl_xor(bo, off);
                const int32_t oi = __shfl_xor(bi, off);
                if (mmr_better(oo, oi, bo, bi)) {
                    bo = oo;
                    bi = oi;
                }
            }
            if (lane == 0) {
                wbest_o[wave] = bo;
                wbest_i[wave] = bi;
            }
            __syncthreads();
            so = wbest_o[0];
            s = wbest_i[0];
#pragma unroll
            for (int w = 1; w < 4; ++w)
                if (mmr_better(wbest_o[w], wbest_i[w], so, s)) {
                    so = wbest_o[w];
                    s = wbest_i[w];
                }
            if (s == kMmrNone) break;  // (block-uniform; cannot happen while step < min(k, m))
        }
        // (b) the step's outputs: the candidate list's own bits
        const int64_t label = lab[s];
        if (threadIdx.x == 0) {
            out_labels[o0 + step] = label;
            out_dist[o0 + step] = l_dist[(int64_t)q * F + s];
            out_d64[o0 + step] = dq[s];
            out_rank[o0 + step] = s;
            out_obj[o0 + step] = so;
            picked[s] = 1;
        }
        if (step + 1 == npick) break;  // nobody reads mind again
        // (c) row c_s as the query of the next distances: fp64 image and, for cosine, the norm term of the query prep
        const int64_t ls = label >= 0 ? label : 0;  // (a valid entry of the list never holds a negative label)
        const float* row = X + (ls >> 4) * (int64_t)(kPanelRows * ld) + (ls & 15) * 16;
        double nrm2 = 0.0;
        for (int c = threadIdx.x; c < ld; c += 256) {
            const float v = c < dim ? row[(int64_t)(c >> 4) * kGroupFloats + (c & 15)] : 0.f;
            qs[c] = (double)v;
            nrm2 = __builtin_fma((double)v, (double)v, nrm2);
        }
        double qinv = 0.0;
        if (SPACE == kSpaceCosine) {
            nrm2 = query_norm_wave_sum(nrm2);
            if (lane == 0) red[wave] = nrm2;
        }
        __syncthreads();  // qs, red and picked[s] are written; wbest_* are read
        if (SPACE == kSpaceCosine) qinv = query_aux_from_sums(red, kSpaceCosine);
        // (d) D(s, i) for every candidate, 16 per wave and iteration; mind lowered
        for (int j0 = wave * 16; j0 < m; j0 += 64) {
            const int j = j0 + r;
            const bool have = j < m;
            const int64_t lj = have ? lab[j] : -1;
            const int64_t rr = lj >= 0 ? lj : ls;  // keep the address valid
            const float* base[1] = {X + (rr >> 4) * (int64_t)(kPanelRows * ld) + (rr & 15) * 16 + g * 4};
            double acc[1][1], nx[1];
            accumulate_rows<SPACE, 1, 1, 8>(base, qs, ld, g, acc, nx);
            const double d = finish_distance<SPACE>(acc[0][0], nx[0], qinv);
            if (have && lane < 16 && d < mind[j]) mind[j] = d;
        }
        __syncthreads();  // mind is complete; qs and red may be overwritten
    }
}

size_t mmr_select_lds(int32_t ld, int32_t fetch_k) {
    return (size_t)ld * sizeof(double) + (size_t)fetch_k * (2 * sizeof(double) + sizeof(int32_t));
}

hipError_t launch_mmr_select(const float* X, int32_t dim, int32_t ld, int32_t space, const int64_t* l_lab, const float* l_dist,
                             const double* l_d64, const int32_t* l_cnt, int32_t nq, int32_t fetch_k, int32_t k, double lambda,
                             double one_minus_lambda, int64_t* out_labels, float* out_dist, int32_t* out_counts,
                             double* out_d64, int32_t* out_rank, double* out_obj, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    const size_t lds = mmr_select_lds(ld, fetch_k);
    if (lds > 64 * 1024) return hipErrorInvalidValue;  // (the entry point refuses such a call before anything is launched)
    return with_space(space, [&](auto sp) {
        constexpr auto kern = mmr_select_kernel<decltype(sp)::value>;
        if (hipError_t e = ensure_instance_lds<kern>(lds, 64 * 1024); e != hipSuccess) return e;
        kern<<<nq, 256, lds, s>>>(X, dim, ld, l_lab, l_dist, l_d64, l_cnt, fetch_k, k, lambda, one_minus_lambda, out_labels,
                                  out_dist, out_counts, out_d64, out_rank, out_obj);
        return hipGetLastError();
    });
}

}  // namespace mlvdb
