// Hybrid search (include/mlvdb_hybrid.h): a query's ranked dense list D and sparse list S joined by label into the union C,
// the component each member lacks computed for it, and the fused top-k.  DESIGN.md 11.14.
//
// hybrid_union_kernel   one block per query: C = D's entries in order, then S's entries that D does not hold, in order; each
//                       member's position in both lists, and two label lists for the completion: need_d (members without a
//                       distance yet, -1 elsewhere) for launch_pair_distances and need_s (members without a score yet) for
// sparse_pair_score_kernel, the gathered scorer: one block per query, its terms, weights and the scan's bitmap in LDS, 16
//                       lanes per (query, member) pair, four pairs per wave step.  It repeats the scan's arithmetic for the
//                       pair (kernels_sparse.hip): lane j takes elements j, j + 16, ... in ascending order, a shared term is
//                       fma((double)w_row, (double)w_query, acc) from +0.0, the 16 sums are folded by row16_sum.  A term the
//                       query lacks adds nothing here and fma(w, 0, acc) == acc there, so the 64 bits are the scan's.
// hybrid_fuse_kernel    one block per query: components (the lists' own values where a list holds the member), min / max for
//                       RELATIVE, the fused score, and the exact top-k by counting ranks over (fused descending, label
//                       ascending) -- every member counts the members that precede it and writes itself at that position.
#include "internal.h"
#include "sparse_dpp.h"

namespace mlvdb {

__global__ __launch_bounds__(256) void hybrid_union_kernel(const int64_t* __restrict__ d_lab, const int32_t* __restrict__ d_cnt,
                                                           int32_t fd, const int64_t* __restrict__ s_lab,
                                                           const int32_t* __restrict__ s_cnt, int32_t fs,
                                                           int64_t* __restrict__ u_lab, int32_t* __restrict__ u_rd,
                                                           int32_t* __restrict__ u_rs, int64_t* __restrict__ need_d,
                                                           int64_t* __restrict__ need_s, int32_t* __restrict__ u_cnt) {
    __shared__ int64_t sS[kWave];
    __shared__ int32_t sInD[kWave];  // the S entry's position in D, -1: D does not hold it
    __shared__ int32_t sTotal;
    const int q = blockIdx.x;
    const int m = fd + fs;
    const int nd = min(d_cnt[q], fd), ns = min(s_cnt[q], fs);
    const int64_t* dl = d_lab + (int64_t)q * fd;
    const int64_t ub = (int64_t)q * m;
    if (threadIdx.x < kWave) {
        sS[threadIdx.x] = (int)threadIdx.x < ns ? s_lab[(int64_t)q * fs + threadIdx.x] : -1;
        sInD[threadIdx.x] = -1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nd; i += 256) {
        const int64_t lab = dl[i];
        int rs = -1;
        for (int j = 0; j < ns; ++j)
            if (sS[j] == lab) rs = j;  // (labels are distinct within a list: at most one j, and one i per j)
        if (rs >= 0) sInD[rs] = i;
        u_lab[ub + i] = lab;
        u_rd[ub + i] = i;
        u_rs[ub + i] = rs;
        need_d[ub + i] = -1;
        need_s[ub + i] = rs < 0 ? lab : -1;
    }
    __syncthreads();
    int total = nd;
    if (threadIdx.x < kWave) {  // wave 0: S's own entries behind D's, order kept
        const int j = threadIdx.x;
        const bool fresh = j < ns && sInD[j] < 0;
        const unsigned long long b = __ballot(fresh);
        const int at = nd + __popcll(b & ((1ull << j) - 1ull));
        if (fresh) {
            u_lab[ub + at] = sS[j];
            u_rd[ub + at] = -1;
            u_rs[ub + at] = j;
            need_d[ub + at] = sS[j];
            need_s[ub + at] = -1;
        }
        total = nd + __popcll(b);
        if (j == 0) {
            u_cnt[q] = total;
            sTotal = total;
        }
    }
    __syncthreads();
    total = sTotal;
    for (int i = total + threadIdx.x; i < m; i += 256) {
        u_lab[ub + i] = -1;
        u_rd[ub + i] = -1;
        u_rs[ub + i] = -1;
        need_d[ub + i] = -1;
        need_s[ub + i] = -1;
    }
}

__global__ __launch_bounds__(256) void sparse_pair_score_kernel(const int64_t* __restrict__ slots, const int64_t* __restrict__ pool,
                                                                int64_t total, const int64_t* __restrict__ q_off,
                                                                const int32_t* __restrict__ q_terms,
                                                                const float* __restrict__ q_weights,
                                                                const int64_t* __restrict__ labels, const int32_t* __restrict__ cnt,
                                                                int32_t m, double* __restrict__ out) {
    __shared__ int32_t sT[kSparseMaxUnion];
    __shared__ float sW[kSparseMaxUnion];
    __shared__ unsigned int sB[kSparseBitmapWords];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int g = lane >> 4;
    const int j = lane & 15;
    const int q = blockIdx.x;
    const int64_t t0 = q_off[q];
    const int nt = min((int)(q_off[q + 1] - t0), kSparseMaxUnion);
    for (int c = threadIdx.x; c < kSparseBitmapWords; c += 256) sB[c] = 0u;
    for (int c = threadIdx.x; c < nt; c += 256) {
        sT[c] = q_terms[t0 + c];
        sW[c] = q_weights[t0 + c];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nt; c += 256) {
        const unsigned int t = (unsigned int)sT[c] & (kSparseBitmapBits - 1);
        atomicOr(&sB[t >> 5], 1u << (t & 31));
    }
    __syncthreads();
    const int n = min(cnt[q], m);
    // p0 is uniform over the block: every lane of a wave runs the same steps (the fold needs all of them)
    for (int p0 = 0; p0 < n; p0 += 16) {
        const int p = p0 + wave * 4 + g;
        const int64_t lab = p < n ? labels[(int64_t)q * m + p] : -1;
        const int64_t slot = lab >= 0 && lab < total ? slots[lab] : INT64_MIN;  // -1: padding, or a member S holds already
        const int len = slot != INT64_MIN ? (int)(slot & 0xff) : 0;
        const int64_t* src = pool + (slot >> 8);  // (never read when len == 0)
        double acc = 0.0;
        for (int e = j; e < len; e += 16) {  // in ascending element order: the order of a lane's additions is the scan's
            const int64_t el = src[e];
            const int32_t term = (int32_t)(el >> 32);
            const unsigned int t = (unsigned int)term & (kSparseBitmapBits - 1);
            if (!((sB[t >> 5] >> (t & 31)) & 1u)) continue;
            int lo = 0, hi = nt;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sT[mid] < term) lo = mid + 1; else hi = mid;
            }
            if (lo >= nt || sT[lo] != term) continue;
            const double w = (double)__int_as_float((int32_t)(el & 0xffffffffll));
            acc = fma(w, (double)sW[lo], acc);
        }
        const double score = row16_sum(acc);
        if (j == 0 && p < n) out[(int64_t)q * m + p] = score;
    }
}

// the larger / smaller of a block's values of v, on every thread (sred: 4 doubles)
template <bool MAX>
__device__ __forceinline__ double block_extreme(double v, double* sred) {
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off);
        v = MAX ? (o > v ? o : v) : (o < v ? o : v);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sred[0];
    for (int w = 1; w < 4; ++w) r = MAX ? (sred[w] > r ? sred[w] : r) : (sred[w] < r ? sred[w] : r);
    return r;
}

__global__ __launch_bounds__(256) void hybrid_fuse_kernel(const int64_t* __restrict__ u_lab, const int32_t* __restrict__ u_rd,
                                                          const int32_t* __restrict__ u_rs, const int32_t* __restrict__ u_cnt,
                                                          int32_t m, const double* __restrict__ d_d64, int32_t fd,
                                                          const double* __restrict__ s_d64, int32_t fs,
                                                          const double* __restrict__ comp_d, const double* __restrict__ comp_s,
                                                          int32_t method, double w_dense, double w_sparse, double rrf_c,
                                                          int32_t k, int64_t* __restrict__ out_labels,
                                                          double* __restrict__ out_fused, int32_t* __restrict__ out_counts,
                                                          double* __restrict__ out_d64, double* __restrict__ out_s64,
                                                          int32_t* __restrict__ out_rd, int32_t* __restrict__ out_rs) {
    __shared__ double sF[kHybridMaxUnion], sD[kHybridMaxUnion], sS[kHybridMaxUnion];
    __shared__ int32_t sL[kHybridMaxUnion], sRd[kHybridMaxUnion], sRs[kHybridMaxUnion];
    __shared__ double sred[4];
    const int q = blockIdx.x;
    const int n = min(u_cnt[q], min(m, kHybridMaxUnion));
    const int64_t ub = (int64_t)q * m;
    const bool complete = comp_d != nullptr;  // (an RRF call that wants no component runs without the completion launches)
    double dmin = __builtin_inf(), dmax = -__builtin_inf(), smin = __builtin_inf(), smax = -__builtin_inf();
    for (int c = threadIdx.x; c < n; c += 256) {
        const int rd = u_rd[ub + c], rs = u_rs[ub + c];
        double dd = 0.0, ss = 0.0;
        if (rd >= 0) dd = d_d64[(int64_t)q * fd + rd];
        else if (complete) dd = comp_d[ub + c];
        if (rs >= 0) ss = s_d64[(int64_t)q * fs + rs];
        else if (complete) ss = comp_s[ub + c];
        sL[c] = (int32_t)u_lab[ub + c];
        sRd[c] = rd;
        sRs[c] = rs;
        sD[c] = dd;
        sS[c] = ss;
        dmin = dd < dmin ? dd : dmin;
        dmax = dd > dmax ? dd : dmax;
        smin = ss < smin ? ss : smin;
        smax = ss > smax ? ss : smax;
    }
    if (method == MLVDB_FUSE_RELATIVE) {  // (uniform)
        dmin = block_extreme<false>(dmin, sred);
        dmax = block_extreme<true>(dmax, sred);
        smin = block_extreme<false>(smin, sred);
        smax = block_extreme<true>(smax, sred);
    }
    for (int c = threadIdx.x; c < n; c += 256) {  // (each thread reads back what it wrote itself)
        const double dd = sD[c], ss = sS[c];
        double fused;
        if (method == MLVDB_FUSE_RRF) {
            const double td = sRd[c] >= 0 ? w_dense / (rrf_c + (double)(sRd[c] + 1)) : 0.0;
            const double ts = sRs[c] >= 0 ? w_sparse / (rrf_c + (double)(sRs[c] + 1)) : 0.0;
            fused = td + ts;
        } else if (method == MLVDB_FUSE_LINEAR) {
            const double a = w_sparse * ss;
            const double b = w_dense * dd;
            fused = a - b;
        } else {
            const double nd = dmax == dmin ? 0.0 : (dmax - dd) / (dmax - dmin);
            const double ns = smax == smin ? 0.0 : (ss - smin) / (smax - smin);
            const double a = w_dense * nd;
            const double b = w_sparse * ns;
            fused = a + b;
        }
        sF[c] = fused;
    }
    __syncthreads();
    const int64_t ob = (int64_t)q * k;
    for (int c = threadIdx.x; c < n; c += 256) {
        const double f = sF[c];
        const int32_t l = sL[c];
        int before = 0;
        for (int o = 0; o < n; ++o) {  // (the same LDS address on every lane: a broadcast read)
            const double fo = sF[o];
            before += (fo > f || (fo == f && sL[o] < l)) ? 1 : 0;
        }
        if (before < k) {
            out_labels[ob + before] = l;
            out_fused[ob + before] = f;
            if (out_d64) out_d64[ob + before] = sD[c];
            if (out_s64) out_s64[ob + before] = sS[c];
            if (out_rd) out_rd[ob + before] = sRd[c];
            if (out_rs) out_rs[ob + before] = sRs[c];
        }
    }
    for (int i = n + threadIdx.x; i < k; i += 256) {
        out_labels[ob + i] = -1;
        out_fused[ob + i] = -__builtin_inf();
        if (out_d64) out_d64[ob + i] = __builtin_inf();
        if (out_s64) out_s64[ob + i] = -__builtin_inf();
        if (out_rd) out_rd[ob + i] = -1;
        if (out_rs) out_rs[ob + i] = -1;
    }
    if (threadIdx.x == 0) out_counts[q] = n < k ? n : k;
}

hipError_t launch_hybrid_union(const int64_t* d_lab, const int32_t* d_cnt, int32_t fd, const int64_t* s_lab,
                               const int32_t* s_cnt, int32_t fs, int32_t nq, int64_t* u_lab, int32_t* u_rd, int32_t* u_rs,
                               int64_t* need_d, int64_t* need_s, int32_t* u_cnt, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    if (fd < 1 || fs < 1 || fs > kWave || fd + fs > kHybridMaxUnion) return hipErrorInvalidValue;
    hybrid_union_kernel<<<(unsigned)nq, 256, 0, s>>>(d_lab, d_cnt, fd, s_lab, s_cnt, fs, u_lab, u_rd, u_rs, need_d, need_s, u_cnt);
    return hipGetLastError();
}

hipError_t launch_sparse_pair_score(const int64_t* slots, const int64_t* pool, int64_t total, const int64_t* q_off,
                                    const int32_t* q_terms, const float* q_weights, const int64_t* labels, const int32_t* cnt,
                                    int32_t nq, int32_t m, double* out, hipStream_t s) {
    if (nq <= 0 || m <= 0) return hipSuccess;
    sparse_pair_score_kernel<<<(unsigned)nq, 256, 0, s>>>(slots, pool, total, q_off, q_terms, q_weights, labels, cnt, m, out);
    return hipGetLastError();
}

hipError_t launch_hybrid_fuse(const int64_t* u_lab, const int32_t* u_rd, const int32_t* u_rs, const int32_t* u_cnt, int32_t nq,
                              int32_t m, const double* d_d64, int32_t fd, const double* s_d64, int32_t fs, const double* comp_d,
                              const double* comp_s, int32_t method, double w_dense, double w_sparse, double rrf_c, int32_t k,
                              int64_t* out_labels, double* out_fused, int32_t* out_counts, double* out_d64, double* out_s64,
                              int32_t* out_rd, int32_t* out_rs, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    if (m < 1 || m > kHybridMaxUnion || k < 1 || (comp_d == nullptr) != (comp_s == nullptr)) return hipErrorInvalidValue;
    hybrid_fuse_kernel<<<(unsigned)nq, 256, 0, s>>>(u_lab, u_rd, u_rs, u_cnt, m, d_d64, fd, s_d64, fs, comp_d, comp_s, method,
                                                   w_dense, w_sparse, rrf_c, k, out_labels, out_fused, out_counts, out_d64,
                                                   out_s64, out_rd, out_rs);
    return hipGetLastError();
}

}  // namespace mlvdb
