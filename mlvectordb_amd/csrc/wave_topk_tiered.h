// Wave-level sorted selection list with a tier in front of the value: lane i of a 64-lane wavefront holds the i-th best
// (tier, value, label) entry seen so far, ordered ascending by tier, then value, then label -- the ranking of
// include/mlvdb_examples.h.  WaveTopK (wave_topk.h) with one more key word: the same insertion, the same rules -- every
// operation is executed by the full wavefront, and the cross-lane moves are lane_read / lane_shr1 (__shfl-based: the comment
// in wave_topk.h says why nothing faster-looking is used).  A partial entry travels as a TopEntry with the tier in `pad`.
#pragma once
#include "wave_topk.h"

namespace mlvdb {

constexpr int32_t kNoTier = 0x7fffffff;  // sorts after every real tier; the padding of out_tier

__device__ __forceinline__ bool tiered_less(int32_t at, double ad, int32_t al, int32_t bt, double bd, int32_t bl) {
    return at < bt || (at == bt && entry_less(ad, al, bd, bl));
}

struct WaveTopKTiered {
    double d;  // this lane's entry
    int32_t t, l;
    double kth_d;  // wave-uniform copy of entry k-1 (admission threshold)
    int32_t kth_t, kth_l;

    __device__ __forceinline__ void init() {
        d = kth_d = __builtin_inf();
        t = kth_t = kNoTier;
        l = kth_l = kNoLabel;
    }

    // Offer one candidate per lane (lanes with want == false offer nothing; a NaN value must not be offered).  k in 1..64.
    __device__ __forceinline__ void offer(bool want, int32_t ct, double cd, int32_t cl, int k, int lane) {
        unsigned long long m = __ballot(want && tiered_less(ct, cd, cl, kth_t, kth_d, kth_l));
        while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t vt = lane_read(ct, src);
            const double vd = lane_read(cd, src);
            const int32_t vl = lane_read(cl, src);
            if (!tiered_less(vt, vd, vl, kth_t, kth_d, kth_l)) continue;  // threshold moved since the ballot
            const int pos = __popcll(__ballot(tiered_less(t, d, l, vt, vd, vl)));
            const int32_t up_t = lane_shr1(t);
            const double up_d = lane_shr1(d);
            const int32_t up_l = lane_shr1(l);
            if (lane > pos) {
                t = up_t;
                d = up_d;
                l = up_l;
            } else if (lane == pos) {
                t = vt;
                d = vd;
                l = vl;
            }
            kth_t = lane_read(t, k - 1);
            kth_d = lane_read(d, k - 1);
            kth_l = lane_read(l, k - 1);
        }
    }

    __device__ __forceinline__ void offer(bool want, const TopEntry& e, int k, int lane) { offer(want, e.pad, e.d, e.l, k, lane); }

    __device__ __forceinline__ TopEntry entry() const {
        TopEntry e;
        e.d = d;
        e.l = l;
        e.pad = t;
        return e;
    }
};

}  // namespace mlvdb
