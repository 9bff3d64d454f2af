// WaveTopK (wave_topk.h) with one group code per entry: lane i of a 64-lane wavefront holds the i-th best
// (distance, label, group) seen so far, ordered by (distance, label), and NO TWO ENTRIES SHARE A GROUP -- each listed
// group is represented by the best of its rows offered so far.  All operations must be executed by the full wavefront.
#pragma once
#include "wave_topk.h"

namespace mlvdb {

constexpr int64_t kNoGroup = INT64_MIN;  // the absent sentinel of an int64 attribute column: never a listed entry's group

__device__ __forceinline__ int64_t lane_read(int64_t v, int src) { return (int64_t)__shfl((long long)v, src); }
__device__ __forceinline__ int64_t lane_shr1(int64_t v) { return (int64_t)__shfl_up((long long)v, 1); }

struct WaveTopKDistinct {
    double d;     // this lane's entry
    int32_t l;
    int64_t g;
    double kth_d;  // wave-uniform copy of entry k-1 (admission threshold)
    int32_t kth_l;

    __device__ __forceinline__ void init() {
        d = __builtin_inf();
        l = kNoLabel;
        g = kNoGroup;
        kth_d = __builtin_inf();
        kth_l = kNoLabel;
    }

    // Offer one candidate per lane (lanes with want == false offer nothing).  k in 1..64.
    // A candidate that does not beat entry k-1 is dropped whatever its group: a listed row of its group would sit at or
    // before k-1 and be the better one.  Entry k-1 only ever improves: an in-place replacement moves entries of
    // (pos, j] down by one and leaves every lane beyond j alone, so nothing returns from behind k-1.
    __device__ __forceinline__ void offer(bool want, double cd, int32_t cl, int64_t cg, int k, int lane) {
        unsigned long long m = __ballot(want && entry_less(cd, cl, kth_d, kth_l));
        while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const double vd = lane_read(cd, src);
            const int32_t vl = lane_read(cl, src);
            const int64_t vg = lane_read(cg, src);
            if (!entry_less(vd, vl, kth_d, kth_l)) continue;  // threshold moved since the ballot
            const unsigned long long same = __ballot(l != kNoLabel && g == vg);  // at most one lane
            const int pos = __popcll(__ballot(entry_less(d, l, vd, vl)));
            const int j = same ? __builtin_ctzll(same) : kWave;  // no listed row of the group: everything behind pos moves
            if (j < pos) continue;                               // the listed row of the group is the better one
            const double up_d = lane_shr1(d);
            const int32_t up_l = lane_shr1(l);
            const int64_t up_g = lane_shr1(g);
            if (lane > pos && lane <= j) {
                d = up_d;
                l = up_l;
                g = up_g;
            } else if (lane == pos) {
                d = vd;
                l = vl;
                g = vg;
            }
            kth_d = lane_read(d, k - 1);
            kth_l = lane_read(l, k - 1);
        }
    }
};

// 24-byte record of the per-block partial lists of the grouped scan
struct __attribute__((aligned(8))) DistinctEntry {
    double d;
    int64_t g;
    int32_t l;
    int32_t pad;
};

}  // namespace mlvdb
