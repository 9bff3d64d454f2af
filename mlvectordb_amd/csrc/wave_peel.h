// The wave peel of the counting kernels (kernels_facet.hip, kernels_order.hip): lanes of a wave that add under the same key
// are counted by one add.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"

namespace mlvdb {

// Wave peel: the lanes that hold the first active lane's key are counted by one add of their popcount, for at most
// kFacetPeelRounds leading keys; a round that found its key on a single lane ends the peel (a column of many values: the
// lanes left add one each).  A bool column is done in two rounds, six genres in six, and 64 different values cost one round.
// Every lane of the wave must call this (ballots); add(key, n) runs on one lane per key, all of them at one call site after
// the rounds (a lane leads at most once: its own key leaves with it).
template <class Add>
__device__ __forceinline__ void wave_peel_add(bool has, int64_t key, Add&& add) {
    const int lane = threadIdx.x & 63;
    uint32_t mine = 1;  // what this lane adds under its key, if it adds
    bool adds = false;
    for (int r = 0; r < kFacetPeelRounds; ++r) {
        const unsigned long long active = __ballot(has);
        if (!active) break;
        const int leader = __ffsll((long long)active) - 1;
        const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)key, leader);
        const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)key >> 32), leader);
        const int64_t lead = (int64_t)(((uint64_t)hi << 32) | lo);
        const bool same = has && key == lead;
        const int n = __popcll(__ballot(same));
        if (lane == leader) {
            mine = (uint32_t)n;
            adds = true;
        }
        has = has && !same;
        if (n == 1) break;
    }
    if (adds || has) add(key, mine);
}

// The same peel for a minimum (kernels_maxsim.hip): the lanes that hold the first active lane's key fold their values into
// one unsigned minimum, which the leading lane hands to put(key, minimum) -- one call per key instead of one per lane, by
// the rounds and the early end of wave_peel_add.  Only lanes below WIDTH (a power of two) may have `has` set: the fold is a
// butterfly over xor 1 .. WIDTH / 2, which stays inside those lanes.  Every lane of the wave must call this.
template <int WIDTH, class Put>
__device__ __forceinline__ void wave_peel_min(bool has, int32_t key, unsigned long long value, Put&& put) {
    const int lane = threadIdx.x & 63;
    unsigned long long mine = value;  // what this lane puts under its key, if it puts
    bool puts = false;
    for (int r = 0; r < kFacetPeelRounds; ++r) {
        const unsigned long long active = __ballot(has);
        if (!active) break;
        const int leader = __ffsll((long long)active) - 1;
        const int32_t lead = __builtin_amdgcn_readlane(key, leader);
        const bool same = has && key == lead;
        const int n = __popcll(__ballot(same));
        if (n > 1) {
            unsigned long long m = same ? value : ~0ull;
#pragma unroll
            for (int x = 1; x < WIDTH; x <<= 1) {
                const unsigned long long o = (unsigned long long)__shfl_xor((long long)m, x);
                m = o < m ? o : m;
            }
            if (lane == leader) mine = m;
        }
        if (lane == leader) puts = true;
        has = has && !same;
        if (n == 1) break;
    }
    if (puts || has) put(key, mine);
}

}  // namespace mlvdb
