// The host-built code table of the grouped and late-interaction stages (api.hip: grouped_members, maxsim_impl): group codes
// placed by facet_hash with linear probing, INT64_MIN = empty, at most half full.  A row's slot is found by probing, never
// inserted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"

namespace mlvdb {

// the slot of code v, or -1 when no query picked it (v != INT64_MIN; the table is at most half full: the probe ends)
__device__ __forceinline__ int32_t grouped_lookup(const long long* __restrict__ keys, uint64_t mask, int64_t v) {
    uint64_t s = facet_hash(v) & mask;
    for (;;) {
        const long long key = keys[s];
        if (key == v) return (int32_t)s;
        if (key == INT64_MIN) return -1;
        s = (s + 1) & mask;
    }
}

// the slot of row i's group when the row is live (finite norm: not tombstoned, allowed by the call's mask) and holds a
// picked code; the column is read for live rows only
__device__ __forceinline__ int32_t grouped_row_slot(const float* __restrict__ rn, const int64_t* __restrict__ col, int64_t i,
                                                    int64_t total, const long long* __restrict__ keys, uint64_t mask) {
    if (i >= total) return -1;
    const float norm = rn[i];
    if (!(norm == norm)) return -1;
    const int64_t v = col[i];
    return v == INT64_MIN ? -1 : grouped_lookup(keys, mask, v);
}

}  // namespace mlvdb
