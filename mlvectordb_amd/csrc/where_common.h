// The predicate program of a metadata filter evaluated on one row (include/mlvdb_where.h): shared by the single-program
// kernel (kernels_where.hip) and the multi-program one of per-query filters (kernels_where_each.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geo_common.h"
#include "internal.h"

namespace mlvdb {

// `prog` (validated on the host, usually staged in LDS) on one row; the boolean stack is one 32-bit register (bit 0 = top).
// Every op is uniform over the wave, so the branches never diverge; what differs per lane is only the value `load(op)`
// returns for the op's column (INT64_MIN / NaN bits when the row has none).  The column type is the low byte of op.type.
template <class Load>
__device__ __forceinline__ bool where_eval_with(const WhereOp* prog, int32_t n_ops, const int64_t* __restrict__ set,
                                                Load&& load) {
    uint32_t st = 0;
    for (int p = 0; p < n_ops; ++p) {
        const WhereOp o = prog[p];
        if (o.op == MLVDB_WHERE_AND || o.op == MLVDB_WHERE_OR) {
            const uint32_t x = st & 1u, y = (st >> 1) & 1u;
            st = ((st >> 2) << 1) | (o.op == MLVDB_WHERE_AND ? (x & y) : (x | y));
            continue;
        }
        if (o.op == MLVDB_WHERE_NOT) {
            st ^= 1u;
            continue;
        }
        bool bit = true;  // MLVDB_WHERE_TRUE
        if (o.op != MLVDB_WHERE_TRUE) {
            const int64_t raw = load(o);
            if ((o.type & 0xff) == MLVDB_ATTR_INT64) {
                const bool have = raw != INT64_MIN;
                switch (o.op) {
                    case MLVDB_WHERE_EQ: bit = have && raw == o.a; break;
                    case MLVDB_WHERE_NE: bit = !(have && raw == o.a); break;
                    case MLVDB_WHERE_LT: bit = have && raw < o.a; break;
                    case MLVDB_WHERE_LE: bit = have && raw <= o.a; break;
                    case MLVDB_WHERE_GT: bit = have && raw > o.a; break;
                    case MLVDB_WHERE_GE: bit = have && raw >= o.a; break;
                    case MLVDB_WHERE_EXISTS: bit = have; break;
                    default: {  // MLVDB_WHERE_IN: binary search of set[a, a + b), sorted ascending
                        int64_t lo = o.a, hi = o.a + o.b;
                        while (lo < hi) {
                            const int64_t mid = lo + ((hi - lo) >> 1);
                            if (set[mid] < raw) lo = mid + 1; else hi = mid;
                        }
                        bit = have && lo < o.a + o.b && set[lo] == raw;
                    }
                }
            } else if ((o.type & 0xff) == MLVDB_ATTR_INT64_LIST) {
                // raw is the row's slot, (offset << 8) | len into the pool whose address the host put into o.b
                // (include/mlvdb_list.h); an absent slot reads as len 0.  The walks below diverge per lane (<= 255 steps).
                const bool have = raw != INT64_MIN;
                const int len = (int)(raw & 0xff);
                const int64_t* lp = reinterpret_cast<const int64_t*>(o.b) + (raw >> 8);
                if (o.op == MLVDB_WHERE_EXISTS) {
                    bit = have;
                } else if (o.op == MLVDB_WHERE_LEN) {
                    bit = have && len >= o.a && len <= o.b;
                } else if (o.op == MLVDB_WHERE_HAS) {  // binary search of the row's sorted list
                    int lo = 0, hi = len;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (lp[mid] < o.a) lo = mid + 1; else hi = mid;
                    }
                    bit = lo < len && lp[lo] == o.a;
                } else {  // HAS_ANY / HAS_ALL: every element looked up in set[s0, s0 + sn) (o.a = s0 << 32 | sn)
                    const int64_t s0 = o.a >> 32, sn = o.a & 0xffffffffll;
                    const bool all = o.op == MLVDB_WHERE_HAS_ALL;
                    int found = 0;
                    const int walk = (all && len < sn) ? 0 : len;  // a shorter list cannot hold them all
                    for (int j = 0; j < walk; ++j) {
                        const int64_t v = lp[j];
                        int64_t lo = s0, hi = s0 + sn;
                        while (lo < hi) {
                            const int64_t mid = lo + ((hi - lo) >> 1);
                            if (set[mid] < v) lo = mid + 1; else hi = mid;
                        }
                        if (lo < s0 + sn && set[lo] == v) {
                            ++found;
                            if (!all) break;
                        }
                    }
                    // (both sides strictly ascending under HAS_ALL: every set value is found at most once)
                    bit = all ? (have && found == sn) : found > 0;
                }
            } else if ((o.type & 0xff) == MLVDB_ATTR_GEO) {
                // raw is a packed point (include/mlvdb_geo.h); an absent row fails both ops, and computes nothing
                const bool have = raw != INT64_MIN;
                if (o.op == MLVDB_WHERE_EXISTS) {
                    bit = have;
                } else if (o.op == MLVDB_WHERE_GEO_BOX) {  // a = south-west, b = north-east; inclusive, in integers
                    const int32_t lat = geo_lat(raw), lon = geo_lon(raw), w = geo_lon(o.a), e = geo_lon(o.b);
                    const bool in_lon = w <= e ? (lon >= w && lon <= e) : (lon >= w || lon <= e);  // (else: across the antimeridian)
                    bit = have && lat >= geo_lat(o.a) && lat <= geo_lat(o.b) && in_lon;
                } else {  // GEO_RADIUS: a = the centre, b = the bits of sin^2(r / 2R)
                    const int32_t lat_c = geo_lat(o.a);
                    bit = have && geo_hav(raw, lat_c, geo_lon(o.a), geo_cos_lat(lat_c)) <= __longlong_as_double(o.b);
                }
            } else {  // float64: absent = NaN, so every ordered comparison of an absent value is false by itself
                const double v = __longlong_as_double(raw), a = __longlong_as_double(o.a);
                switch (o.op) {
                    case MLVDB_WHERE_EQ: bit = v == a; break;
                    case MLVDB_WHERE_NE: bit = !(v == a); break;
                    case MLVDB_WHERE_LT: bit = v < a; break;
                    case MLVDB_WHERE_LE: bit = v <= a; break;
                    case MLVDB_WHERE_GT: bit = v > a; break;
                    case MLVDB_WHERE_GE: bit = v >= a; break;
                    default: bit = v == v;  // MLVDB_WHERE_EXISTS
                }
            }
        }
        st = (st << 1) | (bit ? 1u : 0u);
    }
    return st & 1u;
}

// ... on row i of the ops' own columns (8 coalesced bytes per row and referenced op).  in == false: the row does not exist
// (nothing is loaded).
__device__ __forceinline__ bool where_eval_row(const WhereOp* prog, int32_t n_ops, const int64_t* __restrict__ set,
                                               int64_t i, bool in) {
    return where_eval_with(prog, n_ops, set,
                           [&](const WhereOp& o) { return in ? static_cast<const int64_t*>(o.col)[i] : INT64_MIN; });
}

}  // namespace mlvdb
