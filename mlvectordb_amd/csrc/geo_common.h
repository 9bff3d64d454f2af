// The distance of geo columns (include/mlvdb_geo.h): one definition of hav for the predicate ops (where_common.h) and for
// every pass of mlvdb_geo_nearest (kernels_order.hip).  The nearest chain selects by digits of hav's bits in one launch
// and collects by them in another, so a row's hav must have the same bits in every launch: the function is inlined
// everywhere from this one text and FP contraction is off inside it (no fma may be formed in one kernel and not in another).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"

namespace mlvdb {

constexpr double kGeoRadPerE7 = 3.14159265358979323846 / (180.0 * 1e7);  // K of mlvdb_geo.h
constexpr int64_t kGeoTurnE7 = 3600000000ll;                             // 360 degrees

__host__ __device__ inline int32_t geo_lat(int64_t p) { return (int32_t)(p >> 32); }
__host__ __device__ inline int32_t geo_lon(int64_t p) { return (int32_t)(uint32_t)p; }

// a packed point whose halves are inside the ranges (INT64_MIN, absent, is none)
inline bool geo_valid(int64_t p) {
    const int64_t lat = geo_lat(p), lon = geo_lon(p);
    return lat >= -MLVDB_GEO_LAT_MAX_E7 && lat <= MLVDB_GEO_LAT_MAX_E7 && lon >= -MLVDB_GEO_LON_MAX_E7 &&
           lon <= MLVDB_GEO_LON_MAX_E7;
}

__device__ __forceinline__ double geo_cos_lat(int32_t lat) {
#pragma clang fp contract(off)
    return cos((double)lat * kGeoRadPerE7);
}

// hav of the present point `p` from the centre (lat_c, lon_c), cos_c = geo_cos_lat(lat_c)
__device__ __forceinline__ double geo_hav(int64_t p, int32_t lat_c, int32_t lon_c, double cos_c) {
#pragma clang fp contract(off)
    const int32_t lat = geo_lat(p);
    const int64_t dlat = (int64_t)lat - lat_c;
    int64_t dlon = (int64_t)geo_lon(p) - lon_c;  // in (-360, 360) degrees -> [-180, 180)
    if (dlon >= kGeoTurnE7 / 2) dlon -= kGeoTurnE7;
    if (dlon < -kGeoTurnE7 / 2) dlon += kGeoTurnE7;
    const double dphi = (double)dlat * kGeoRadPerE7, dlam = (double)dlon * kGeoRadPerE7;
    const double sp = sin(dphi * 0.5), sl = sin(dlam * 0.5);
    const double cc = cos_c * geo_cos_lat(lat);
    const double sp2 = sp * sp, sl2 = sl * sl;
    const double t = cc * sl2;
    return sp2 + t;
}

// metres
__device__ __forceinline__ double geo_dist_m(double hav) {
#pragma clang fp contract(off)
    return 2.0 * MLVDB_GEO_EARTH_RADIUS_M * asin(sqrt(hav < 1.0 ? hav : 1.0));
}

}  // namespace mlvdb
