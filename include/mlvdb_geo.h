/*
 * mlvdb_geo.h -- geo attribute columns: one location per row, filtered by radius or box and ranked by distance on the
 * device (companion of mlvdb_where.h and mlvdb_order.h; the ABI version of mlvdb_hip.h is unchanged).
 *
 * Column type MLVDB_ATTR_GEO.  A value is one int64,
 *     (lat_e7 << 32) | (uint32)lon_e7      lat_e7, lon_e7: int32 counts of 1e-7 degree (about 1.1 cm),
 *                                          lat_e7 in [-900000000, 900000000], lon_e7 in [-1800000000, 1800000000]
 *     INT64_MIN                            the row has no location (absent; it decodes to lat_e7 = INT32_MIN: no latitude)
 * and the storage is that of an MLVDB_ATTR_INT64 column on every path: regrowth, compaction, reset, mlvdb_attr_set / _get,
 * mlvdb_attr_set_at and ASSIGN in mlvdb_attr_update_where (ADD is refused).  Every entry that writes values checks the two
 * halves of every non-absent value against the ranges above on the host: a bad one is MLVDB_ERR_INVALID_ARG and nothing is
 * launched.  Entries that need an int64 or float64 value column (distinct, grouped, maxsim `by`, mlvdb_where_ordered,
 * mlvdb_facet_values, mlvdb_facet_bins) refuse a geo column.
 *
 * Predicate ops (valid on geo columns only; on a geo column only these two and EXISTS are valid; an absent value fails both):
 *   GEO_BOX      a = the packed south-west corner, b = the packed north-east corner (both valid points, lat_sw <= lat_ne).
 *                Inclusive, in integers: lat_sw <= lat <= lat_ne, and lon_sw <= lon <= lon_ne when lon_sw <= lon_ne;
 *                otherwise the box crosses the antimeridian and the test is lon >= lon_sw || lon <= lon_ne.
 *   GEO_RADIUS   a = the packed centre, b = the bits of a double, the threshold sin^2(r / 2R) of a radius of r metres,
 *                in [0, 1]: the caller computes it, clamped to 1 so that r >= pi R matches every row that holds a point
 *                (r finite and >= 0; a threshold outside [0, 1] or NaN is refused).  A row matches when hav <= threshold.
 *
 * Distance (every use follows this; all arithmetic in fp64 without contraction, differences taken in integers first):
 *     dphi = (lat - lat_c) * K               K = pi / (180 * 1e7)
 *     dlam = wrap(lon - lon_c) * K           wrap maps the integer difference into [-180, 180) degrees
 *     hav  = sin^2(dphi / 2) + cos(lat_c * K) * cos(lat * K) * sin^2(dlam / 2)
 *     d    = 2 R asin(sqrt(min(hav, 1)))     metres, R = MLVDB_GEO_EARTH_RADIUS_M
 * A row at the centre's own coordinates has hav == 0 exactly, so a radius of 0 matches exactly those rows.  The device
 * evaluates hav by one function in every kernel, so a row's hav has the same bits in every launch.
 */
#ifndef MLVDB_GEO_H
#define MLVDB_GEO_H

#include <stdint.h>

#include "mlvdb_order.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLVDB_ATTR_GEO 5 /* accepted by mlvdb_attr_define */

#define MLVDB_WHERE_GEO_BOX 16
#define MLVDB_WHERE_GEO_RADIUS 17

#define MLVDB_GEO_LAT_MAX_E7 900000000
#define MLVDB_GEO_LON_MAX_E7 1800000000
#define MLVDB_GEO_EARTH_RADIUS_M 6371008.8

/* Ranks [offset, offset + limit) of the candidates -- the live rows (those `where` matches, when given) that hold a point
 * in geo column `attr` -- by ascending hav from `center` (a packed point), rows of equal hav by ascending label: the
 * contract of mlvdb_where_ordered, with *matched / *absent as there.  out_labels, out_points (the stored values bit for
 * bit) and out_dist_m (d as defined above) hold `limit` entries each, *n_out of them written.  A maximum distance is a
 * GEO_RADIUS op in `where`.  offset >= 0, limit >= 1, offset + limit <= MLVDB_ORDER_MAX_ROWS; no pointer but `where` may
 * be null; everything is validated on the host before a launch, and an index without rows answers zeros. */
int mlvdb_geo_nearest(mlvdb_index* h, int32_t attr, int64_t center, const mlvdb_where* where, int64_t offset,
                      int64_t limit, int64_t* out_labels, int64_t* out_points, double* out_dist_m, int64_t* n_out,
                      int64_t* matched, int64_t* absent);

#ifdef __cplusplus
}
#endif

#endif /* MLVDB_GEO_H */
