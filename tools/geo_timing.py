"""Times the geo entries beside their scalar siblings on one index: where_count with a 25 km radius
beside an int64 $gte/$lte pair, and geo_nearest(limit=20) beside where_ordered(limit=20) on a float column.  Every call
ends in a device synchronise inside the library, so a host clock around it is the call's time; each is warmed up, repeated
and reported as its median and spread.  usage: python tools/geo_timing.py [--rows 4000000] [--repeats 30]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

SCHEMA = {"loc": "geo", "year": "int", "price": "float"}
CENTRE = (48.2082, 16.3738)


def timed(call, repeats):
    for _ in range(3):
        call()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    n = args.rows
    # half of the points in a cluster of 0.2 degrees around the centre, the rest uniform on the sphere; 10 % absent
    near = rng.random(n) < 0.5
    lat = np.where(near, CENTRE[0] + 0.2 * rng.standard_normal(n), np.degrees(np.arcsin(rng.uniform(-1, 1, n))))
    lon = np.where(near, CENTRE[1] + 0.2 * rng.standard_normal(n), rng.uniform(-180, 180, n))
    loc = (np.rint(lat * 1e7).astype(np.int64) << 32) | (np.rint(lon * 1e7).astype(np.int64) & 0xFFFFFFFF)
    loc[rng.random(n) < 0.1] = W.INT64_ABSENT
    year = rng.integers(1900, 2030, n).astype(np.int64)
    price = rng.uniform(0, 1000, n)
    eng = HipScanEngine(4, "l2", device=0)
    eng.append(np.ones((n, 4), dtype=np.float32))
    for a, (kind, col) in enumerate((("geo", loc), ("int64", year), ("float64", price))):
        eng.define_attr(a, kind)
        eng.set_attr(a, 0, col)
    radius = W.compile_where({"loc": {"$geo_radius": {"center": CENTRE, "radius": 25_000}}}, SCHEMA)
    box = W.compile_where({"loc": {"$geo_box": {"sw": (48.0, 16.0), "ne": (48.4, 16.7)}}}, SCHEMA)
    span = W.compile_where({"year": {"$gte": 1990, "$lte": 2010}}, SCHEMA)
    centre = W.geo_pack(CENTRE)
    out = {"rows": n, "repeats": args.repeats,
           "matches": {"radius_25km": eng.where_count(radius), "box": eng.where_count(box), "year_span": eng.where_count(span)},
           "where_count_radius_25km": timed(lambda: eng.where_count(radius), args.repeats),
           "where_count_box": timed(lambda: eng.where_count(box), args.repeats),
           "where_count_int64_gte_lte": timed(lambda: eng.where_count(span), args.repeats),
           "geo_nearest_limit20": timed(lambda: eng.geo_nearest(0, centre, 20), args.repeats),
           "geo_nearest_limit20_where_radius": timed(lambda: eng.geo_nearest(0, centre, 20, where=radius), args.repeats),
           "where_ordered_float_limit20": timed(lambda: eng.where_ordered(2, 20), args.repeats)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
