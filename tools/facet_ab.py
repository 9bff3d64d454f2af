#!/usr/bin/env python3
"""Value facets of one int64 column over N rows (default 10M x 4 floats), at several cardinalities and one skewed column
(90 % of the rows on one value, the rest unique), without a filter and with a one-column filter ({"sel": {"$lt": 500}},
half the rows).  Per column, the p50 over --iters calls after warm-up of
  facet_values     eng.facet_values(attr, max_values[, where]): one pass, the program evaluated in the kernel
  where_count      eng.where_count(where): the pass the facet kernel extends (filtered runs only)
  host             eng.get_attr of the whole column + np.unique: what a caller had to do before (unfiltered, ignores tombstones)
and whether the facet answer equals np.unique over the same rows.  Every timed call ends in a stream synchronise inside the
library, so the host clock around it is the call's time; the kernels' own times: run this under
`rocprofv3 --kernel-trace --stats` (facet_values_kernel, facet_collect_kernel, where_eval_kernel in the stats).  A 32-edge
histogram of the same column is timed last."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--cardinalities", default="2,100,10000,1000000")
args = ap.parse_args()
N = args.rows
SCHEMA = {"facet": "int", "sel": "int"}


def p50(fn, iters):
    for _ in range(3):
        fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


rng = np.random.default_rng(0)
eng = HipScanEngine(4, "l2", device=0, capacity_hint=N)
chunk = 1 << 20
for first in range(0, N, chunk):
    eng.append(np.ones((min(chunk, N - first), 4), dtype=np.float32))
sel = np.arange(N, dtype=np.int64) % 1000
eng.define_attr(0, "int64")
eng.define_attr(1, "int64")
eng.set_attr(1, 0, sel)
prog = W.compile_where({"sel": {"$lt": 500}}, SCHEMA)
half = sel < 500
print(f"{N} rows, one int64 column, p50 of {args.iters} calls (ms)", flush=True)
t_count = p50(lambda: eng.where_count(prog), args.iters)
print(f"where_count of the filter alone: {t_count:.3f}", flush=True)
columns = [(f"{c} values", rng.integers(0, int(c), N).astype(np.int64)) for c in args.cardinalities.split(",")]
skew = 10_000_000 + np.arange(N, dtype=np.int64)
skew[rng.random(N) < 0.9] = 42
columns.append(("skewed", skew))
for name, col in columns:
    eng.set_attr(0, 0, col)
    max_values = 1 << 20
    t_all = p50(lambda: eng.facet_values(0, max_values), args.iters)
    t_half = p50(lambda: eng.facet_values(0, max_values, where=prog), args.iters)
    t_host = p50(lambda: np.unique(eng.get_attr(0, 0, N), return_counts=True), max(3, args.iters // 10))
    values, counts, matched, absent = eng.facet_values(0, max_values, where=prog)
    wv, wc = np.unique(col[half], return_counts=True)
    same = bool(np.array_equal(values, wv) and np.array_equal(counts, wc) and matched == int(half.sum()))
    print(f"{name:>16}: facet_values {t_all:.3f}  with filter {t_half:.3f} (where_count {t_count:.3f})  "
          f"host get_attr + np.unique {t_host:.1f}  == np.unique: {same}", flush=True)
eng.set_attr(0, 0, columns[2][1] if len(columns) > 2 else columns[0][1])
edges = np.linspace(0, 10_000, 32).astype(np.int64)
t_bins = p50(lambda: eng.facet_bins(0, edges), args.iters)
t_bins_half = p50(lambda: eng.facet_bins(0, edges, where=prog), args.iters)
print(f"32-edge histogram: facet_bins {t_bins:.3f}  with filter {t_bins_half:.3f}", flush=True)
eng.close()
