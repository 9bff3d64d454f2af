#!/usr/bin/env python3
"""Statistics of one int64 and one float64 column over N rows (default 10M x 4 floats), ungrouped and grouped by an int64
column of several cardinalities, without a filter and with a one-column filter ({"sel": {"$lt": 500}}, half the rows).
Per case, the median and the spread (p10..p90) over --iters calls after warm-up of
  attr_stats     eng.attr_stats(attr, by, max_groups[, where]): one pass (int64) or two (float64), the program evaluated
                 in the kernels
  facet_values   eng.facet_values(by, max_groups[, where]): the same pass shape counting rows only -- the floor a grouped
                 call is measured against (grouped runs only)
  host           eng.get_attr of the column (and of the group column) + NumPy: what a caller had to do before (unfiltered,
                 ignores tombstones; a float sum by np.add.reduceat, whose bits depend on the order of the rows)
and whether the answer equals the model of tests/stats_helpers.py over the same rows.  Every timed call ends in a stream
synchronise inside the library, so the host clock around it is the call's time; the kernels' own times: run this under
`rocprofv3 --kernel-trace --stats` (stats_pass1_kernel, stats_pass2_kernel, stats_collect_kernel in the stats)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mlvectordb_amd import stats as host_stats  # noqa: E402
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402
from tests import stats_helpers as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--cardinalities", default="1,2,100,10000,1000000", help="1 = ungrouped")
ap.add_argument("--check-groups", type=int, default=100, help="compare with the model up to this many groups")
ap.add_argument("--max-groups", type=int, default=1 << 20, help="max_groups of the grouped calls: sizes the device table")
ap.add_argument("--skip-host", action="store_true", help="do not time the host path (a profiler run)")
args = ap.parse_args()
N = args.rows
SCHEMA = {"value_i": "int", "value_f": "float", "by": "int", "sel": "int"}


def timed(fn, iters):
    for _ in range(3):
        fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    p10, p50, p90 = np.percentile(np.array(times) * 1e3, [10, 50, 90])
    return f"{p50:.3f} ({p10:.3f}..{p90:.3f})"


def host(col, by):
    if by is None:
        return col.min(), col.max(), col.sum()
    order = np.argsort(by, kind="stable")
    keys, starts = np.unique(by[order], return_index=True)
    v = col[order]
    return keys, np.minimum.reduceat(v, starts), np.maximum.reduceat(v, starts), np.add.reduceat(v, starts)


def equals_model(got, col, by, mask):
    want = S.stats_oracle(col, by, mask)
    sums = [host_stats.int128(h, l) for h, l in zip(got[5].tolist(), got[6].tolist())]
    return bool(all(np.array_equal(got[i], want[i]) for i in range(3)) and sums == want[5] and got[7:] == want[6:] and
                got[3].tobytes() == want[3].tobytes() and got[4].tobytes() == want[4].tobytes())


rng = np.random.default_rng(0)
eng = HipScanEngine(4, "l2", device=0, capacity_hint=N)
chunk = 1 << 20
for first in range(0, N, chunk):
    eng.append(np.ones((min(chunk, N - first), 4), dtype=np.float32))
sel = np.arange(N, dtype=np.int64) % 1000
cols = {0: rng.integers(-10 ** 9, 10 ** 9, N).astype(np.int64), 1: np.round(rng.uniform(0, 1000, N), 2)}
for a, kind in enumerate(("int64", "float64", "int64", "int64")):
    eng.define_attr(a, kind)
eng.set_attr(0, 0, cols[0])
eng.set_attr(1, 0, cols[1])
eng.set_attr(3, 0, sel)
prog = W.compile_where({"sel": {"$lt": 500}}, SCHEMA)
half = sel < 500
live = np.ones(N, bool)
print(f"{N} rows, median (p10..p90) of {args.iters} calls (ms)", flush=True)
print(f"where_count of the filter alone: {timed(lambda: eng.where_count(prog), args.iters)}", flush=True)
for card in (int(c) for c in args.cardinalities.split(",")):
    by = None if card == 1 else rng.integers(0, card, N).astype(np.int64)
    if by is not None:
        eng.set_attr(2, 0, by)
    group, max_groups = (None, 1) if by is None else (2, args.max_groups)
    if by is not None:
        print(f"{card:>8} groups: facet_values {timed(lambda: eng.facet_values(2, max_groups), args.iters)}  "
              f"with filter {timed(lambda: eng.facet_values(2, max_groups, where=prog), args.iters)}", flush=True)
    for attr, name in ((0, "int64"), (1, "float64")):
        t_all = timed(lambda: eng.attr_stats(attr, group, max_groups), args.iters)
        t_half = timed(lambda: eng.attr_stats(attr, group, max_groups, where=prog), args.iters)
        t_host = "skipped" if args.skip_host else timed(
            lambda: host(eng.get_attr(attr, 0, N, dtype=cols[attr].dtype), None if by is None else eng.get_attr(2, 0, N)),
            max(3, args.iters // 10))
        same = "not compared"
        if card <= args.check_groups:
            same = equals_model(eng.attr_stats(attr, group, max_groups), cols[attr], by, live) and \
                equals_model(eng.attr_stats(attr, group, max_groups, where=prog), cols[attr], by, half)
        print(f"{card:>8} groups, {name:>7}: attr_stats {t_all}  with filter {t_half}  host get_attr + NumPy {t_host}  "
              f"== model: {same}", flush=True)
eng.close()
