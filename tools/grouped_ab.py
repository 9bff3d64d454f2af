#!/usr/bin/env python3
"""Grouped kNN (include/mlvdb_grouped.h): N x 768 cosine (synth.py's bench corpus), 256-query waves, k = 10, group_size
1 / 3 / 10.

Group columns: label // S for S rows per value (--group-sizes; contiguous chunks of a document) and one skewed column in
which a single value holds 1 % of the rows (every other row its own value).  Per column the p50 wave time of
  distinct          search_distinct at the same k: the distinct stage alone.  The grouped call runs the same code for it
                    (distinct_chunk), so this is also the parent commit's search_distinct; to time the parent's own build,
                    run this tool with --only-distinct and MLVDB_HIP_LIBRARY pointing at a library built from that commit
  grouped g         search_grouped at group_size g
and `added` = grouped - distinct: the member stage (two column passes, the gather, the merge, its copies) per wave, and
whether slot 0 of every group equals the distinct call's hit.  Run each GPU step of a job under `timeout`."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--group-sizes", default="1,10,100,10000")
ap.add_argument("--members", default="1,3,10", help="the group_size settings")
ap.add_argument("--no-skewed", action="store_true")
ap.add_argument("--only-distinct", action="store_true", help="time search_distinct alone (a library without the grouped entry)")
args = ap.parse_args()

from mlvectordb_amd import synth  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D, K, B = args.rows, args.dim, args.k, args.batch


def p50(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


eng = HipScanEngine(D, "cosine", device=0, capacity_hint=N)
for _, rows in synth.iter_corpus(0, N, D, threads=16):
    eng.append(rows)
del rows
eng.define_attr(0, "int64")
labels = np.arange(N, dtype=np.int64)
q = synth.queries(B, D)
print(f"corpus {N} x {D} cosine, k={K}, batch {B}", flush=True)
columns = [(f"{s} rows/value", labels // int(s)) for s in args.group_sizes.split(",")]
if not args.no_skewed:
    skew = labels.copy()
    skew[np.random.default_rng(0).choice(N, N // 100, replace=False)] = -7
    columns.append(("skewed (one value = 1 %)", skew))
for name, col in columns:
    eng.set_attr(0, 0, col)
    ref = eng.search_distinct(q, K, 0)[0]
    base = p50(lambda: eng.search_distinct(q, K, 0), args.iters)
    print(f"{name:26s} distinct      : {base:9.3f} ms", flush=True)
    if args.only_distinct:
        continue
    for g in [int(x) for x in args.members.split(",")]:
        lab, _, _, sizes, _ = eng.search_grouped(q, K, g, 0)
        t = p50(lambda: eng.search_grouped(q, K, g, 0), args.iters)
        print(f"{name:26s} grouped g={g:3d}: {t:9.3f} ms  added {t - base:8.3f} ms  members {int(sizes.sum()):7d}  "
              f"slot 0 equal: {np.array_equal(lab[:, :, 0], ref)}", flush=True)
eng.close()
