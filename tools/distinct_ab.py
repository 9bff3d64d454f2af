#!/usr/bin/env python3
"""Distinct-by-attribute kNN (include/mlvdb_distinct.h): N x 768 cosine (synth.py's bench corpus), 256-query waves, k = 10.

Group columns: label // S for S rows per value (--group-sizes; contiguous chunks of a document) and one skewed column in
which a single value holds 1 % of the rows (every other row its own value).  Per column, the p50 wave time and the
fallback count (queries the list pass could not finish, mlvdb_stats.fallback_queries) of
  plain L           the plain search at top_k = L, L = min(1024, max(64, f x k)): the first step of the host loop that
                    dedupes in Python -- the baseline each factor f is compared with
  distinct f        search_distinct with DISTINCT_OVERSAMPLE = f, for f = 0 (every query on the grouped exact scan; at most
                    --scan-iters waves: 0.2 s each at 10M rows) and the --factors
and whether every setting's ids equal the default's.  Every setting returns the same answer; the table decides the default.
Run each GPU step of a job under `timeout`."""
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
ap.add_argument("--scan-iters", type=int, default=2)
ap.add_argument("--group-sizes", default="1,10,100,10000")
ap.add_argument("--factors", default="2,4,16,64")
ap.add_argument("--no-skewed", action="store_true")
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
default = eng.get_tuning("DISTINCT_OVERSAMPLE")
q = synth.queries(B, D)
factors = [int(x) for x in args.factors.split(",")]
print(f"corpus {N} x {D} cosine, k={K}, batch {B}, DISTINCT_OVERSAMPLE default {default}", flush=True)
plain = {}
for L in sorted({min(1024, max(64, f * K)) for f in factors}):
    plain[L] = p50(lambda: eng.search(q, L), args.iters)
    print(f"plain search top_k={L}: {plain[L]:.3f} ms", flush=True)
columns = [(f"{s} rows/value", labels // int(s)) for s in args.group_sizes.split(",")]
if not args.no_skewed:
    skew = labels.copy()
    skew[np.random.default_rng(0).choice(N, N // 100, replace=False)] = -7
    columns.append(("skewed (one value = 1 %)", skew))
for name, col in columns:
    eng.set_attr(0, 0, col)
    eng.set_tuning(DISTINCT_OVERSAMPLE=default)
    ref = eng.search_distinct(q, K, 0)[0]
    for f in [0] + factors:
        eng.set_tuning(DISTINCT_OVERSAMPLE=f)
        eng.last_stats()
        lab = eng.search_distinct(q, K, 0)[0]
        fallbacks = eng.last_stats()["fallback_queries"]
        t = p50(lambda: eng.search_distinct(q, K, 0), args.scan_iters if f == 0 else args.iters)
        L = min(1024, max(64, f * K))
        base = f"  plain L={L}: {plain[L]:.3f} ms (x{t / plain[L]:.2f})" if f else ""
        print(f"{name:26s} oversample {f:3d}: {t:9.3f} ms  fallbacks {fallbacks:4d}{base}  ids equal: "
              f"{np.array_equal(lab, ref)}", flush=True)
eng.set_tuning(DISTINCT_OVERSAMPLE=default)
eng.close()
