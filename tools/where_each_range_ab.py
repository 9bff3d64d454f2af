#!/usr/bin/env python3
"""Per-query filters in batched range search (include/mlvdb_where_each_range.h): N x 768 l2 (synth.py's bench corpus),
256-query waves, one radius set on the first 1M rows so that an unfiltered query has ~128 hits on the whole corpus
(BASELINE configs[3]'s mean hit count: the distance below which the wave has 128 x 1M / N hits per query there).

tenant = label % T and bucket = label // T; filter t of a combination is {"tenant": t, "bucket": {"$lt": R}}: R rows per
filter (clamped at the whole tenant, N / T rows).  Query i uses filter i % T.  For T in --tenants and each R, the p50 wave
time of
  loop            one single-filter range(where=...) per distinct filter on its queries (the only way without the batched
                  entry: the baseline)
  each            one range_each call (what Index.range_search_many(where=[...]) issues), default WHERE_GATHER
  scan / gather   the same call with WHERE_GATHER=0 (every program scanned) / huge (every program gathered)
the routes the default takes, the route rule's ratio matches x ceil(queries / 4) x 1000 / live per program (what
WHERE_GATHER is compared against), the hits per query and whether every route's hits equal the loop's, labels and distance
bits.  The gather / scan pair brackets the crossover.

Kernel times: --rocprof runs the headline combinations once more in a child process under
`rocprofv3 --kernel-trace --stats` (a run of its own, nothing else traced) and prints the stats' top kernels.  Every GPU
step runs under `timeout`."""
import argparse
import csv
import subprocess
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
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--tenants", default="1,8,64,256")
ap.add_argument("--rows-per-filter", default="1000,10000,100000")
ap.add_argument("--hits", type=float, default=128.0, help="mean hits of an unfiltered query the radius is set for")
ap.add_argument("--no-loop", action="store_true", help="skip the single-filter loop (profiling runs)")
ap.add_argument("--rocprof", default="", help="output directory: also run --rocprof-combos under rocprofv3 --stats")
ap.add_argument("--rocprof-combos", default="256:10000,8:100000")
ap.add_argument("--timeout", type=int, default=900, help="time limit of the rocprofv3 child (s)")
args = ap.parse_args()

if args.rocprof:
    out = Path(args.rocprof)
    out.mkdir(parents=True, exist_ok=True)
    for combo in args.rocprof_combos.split(","):
        t, s = combo.split(":")
        tag = f"T{t}_r{s}"
        cmd = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
               "-d", str(out / tag),
               "-o", tag, "--", sys.executable, str(Path(__file__).resolve()), "--rows", str(args.rows), "--dim",
               str(args.dim), "--batch", str(args.batch), "--hits", str(args.hits), "--iters", "3", "--tenants", t,
               "--rows-per-filter", s, "--no-loop"]
        print("$", " ".join(cmd), flush=True)
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"rocprofv3 run {tag} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
        for stats in sorted((out / tag).rglob("*kernel_stats.csv")):
            with open(stats) as fh:
                rows = list(csv.DictReader(fh))
            rows.sort(key=lambda r: -float(r.get("TotalDurationNs", 0)))
            print(f"-- {stats.relative_to(out)}")
            for r in rows[:12]:
                print(f"   {r['Name'][:70]:70s} calls {int(r['Calls']):6d}  avg {float(r['AverageNs']) / 1e3:9.1f} us  "
                      f"total {float(r['TotalDurationNs']) / 1e6:9.2f} ms")
    sys.exit(0)

from mlvectordb_amd import _native, synth  # noqa: E402
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D, B = args.rows, args.dim, args.batch
SCHEMA = {"tenant": "int", "bucket": "int"}
ALWAYS = 1 << 30
CAP = 8192  # the capacity bench.py's range leg asks for
SAMPLE = min(N, 1_000_000)


def p50(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


def same_hits(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.int32), y[1].view(np.int32)) for x, y in zip(a, b))


eng = HipScanEngine(D, "l2", device=0, capacity_hint=N)
q = synth.queries(B, D)
radius, done = None, 0
for _, rows in synth.iter_corpus(0, N, D, threads=16):
    eng.append(rows)
    done += rows.shape[0]
    if radius is None and done >= SAMPLE:  # the radius: from the rows appended so far
        want = int(round(args.hits * done / N * B))  # hits of the whole wave on these rows
        near = np.sort(eng.search(q, 1024)[1], axis=None)  # (a query with more than 1024 hits here counts as 1024)
        radius = float(near[min(want, near.size - 1)])
del rows
eng.define_attr(0, "int64")
eng.define_attr(1, "int64")
labels = np.arange(N, dtype=np.int64)
default_gather = eng.get_tuning("WHERE_GATHER")
plain = eng.range(q, radius, CAP)
nh = np.array([h[0].size for h in plain])
print(f"corpus {N} x {D} l2, batch {B}, radius {radius:.6g} (squared l2): unfiltered hits per query mean {nh.mean():.1f} "
      f"max {nh.max()}, WHERE_GATHER default {default_gather}", flush=True)
print(f"unfiltered range wave: {p50(lambda: eng.range(q, radius, CAP), args.iters):.3f} ms", flush=True)
one = W.compile_where({"tenant": 0}, SCHEMA)
eng.set_attr(0, 0, labels % 2)
eng.set_attr(1, 0, labels // 2)
print(f"masked range wave (one filter, half the rows, all {B} queries): "
      f"{p50(lambda: eng.range(q, radius, CAP, where=one), args.iters):.3f} ms", flush=True)
for T in [int(x) for x in args.tenants.split(",")]:
    eng.set_attr(0, 0, labels % T)
    eng.set_attr(1, 0, labels // T)
    of_all = (np.arange(B) % T).astype(np.int32)
    for R in [int(x) for x in args.rows_per_filter.split(",")]:
        fs = [{"tenant": t, "bucket": {"$lt": R}} for t in range(min(T, B))]
        programs, of = W.compile_each([fs[i] for i in of_all], SCHEMA)
        matches = eng.count_each(programs)
        nq_p = np.bincount(of, minlength=len(programs))
        ratio = matches * -(-nq_p // 4) * 1000 / N
        eng.set_tuning(WHERE_GATHER=default_gather)
        t_each = p50(lambda: eng.range_each(q, radius, CAP, programs, of), args.iters)
        hits, routes = eng.range_each(q, radius, CAP, programs, of, return_routes=True)
        eng.set_tuning(WHERE_GATHER=0)
        t_scan = p50(lambda: eng.range_each(q, radius, CAP, programs, of), args.iters)
        hits_s = eng.range_each(q, radius, CAP, programs, of)
        eng.set_tuning(WHERE_GATHER=ALWAYS)
        t_gather = p50(lambda: eng.range_each(q, radius, CAP, programs, of), args.iters)
        hits_g = eng.range_each(q, radius, CAP, programs, of)
        eng.set_tuning(WHERE_GATHER=default_gather)
        per = np.array([h[0].size for h in hits])
        line = (f"T={T:4d} {int(matches.mean()):7d} rows/filter (ratio {np.median(ratio):9.1f}, hits/query mean {per.mean():7.2f} "
                f"max {per.max():5d}): each {t_each:8.3f} ms  scan {t_scan:8.3f}  gather {t_gather:8.3f}")
        same = same_hits(hits, hits_s) and same_hits(hits, hits_g)
        if not args.no_loop:
            def loop():
                out = [None] * B
                for p, prog in enumerate(programs):
                    sel = np.flatnonzero(of == p)
                    for j, h in zip(sel, eng.range(q[sel], radius, CAP, where=prog)):
                        out[j] = h
                return out
            t_loop = p50(loop, max(1, min(args.iters, 3)))
            same = same and same_hits(hits, loop())
            line += f"  loop {t_loop:9.3f}  (x{t_loop / t_each:.1f})"
        names = {r: int((routes == r).sum()) for r in (_native.ROUTE_NONE, _native.ROUTE_SCAN, _native.ROUTE_GATHER)}
        line += "  routes " + " ".join(f"{_native.ROUTE_NAMES[r]}={c}" for r, c in names.items() if c)
        line += f"  hits equal: {same}"
        print(line, flush=True)
eng.close()
