#!/usr/bin/env python3
"""Per-query filters (include/mlvdb_where_each.h): N x 768 cosine (synth.py's bench corpus), 256-query waves, k = 10.

tenant = label % T and bucket = (label // T) % 10000; filter t of a combination is {"tenant": t, "bucket": {"$lt": B}}
with B set for the requested selectivity (clamped at the whole tenant: 1 / T of the rows).  Query i uses filter i % T.
For T in --tenants and each selectivity, the p50 wave time of
  each            one search_each call (what Index.search_many(where=[...]) issues), default WHERE_GATHER
  scan / gather   the same call with WHERE_GATHER=0 (every program scanned) / huge (every program gathered)
  loop            one single-program search(where=...) per distinct filter on its queries (today's only way)
the routes the default takes, the route rule's ratio matches x ceil(queries / 4) x 1000 / live per program (what
WHERE_GATHER is compared against) and whether every route's ids equal the loop's.  The gather / scan pair brackets the
crossover that sets WHERE_GATHER's default.

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
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--tenants", default="1,8,64,256")
ap.add_argument("--selectivities", default="0.0001,0.001,0.01,0.1")
ap.add_argument("--no-loop", action="store_true", help="skip the single-filter loop (profiling runs)")
ap.add_argument("--rocprof", default="", help="output directory: also run --rocprof-combos under rocprofv3 --stats")
ap.add_argument("--rocprof-combos", default="256:0.001,1:0.001")
ap.add_argument("--timeout", type=int, default=900, help="time limit of the rocprofv3 child (s)")
args = ap.parse_args()

if args.rocprof:
    out = Path(args.rocprof)
    out.mkdir(parents=True, exist_ok=True)
    for combo in args.rocprof_combos.split(","):
        t, s = combo.split(":")
        tag = f"T{t}_s{s}"
        cmd = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv",
               "-d", str(out / tag),
               "-o", tag, "--", sys.executable, str(Path(__file__).resolve()), "--rows", str(args.rows), "--dim",
               str(args.dim), "--batch", str(args.batch), "--k", str(args.k), "--iters", "3", "--tenants", t,
               "--selectivities", s, "--no-loop"]
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

N, D, K, B = args.rows, args.dim, args.k, args.batch
SCHEMA = {"tenant": "int", "bucket": "int"}
ALWAYS = 1 << 30


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
eng.define_attr(1, "int64")
labels = np.arange(N, dtype=np.int64)
default_gather = eng.get_tuning("WHERE_GATHER")
q = synth.queries(B, D)
print(f"corpus {N} x {D} cosine, k={K}, batch {B}, WHERE_GATHER default {default_gather}", flush=True)
print(f"unfiltered wave: {p50(lambda: eng.search(q, K), args.iters):.3f} ms", flush=True)
for T in [int(x) for x in args.tenants.split(",")]:
    eng.set_attr(0, 0, labels % T)
    bucket = (labels // T) % 10000
    eng.set_attr(1, 0, bucket)
    of_all = (np.arange(B) % T).astype(np.int32)
    for s in [float(x) for x in args.selectivities.split(",")]:
        lim = int(min(10000, max(1, round(s * T * 10000))))
        fs = [{"tenant": t, "bucket": {"$lt": lim}} for t in range(min(T, B))]
        programs, of = W.compile_each([fs[i] for i in of_all], SCHEMA)
        matches = eng.count_each(programs)
        nq_p = np.bincount(of, minlength=len(programs))
        ratio = matches * -(-nq_p // 4) * 1000 / N
        eng.set_tuning(WHERE_GATHER=default_gather)
        t_each = p50(lambda: eng.search_each(q, K, programs, of), args.iters)
        lab, _, _, routes = eng.search_each(q, K, programs, of, return_routes=True)
        eng.set_tuning(WHERE_GATHER=0)
        t_scan = p50(lambda: eng.search_each(q, K, programs, of), args.iters)
        lab_s, _, _ = eng.search_each(q, K, programs, of)
        eng.set_tuning(WHERE_GATHER=ALWAYS)
        t_gather = p50(lambda: eng.search_each(q, K, programs, of), args.iters)
        lab_g, _, _ = eng.search_each(q, K, programs, of)
        eng.set_tuning(WHERE_GATHER=default_gather)
        line = (f"T={T:4d} sel {matches.mean() / N:8.4%} ({int(matches.mean())} rows/filter, ratio {np.median(ratio):9.1f}): "
                f"each {t_each:8.3f} ms  scan {t_scan:8.3f}  gather {t_gather:8.3f}")
        same = np.array_equal(lab, lab_s) and np.array_equal(lab, lab_g)
        if not args.no_loop:
            def loop():
                out = np.empty((B, K), np.int64)
                for p, prog in enumerate(programs):
                    sel = np.flatnonzero(of == p)
                    out[sel] = eng.search(q[sel], K, where=prog)[0]
                return out
            t_loop = p50(loop, max(1, min(args.iters, 3)))
            same = same and np.array_equal(lab, loop())
            line += f"  loop {t_loop:9.3f}  (x{t_loop / t_each:.1f})"
        names = {r: int((routes == r).sum()) for r in (_native.ROUTE_NONE, _native.ROUTE_SCAN, _native.ROUTE_GATHER)}
        line += "  routes " + " ".join(f"{_native.ROUTE_NAMES[r]}={c}" for r, c in names.items() if c)
        line += f"  ids equal: {same}"
        print(line, flush=True)
eng.close()
