#!/usr/bin/env python3
"""Top rows by one attribute column over N rows (default 10M x 4 floats): int64 columns of 2, 100 and N distinct values and one
float64 column, without a filter and with a one-column filter ({"sel": {"$lt": 500}}, half the rows), for the windows
limit 20 at offset 0 and limit 20 at offset 4076, ascending.  Per column, filter and window, the p50 over --iters calls after
warm-up of
  where_ordered    eng.where_ordered(attr, 20, where, offset=...): ranked on the device, the window alone comes back
  host             what a caller had to do before: eng.where_labels(where) (every live row without a filter) + eng.get_attr of
                   the whole column + np.lexsort((labels, values)) on the CPU
and whether both give the same labels; first of all the same call on a 1000-row index, which is the fixed floor of a call
(launches, copies, synchronisations).  The two routes are timed alternately, call by call.  Every timed call ends in a stream
synchronise inside the library, so the host clock around it is the call's time; the kernels' own times: run this under
`rocprofv3 --kernel-trace --stats` (order_hist_kernel, order_scan_kernel, order_collect_kernel, order_sort_kernel,
where_eval_kernel in the stats).  The output goes to stdout and, with --out, to the next unused profiles/rNN/order_ab.txt."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--host-iters", type=int, default=5)
ap.add_argument("--out", action="store_true", help="also write profiles/rNN/order_ab.txt (the next unused NN)")
args = ap.parse_args()
N = args.rows
SCHEMA = {"by": "int", "sel": "int", "byf": "float"}
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def alternate(fns, iters):
    """p50 (ms) of each of `fns`, called in turn `iters[i]` times after a warm-up call of each."""
    times = [[] for _ in fns]
    for fn in fns:
        fn()
    for it in range(max(iters)):
        for j, fn in enumerate(fns):
            if it < iters[j]:
                t0 = time.perf_counter()
                fn()
                times[j].append(time.perf_counter() - t0)
    return [float(np.median(t)) * 1e3 for t in times]


rng = np.random.default_rng(0)
eng = HipScanEngine(4, "l2", device=0, capacity_hint=N)
chunk = 1 << 20
for first in range(0, N, chunk):
    eng.append(np.ones((min(chunk, N - first), 4), dtype=np.float32))
sel = np.arange(N, dtype=np.int64) % 1000
eng.define_attr(0, "int64")
eng.define_attr(1, "int64")
eng.define_attr(2, "float64")
eng.set_attr(1, 0, sel)
prog = W.compile_where({"sel": {"$lt": 500}}, SCHEMA)
everything = W.Program(np.array([(W.TRUE, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
# the fixed cost of a call (its twenty-odd launches, two copies and two synchronisations): a 1000-row index of its own
small = HipScanEngine(4, "l2", device=0)
small.append(np.ones((1000, 4), dtype=np.float32))
small.define_attr(0, "int64")
small.set_attr(0, 0, rng.permutation(1000).astype(np.int64))
say(f"floor: where_ordered(limit 20) on 1000 rows, p50 of {args.iters} calls: "
    f"{alternate((lambda: small.where_ordered(0, 20),), (args.iters,))[0]:.3f} ms")
small.close()
say(f"{N} rows, one attribute column, p50 (ms) of {args.iters} where_ordered calls and {args.host_iters} host-route calls, "
    f"timed alternately")
columns = [(f"{c} values", 0, rng.integers(0, c, N).astype(np.int64)) for c in (2, 100)]
columns.append((f"{N} values", 0, rng.permutation(N).astype(np.int64)))
columns.append(("float64", 2, rng.standard_normal(N)))
for name, attr, col in columns:
    eng.set_attr(attr, 0, col)
    for where, label in ((None, "no filter"), (prog, "filter")):
        for offset, limit in ((0, 20), (4076, 20)):

            def device():
                return eng.where_ordered(attr, limit, where=where, offset=offset)

            def host():
                labels = eng.where_labels(everything if where is None else where)
                values = eng.get_attr(attr, 0, N, dtype=col.dtype)[labels]
                order = np.lexsort((labels, values))[offset:offset + limit]
                return labels[order]

            t_dev, t_host = alternate((device, host), (args.iters, args.host_iters))
            same = bool(np.array_equal(device()[0], host()))
            say(f"{name:>16} {label:>9} offset {offset:4d} limit {limit}: where_ordered {t_dev:8.3f}  "
                f"host where_labels + get_attr + lexsort {t_host:9.1f}  same labels: {same}")
eng.close()
if args.out:
    nn = 1
    while (ROOT / "profiles" / f"r{nn:02d}").exists():
        nn += 1
    out = ROOT / "profiles" / f"r{nn:02d}"
    out.mkdir(parents=True)
    (out / "order_ab.txt").write_text("\n".join(lines) + "\n")
    print(f"written to {out / 'order_ab.txt'}")
