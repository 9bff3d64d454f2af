#!/usr/bin/env python3
"""List-valued attribute columns at size: N rows with about four tags per row out of --tags distinct ones (a Zipf-like
draw, so a few tags are common and most are rare).  Wall-clock p50 per call, the host's share included, of
  where_count(HAS common tag)     where_eval_kernel walking the lists
  where_count(scalar EQ)          the same kernel on an int64 column of the same handle: the yardstick
  facet_list_values               facet_list_values_kernel over every live row
  compact                         after overwriting a tenth of the lists (the pool repack), with the pool counters around it
The kernels read the columns, the norms and the pool, never the rows: --dim only sizes the corpus."""
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
ap.add_argument("--dim", type=int, default=16)
ap.add_argument("--tags", type=int, default=1000)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
N, T = args.rows, args.tags


def p50(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3, float(np.min(times)) * 1e3, float(np.max(times)) * 1e3


def tagged(rng, n):
    """n rows of 4 draws each (duplicates collapse: about four tags per row) as a ``where.ListColumn``."""
    draws = np.minimum((T * rng.random((n, 4)) ** 3).astype(np.int64), T - 1)  # cubed: tag 0 is in ~ 1/3 of the rows
    draws.sort(axis=1)
    keep = np.ones_like(draws, dtype=bool)
    keep[:, 1:] = draws[:, 1:] != draws[:, :-1]
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=offsets[1:])
    return W.ListColumn(offsets, draws[keep], np.ones(n, dtype=np.uint8))


rng = np.random.default_rng(0)
eng = HipScanEngine(args.dim, "l2", device=0, capacity_hint=N)
step = 1_000_000
for first in range(0, N, step):
    eng.append(rng.standard_normal((min(step, N - first), args.dim), dtype=np.float32))
eng.define_attr(0, "int64_list")
eng.define_attr(1, "int64")
for first in range(0, N, step):
    n = min(step, N - first)
    eng.set_attr_list(0, first, tagged(rng, n))
    eng.set_attr(1, first, (np.arange(first, first + n, dtype=np.int64) % 1000))
used, live = eng.list_stats(0)
print(f"{N} rows, {T} tags, {live / N:.2f} tags per row, pool {used} values", flush=True)


def op(code, attr, a=0, b=0, table=()):
    return W.Program(np.array([(code, attr, a, b)], dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


for name, program in (("HAS tag 0 (common)", op(W.HAS, 0, 0)), (f"HAS tag {T - 1} (rare)", op(W.HAS, 0, T - 1)),
                      ("HAS_ANY of 8", op(W.HAS_ANY, 0, 0, 8, np.arange(0, 8 * 50, 50))),
                      ("scalar EQ (int64 column)", op(W.EQ, 1, 7))):
    med, lo, hi = p50(lambda: eng.where_count(program), args.iters)
    print(f"where_count {name:28s} {med:8.3f} ms  ({lo:.3f} .. {hi:.3f})  matches {eng.where_count(program)}", flush=True)
med, lo, hi = p50(lambda: eng.facet_list_values(0, 1 << 16), max(3, args.iters // 4))
print(f"facet_list_values                        {med:8.3f} ms  ({lo:.3f} .. {hi:.3f})  "
      f"{eng.facet_list_values(0, 1 << 16)[0].size} values", flush=True)
labels = rng.choice(N, N // 10, replace=False)
eng.set_attr_list_at(0, labels, tagged(rng, labels.size))
before = eng.list_stats(0)
t0 = time.perf_counter()
eng.compact()
print(f"compact (identity + repack)              {(time.perf_counter() - t0) * 1e3:8.3f} ms  pool used / live "
      f"{before} -> {eng.list_stats(0)}", flush=True)
eng.close()
