#!/usr/bin/env python3
"""Binary vector search at size (include/mlvdb_bits.h): --rows rows of uniformly random codes of 256, 1024 and 2048 bits,
queries drawn the same way.  Wall-clock p50 per call of search_bits, the host's share included (the queries' popcounts, the
upload, the answers' copy back), for 1 / 16 / 256 queries at k = 10 and both metrics, and next to it the bytes the scan must
move -- rows * (8 * words + 8 + 4) per tile pass (the code, the slot and the norm that says "live"; + 1 per row under a
mask), times the call's tiles of 16 queries -- divided by that time, against the 8 TB/s of HBM.  Whether the loads, the
popcounts or the sixteen offers per step bound the kernel is what this is for; a later tile rereads the rows from L2 / MALL
where they fit, so the figure can pass the HBM roof.  The kernel reads the column, the norms and the pool, never the rows:
--dim only sizes the corpus."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=16)
ap.add_argument("--bits", type=int, nargs="+", default=[256, 1024, 2048])
ap.add_argument("--queries", type=int, nargs="+", default=[1, 16, 256])
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--mask", action="store_true", help="search under a filter that matches every row (one more byte per row)")
args = ap.parse_args()
N = args.rows
QT = 16  # kBitsQT


def p50(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


rng = np.random.default_rng(0)
where = W.Program(np.array([(W.TRUE, 0, 0, 0)], dtype=W.OP_DTYPE), np.zeros(0, dtype=np.int64)) if args.mask else None
for bits in args.bits:
    words = bits // 64
    eng = HipScanEngine(args.dim, "ip", device=0, capacity_hint=N)
    eng.define_attr(0, "bits")
    step = 100_000
    for first in range(0, N, step):
        n = min(step, N - first)
        eng.append(rng.standard_normal((n, args.dim), dtype=np.float32))
        eng.bits_set(0, first, W.BitsColumn(rng.integers(0, 2 ** 64, size=(n, words), dtype=np.uint64), np.ones(n, np.uint8)))
    used, live = eng.list_stats(0)
    per_pass = N * (8 * words + 8 + 4 + (1 if args.mask else 0))
    print(f"{N} rows of {bits}-bit codes, pool {used} words, {per_pass / 1e6:.1f} MB per tile pass"
          f"{' (under a mask)' if args.mask else ''}", flush=True)
    for metric in ("hamming", "jaccard"):
        for nq in args.queries:
            q = rng.integers(0, 2 ** 64, size=(nq, words), dtype=np.uint64)
            nt = -(-nq // QT)
            med, lo, hi = p50(lambda: eng.search_bits(0, q, args.k, metric, where), args.iters)
            print(f"{bits:5d} bits  {metric:8s} nq {nq:4d}  {nt:3d} tiles  p50 {med * 1e3:9.3f} ms  ({lo * 1e3:.3f} .. "
                  f"{hi * 1e3:.3f})  {nt * per_pass / med / 1e12:6.3f} TB/s of the 8 TB/s roof  {nq / med:10.0f} queries/s",
                  flush=True)
    eng.close()
