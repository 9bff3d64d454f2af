#!/usr/bin/env python3
"""Range search over bit codes at size (include/mlvdb_bits_range.h) next to the only thing the kNN entry can do with such a
question: --rows rows of uniformly random codes of 256, 1024 and 2048 bits, 1 / 32 / 256 queries drawn the same way, a
Hamming radius at which a query has about 100 hits (the Hamming distance of two random N-bit codes is Binomial(N, 1/2); the
radius is its 100 / rows quantile).  In one process and alternating call by call: range_bits (its counting call and its
filling call, as the engine makes them) and search_bits(k = 64).  Wall-clock p50 with min .. max per call, the host's share
included, and the bytes a pass over the rows must move -- rows * (8 * words + 8 + 4): the code, the slot and the norm that
says "live" -- times the call's passes (tiles of 32 queries, two walks each, for the range; tiles of 16 for the scan),
divided by that time, against the 8 TB/s of HBM.  A later tile rereads the rows from L2 / MALL where they fit, so the figure
can pass the HBM roof.  --count-only times the counting call alone (one walk per tile)."""
import argparse
import sys
import time
from pathlib import Path
from statistics import NormalDist

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=16)
ap.add_argument("--bits", type=int, nargs="+", default=[256, 1024, 2048])
ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 256])
ap.add_argument("--hits", type=float, default=100.0)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--count-only", action="store_true")
args = ap.parse_args()
N = args.rows
RANGE_QT, SCAN_QT = 32, 16  # kBitsRangeQT, kBitsQT


def alternate(fns, iters):
    """p50, min and max of each of `fns`, called in turn `iters` times after one warm-up call each."""
    times = [[] for _ in fns]
    for fn in fns:
        fn()
    for _ in range(iters):
        for t, fn in zip(times, fns):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in times]


rng = np.random.default_rng(0)
for bits in args.bits:
    words = bits // 64
    eng = HipScanEngine(args.dim, "ip", device=0, capacity_hint=N)
    eng.define_attr(0, "bits")
    step = 100_000
    for first in range(0, N, step):
        n = min(step, N - first)
        eng.append(rng.standard_normal((n, args.dim), dtype=np.float32))
        eng.bits_set(0, first, W.BitsColumn(rng.integers(0, 2 ** 64, size=(n, words), dtype=np.uint64), np.ones(n, np.uint8)))
    per_pass = N * (8 * words + 8 + 4)
    radius = float(np.floor(bits / 2 + NormalDist().inv_cdf(args.hits / N) * np.sqrt(bits) / 2))
    print(f"{N} rows of {bits}-bit codes, {per_pass / 1e6:.1f} MB per pass, Hamming radius {radius:.0f}", flush=True)
    for nq in args.queries:
        q = rng.integers(0, 2 ** 64, size=(nq, words), dtype=np.uint64)
        counts = eng.range_bits(0, q, radius, "hamming", count_only=True)
        walks = 1 if args.count_only else 2
        passes = (-(-nq // RANGE_QT) * walks, -(-nq // SCAN_QT))
        timed = alternate([lambda: eng.range_bits(0, q, radius, "hamming", count_only=args.count_only),
                           lambda: eng.search_bits(0, q, 64, "hamming")], args.iters)
        for name, np_, (med, lo, hi) in zip(("range_bits", "search_bits k=64"), passes, timed):
            print(f"{bits:5d} bits  nq {nq:4d}  {name:17s} {np_:3d} passes  p50 {med * 1e3:9.3f} ms  ({lo * 1e3:.3f} .. "
                  f"{hi * 1e3:.3f})  {np_ * per_pass / med / 1e12:6.3f} TB/s of the 8 TB/s roof  {nq / med:10.0f} queries/s",
                  flush=True)
        print(f"             hits per query: mean {counts.mean():.1f}, min {counts.min()}, max {counts.max()}", flush=True)
    eng.close()
