#!/usr/bin/env python3
"""The bits self-join at size (include/mlvdb_bits_join.h) next to the only route there was before it: the codes fetched from
the index (bits_get), range_bits in waves of 256 queries, and a host filter to right > left.  --rows rows of uniformly random
codes of 64, 256 and 1,024 bits with planted near-duplicates (a copy with --flips flipped bits of every twentieth row, so
about one row in ten has a partner), Hamming at the radius that finds the planted pairs alone, and Jaccard on the 256-bit
cell.  Both routes run on one handle in one process and alternate; wall-clock p50 (min .. max) per route, the host's share
included.  Beside the join's time: the share of the VALU ceiling -- 4 lane-operations (two XORs, two bit counts) per 64-bit
word and pair over the triangle of pairs, two walks, against CUs x 4 SIMDs x 16 lanes x clock -- assuming no tile is dropped
early, so a cell where the early exit pays can pass 100 %.  The two routes' pairs are compared once."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mlvectordb_amd import _native  # noqa: E402
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=16)
ap.add_argument("--bits", type=int, nargs="+", default=[64, 256, 1024])
ap.add_argument("--flips", type=int, default=2)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--cus", type=int, default=256)
ap.add_argument("--ghz", type=float, default=2.4)
args = ap.parse_args()
N = args.rows


def join_route(eng, left, metric, radius):
    hits, d64, counts = eng.join_within_bits(0, left, _native.JOIN_LATER, radius, metric=metric, words=WORDS)
    return np.repeat(left, np.diff(hits.offsets)), hits.labels


def range_route(eng, left, metric, radius):
    widths, codes = eng.bits_get(0, 0, N)  # every code crosses the bus, and comes back 256 at a time
    codes = codes.reshape(N, WORDS)
    lefts, rights = [], []
    for lo in range(0, N, 256):
        hits, d64, counts = eng.range_bits(0, codes[lo:lo + 256], radius, metric)
        a = np.repeat(left[lo:lo + 256], np.diff(hits.offsets))
        keep = hits.labels > a
        lefts.append(a[keep])
        rights.append(hits.labels[keep])
    return np.concatenate(lefts), np.concatenate(rights)


rng = np.random.default_rng(0)
ceiling = args.cus * 4 * 16 * args.ghz * 1e9  # lane-operations per second
for bits in args.bits:
    WORDS = bits // 64
    eng = HipScanEngine(args.dim, "ip", device=0, capacity_hint=N)
    eng.define_attr(0, "bits")
    codes = rng.integers(0, 2 ** 64, size=(N, WORDS), dtype=np.uint64)
    planted = N // 20
    copies = codes[:planted].copy()
    for f in rng.integers(0, bits, size=(args.flips, planted)):  # (a bit flipped twice is a nearer copy still)
        copies[np.arange(planted), f >> 6] ^= np.uint64(1) << (f & 63).astype(np.uint64)
    codes[N // 2:N // 2 + planted] = copies
    step = 100_000
    for first in range(0, N, step):
        n = min(step, N - first)
        eng.append(rng.standard_normal((n, args.dim), dtype=np.float32))
        eng.bits_set(0, first, W.BitsColumn(codes[first:first + n], np.ones(n, np.uint8)))
    left = np.arange(N, dtype=np.int64)
    lane_ops = 2 * (N * (N - 1) / 2) * WORDS * 4
    for metric, radius in [("hamming", float(args.flips))] + ([("jaccard", 2.0 * args.flips / bits)] if bits == 256 else []):
        routes = [lambda: join_route(eng, left, metric, radius), lambda: range_route(eng, left, metric, radius)]
        got = [fn() for fn in routes]  # the warm-up calls, and the comparison
        canon = [tuple(x[np.lexsort((p[1], p[0]))] for x in p) for p in got]
        same = all(np.array_equal(x, y) for x, y in zip(*canon))
        times = [[], []]
        for _ in range(args.iters):
            for t, fn in zip(times, routes):
                t0 = time.perf_counter()
                fn()
                t.append(time.perf_counter() - t0)
        for name, t in zip(("join_within_bits", "range_bits waves"), times):
            med = float(np.median(t))
            share = f"  {100 * lane_ops / ceiling / med:5.1f} % of the VALU ceiling" if name == "join_within_bits" else ""
            print(f"{bits:5d} bits  {metric:8s} r={radius:<7g} {name:17s} p50 {med * 1e3:10.1f} ms  ({min(t) * 1e3:.1f} .. "
                  f"{max(t) * 1e3:.1f}){share}", flush=True)
        print(f"             {got[0][0].size} pairs; the routes agree: {same}; speed-up {np.median(times[1]) / np.median(times[0]):.1f}x",
              flush=True)
    eng.close()
