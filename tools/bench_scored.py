#!/usr/bin/env python3
"""Scored kNN (include/mlvdb_score.h) against the plain exact search: N x dim cosine (synth.py's bench corpus), k = 10.

Per batch size of --batches, on one handle under MLVDB_STRATEGY_EXACT, timed alternately (one round = one call of each):
  exact    the plain search: exact_scan_kernel, the code scored_scan_kernel is shaped after -- the yardstick
  dist     search_scored with DIST alone: the evaluator's fixed cost
  bonus    search_scored with "$distance - 0.2 * match(tier == 0)": one cond program per row, five ops per pair
  ops32    search_scored with a 32-op program over two attribute operands
Each time is a host clock around a call that ends in a device synchronise (the outputs come back to the host).  Reported:
the p50 of --iters rounds after --warmup, the min .. max spread, and the ratio of each p50 to the plain search's.
Run each GPU step of a job under `timeout`."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=4_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batches", default="8,64")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

from mlvectordb_amd import score as S  # noqa: E402
from mlvectordb_amd import synth  # noqa: E402
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D, K = args.rows, args.dim, args.k
TIER, LIKES = 0, 1
eng = HipScanEngine(D, "cosine", device=0, capacity_hint=N)
for _, rows in synth.iter_corpus(0, N, D, threads=16):
    eng.append(rows)
del rows
rng = np.random.default_rng(77)
eng.define_attr(TIER, "int64")
eng.define_attr(LIKES, "int64")
eng.set_attr(TIER, 0, rng.integers(0, 3, N).astype(np.int64))
likes = rng.integers(0, 50, N).astype(np.int64)
likes[rng.random(N) < 0.2] = W.INT64_ABSENT
eng.set_attr(LIKES, 0, likes)
eng.set_strategy("exact")


def program(ops, conds=()):
    return S.ScoreProgram(np.array(ops, dtype=S.OP_DTYPE), list(conds))


def const(x):
    return (S.CONST, 0, W.float_bits(x))


gold = W.Program(np.array([(W.EQ, TIER, 0, 0)], dtype=W.OP_DTYPE), np.zeros(0, np.int64))
pushes = (const(0.01), (S.ATTR, LIKES, W.float_bits(0.0)), (S.ATTR, TIER, W.float_bits(0.0)), (S.DIST, 0, 0))
binary = (S.ADD, S.MUL, S.SUB, S.MAX, S.MIN)
programs = {
    "dist": program([(S.DIST, 0, 0)]),
    "bonus": program([(S.DIST, 0, 0), const(0.2), (S.MATCH, 0, 0), (S.MUL, 0, 0), (S.SUB, 0, 0)], [gold]),
    "ops32": program([(S.DIST, 0, 0)] + [t for i in range(15) for t in (pushes[i % 4], (binary[i % 5], 0, 0))] + [(S.NEG, 0, 0)]),
}
assert programs["ops32"].ops.size == S.MAX_OPS
calls = {"exact": lambda q: eng.search(q, K)}
for name, prog in programs.items():
    calls[name] = lambda q, prog=prog: eng.search_scored(q, K, prog)

print(f"corpus {N} x {D} cosine, k {K}, strategy exact, p50 of {args.iters} rounds after {args.warmup}, timed alternately", flush=True)
for nq in (int(x) for x in args.batches.split(",")):
    q = synth.queries(nq, D)
    same = np.array_equal(eng.search(q, K)[0], eng.search_scored(q, K, programs["dist"])[0])
    times = {name: [] for name in calls}
    for it in range(args.warmup + args.iters):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call(q)
            t1 = time.perf_counter()
            if it >= args.warmup:
                times[name].append((t1 - t0) * 1e3)
    base = float(np.median(times["exact"]))
    print(f"nq {nq:3d}: DIST alone returns the plain search's labels: {same}", flush=True)
    for name, t in times.items():
        p50 = float(np.median(t))
        print(f"nq {nq:3d} {name:6s}: p50 {p50:9.3f} ms  (min {min(t):9.3f} .. max {max(t):9.3f})  x{p50 / base:5.2f} of exact  "
              f"{N * D * 4 / 1e9 / (p50 / 1e3):7.0f} GB/s of rows", flush=True)
eng.close()
