#!/usr/bin/env python3
"""Recommend / discover (include/mlvdb_examples.h) against the plain exact search: N x dim cosine (synth.py's bench corpus),
k = 10, --queries queries, bags of --bags examples (half stored rows, half raw vectors; DISCOVER takes one example fewer:
a target and whole pairs).

Per bag size, on one handle under MLVDB_STRATEGY_EXACT, timed alternately (one round = one call of each):
  exact     the yardstick, unchanged code: the same example vectors as queries * bag plain queries through the exact search
            -- the same number of exact passes over the same rows, WaveTopK as the sink
  best      search_examples, MLVDB_EXAMPLES_BEST (roles alternate POS, POS, NEG)
  discover  MLVDB_EXAMPLES_DISCOVER
  context   MLVDB_EXAMPLES_CONTEXT
Each time is a host clock around a call that ends in a device synchronise (the outputs come back to the host).  Reported:
the p50 of --iters rounds after --warmup, the min .. max spread, and the ratio of each p50 to the yardstick's.
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
ap.add_argument("--queries", type=int, default=8)
ap.add_argument("--bags", default="4,8,16,64")
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()

from mlvectordb_amd import _native as N_  # noqa: E402
from mlvectordb_amd import synth  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D, K, NQ = args.rows, args.dim, args.k, args.queries
eng = HipScanEngine(D, "cosine", device=0, capacity_hint=N)
for _, rows in synth.iter_corpus(0, N, D, threads=16):
    eng.append(rows)
del rows
eng.set_strategy("exact")
rng = np.random.default_rng(77)
POS, NEG, TARGET = N_.EXAMPLE_POS, N_.EXAMPLE_NEG, N_.EXAMPLE_TARGET


def bags(mode, size):
    """(labels, vectors, roles, offsets) of NQ bags: every other example a stored row, the others raw vectors."""
    if mode == N_.EXAMPLES_DISCOVER:
        size -= 1 - size % 2
        roles = [TARGET] + [POS, NEG] * (size // 2)
    elif mode == N_.EXAMPLES_CONTEXT:
        roles = [POS, NEG] * (size // 2)
    else:
        roles = [(POS, POS, NEG)[j % 3] for j in range(size)]
    labels = np.where(np.arange(NQ * size) % 2 == 0, rng.integers(0, N, NQ * size), -1).astype(np.int64)
    vectors = synth.queries(NQ * size, D)
    return labels, vectors, np.asarray(roles * NQ, np.int32), np.arange(NQ + 1, dtype=np.int64) * size


print(f"corpus {N} x {D} cosine, k {K}, {NQ} queries, strategy exact, p50 of {args.iters} rounds after {args.warmup}, "
      "timed alternately", flush=True)
for size in (int(x) for x in args.bags.split(",")):
    sets = {name: bags(mode, size) for name, mode in (("best", N_.EXAMPLES_BEST), ("discover", N_.EXAMPLES_DISCOVER),
                                                      ("context", N_.EXAMPLES_CONTEXT))}
    labels, vectors, _, _ = sets["best"]
    plain = vectors.copy()
    plain[labels >= 0] = eng.get_rows_at(labels[labels >= 0])
    calls = {"exact": lambda: eng.search(plain, K)}
    for name, mode in (("best", N_.EXAMPLES_BEST), ("discover", N_.EXAMPLES_DISCOVER), ("context", N_.EXAMPLES_CONTEXT)):
        calls[name] = lambda mode=mode, b=sets[name]: eng.search_examples(mode, *b, K)
    times = {name: [] for name in calls}
    for it in range(args.warmup + args.iters):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            if it >= args.warmup:
                times[name].append((t1 - t0) * 1e3)
    base = float(np.median(times["exact"]))
    for name, t in times.items():
        p50 = float(np.median(t))
        examples = plain.shape[0] if name == "exact" else sets[name][0].size
        print(f"bag {size:2d} {name:8s}: {examples:4d} examples  p50 {p50:9.3f} ms  (min {min(t):9.3f} .. max {max(t):9.3f})  "
              f"x{p50 / base:5.2f} of exact", flush=True)
eng.close()
