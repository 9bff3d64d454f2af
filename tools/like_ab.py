#!/usr/bin/env python3
"""Search by stored examples (include/mlvdb_like.h): N x 768 cosine (synth.py's bench corpus), 256 queries of 4 examples each.

On one Index, timed alternately:
  device   Index.search_like(positive, k): the queries built from the rows in HBM, the plain search at k + 4, the examples
           stripped on the device
  host     the route it replaces: fetch_values_by_id (the rows over PCIe) -> a NumPy average of the unit vectors ->
           search_many at k + 4 -> the examples stripped from the hits on the host
Median and spread (max - min) of --iters repetitions each after --warmup of both.  Run each GPU step of a job under
`timeout`."""
import argparse
import sys
import time
from pathlib import Path
from uuid import UUID

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--examples", type=int, default=4)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()

from mlvectordb_amd import Index, synth  # noqa: E402

N, D, B, E, K = args.rows, args.dim, args.batch, args.examples, args.k
index = Index(space="cosine")
tables = [index.add_arrays(rows, "ns") for _, rows in synth.iter_corpus(0, N, D, threads=16)]
ids = np.concatenate(tables)
del tables
rng = np.random.default_rng(0)
picked = rng.choice(N, (B, E), replace=False)
positive = [[UUID(bytes=ids[j].tobytes()) for j in row] for row in picked]
flat = [u for row in positive for u in row]


def device():
    return index.search_like(positive, K, "ns", "cosine")


def host():
    x = index.fetch_values_by_id("ns", flat).astype(np.float64).reshape(B, E, D)
    x /= np.linalg.norm(x, axis=2, keepdims=True) + 1e-30
    q = x.mean(axis=1).astype(np.float32)
    hits = index.search_many(q, K + E, "ns", "cosine")
    named = [set(row) for row in positive]
    return [[h for h in hits[i] if h.vector_id not in named[i]][:K] for i in range(B)]


print(f"corpus {N} x {D} cosine, {B} queries of {E} examples, k {K}; {args.iters} repetitions each after {args.warmup} "
      f"warm-ups, timed alternately", flush=True)
for _ in range(args.warmup):
    d, h = device(), host()
same = sum([r.vector_id for r in d[i]] == [r.vector_id for r in h[i]] for i in range(B))
print(f"queries whose {K} hits are the same ids on both routes: {same} of {B}", flush=True)
dev, hst = [], []
for _ in range(args.iters):
    t0 = time.perf_counter()
    device()
    t1 = time.perf_counter()
    host()
    t2 = time.perf_counter()
    dev.append((t1 - t0) * 1e3)
    hst.append((t2 - t1) * 1e3)
for name, t in (("device", dev), ("host", hst)):
    print(f"{name:6s}: median {np.median(t):9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}  spread {max(t) - min(t):9.3f} ms  "
          f"p10-p90 {np.percentile(t, 10):.3f}-{np.percentile(t, 90):.3f}", flush=True)
gap, spread = float(np.median(hst) - np.median(dev)), max(max(dev) - min(dev), max(hst) - min(hst))
print(f"host - device {gap:9.3f} ms = {gap / spread:.1f} x the larger spread ({spread:.3f} ms): "
      f"{'resolved' if gap > 3 * spread else 'NOT resolved (needs more than 3 x)'}", flush=True)
index.close()
