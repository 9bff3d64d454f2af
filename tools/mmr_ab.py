#!/usr/bin/env python3
"""Diversified kNN (include/mlvdb_mmr.h): N x 768 cosine (synth.py's bench corpus), 256-query waves.

Per (k, fetch_k) of --shapes, on one handle, timed alternately:
  plain fetch_k     the plain search at top_k = fetch_k: the candidate step of the call, and the first step of the host loop
                    it replaces (which would then fetch nq x fetch_k rows and run a Python greedy)
  mmr               search_mmr(k, fetch_k, --lam): the same search + one launch of mmr_select_kernel
and the difference, which is the selection: k - 1 gathers of fetch_k rows per query (k x fetch_k x ld x 4 bytes).
Run each GPU step of a job under `timeout`."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--lam", type=float, default=0.5)
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--shapes", default="4:20,10:100,10:1024,64:1024")
args = ap.parse_args()

from mlvectordb_amd import synth  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D, B = args.rows, args.dim, args.batch
eng = HipScanEngine(D, "cosine", device=0, capacity_hint=N)
for _, rows in synth.iter_corpus(0, N, D, threads=16):
    eng.append(rows)
del rows
q = synth.queries(B, D)
ld = (D + 15) // 16 * 16
print(f"corpus {N} x {D} cosine, batch {B}, lambda {args.lam}, p50 of {args.iters} waves each, timed alternately", flush=True)
for shape in args.shapes.split(","):
    k, fetch_k = (int(x) for x in shape.split(":"))
    eng.search(q, fetch_k)
    eng.search_mmr(q, k, fetch_k, args.lam)
    plain, mmr = [], []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        eng.search(q, fetch_k)
        t1 = time.perf_counter()
        lab, _, cnt, _, rank, _ = eng.search_mmr(q, k, fetch_k, args.lam)
        t2 = time.perf_counter()
        plain.append(t1 - t0)
        mmr.append(t2 - t1)
    p, m = float(np.median(plain)) * 1e3, float(np.median(mmr)) * 1e3
    gathered = B * (k - 1) * fetch_k * ld * 4 / 1e9
    moved = float((rank[:, :k] != np.arange(k)).any(axis=1).mean())
    print(f"k {k:3d} fetch_k {fetch_k:5d}: plain {p:9.3f} ms  mmr {m:9.3f} ms  selection {m - p:9.3f} ms "
          f"({gathered:6.2f} GB gathered{f', {gathered / ((m - p) / 1e3):7.0f} GB/s' if m > p else ''})  "
          f"queries whose picks differ from the plain top-k: {moved:.2f}", flush=True)
eng.close()
