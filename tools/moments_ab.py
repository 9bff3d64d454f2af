#!/usr/bin/env python3
"""Row moments (include/mlvdb_moments.h): N x 768 Gaussian rows in an ip index.  Alternating on one engine, per repetition:
  device   HipScanEngine.row_moments: the fp64 Gram tile kernel on the rows in HBM, dim + dim^2 doubles come down
  filtered the same call under a dict filter half the rows match (the mask is evaluated first, the FMAs are the same)
then, once (it takes seconds):
  host     the route a user has without the call: get_rows of all rows, the sums and the fp64 X.T @ X in NumPy
The floor printed is rows x ld x (ld + tile) / 2 FMAs -- the upper triangle of 128-column tile pairs -- over the vector fp64
rate of AMD's MI355X data sheet (78.6 TFLOP/s = 39.3 TFMA/s; not measured here).  A host clock around calls that end in a
synchronise.  Run each GPU step of a job under `timeout`."""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-reps", type=int, default=1)
args = ap.parse_args()

from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D = args.rows, args.dim
FMA_PER_S, TILE, STEP = 39.3e12, 128, 250_000
TAG = 0


def line(name, t):
    return f"  {name:8s}: median {np.median(t):9.2f} ms  min {min(t):9.2f}  max {max(t):9.2f}"


rng = np.random.default_rng(1)
eng = HipScanEngine(D, "ip", device=0, capacity_hint=N)
for s in range(0, N, STEP):
    eng.append(rng.standard_normal((min(STEP, N - s), D), dtype=np.float32))
eng.define_attr(TAG, "int64")
eng.set_attr(TAG, 0, np.arange(N, dtype=np.int64) % 2)
half = W.Program(np.array([(W.IN, TAG, 0, 1)], dtype=W.OP_DTYPE), np.array([1], dtype=np.int64))
print(f"corpus {N} x {D} ip, {args.reps} alternated repetitions", flush=True)
dev, filt = [], []
for rep in range(args.reps + 1):  # (the first repetition warms both routes up and is not counted)
    t0 = time.perf_counter()
    count, sums, gram = eng.row_moments()
    t1 = time.perf_counter()
    assert count == N and eng.row_moments(half)[0] == N // 2
    t2 = time.perf_counter()
    if rep:
        dev.append((t1 - t0) * 1e3)
        filt.append((t2 - t1) * 1e3)
ld = (D + 15) // 16 * 16
floor = N * ld * (ld + TILE) / 2 / FMA_PER_S * 1e3
print(line("device", dev) + f"   fp64 FMA floor {floor:.2f} ms = {floor / np.median(dev):.1%} of the call", flush=True)
print(line("filtered", filt), flush=True)
host = []
for rep in range(args.host_reps):
    t0 = time.perf_counter()
    h_sums, h_gram = np.zeros(D), np.zeros((D, D))
    for s in range(0, N, STEP):  # (chunked: the fp64 copy of all rows at once would be 6 GB)
        x = eng.get_rows(s, min(STEP, N - s)).astype(np.float64)
        h_sums += x.sum(axis=0)
        h_gram += x.T @ x
    host.append((time.perf_counter() - t0) * 1e3)
if host:
    print(line("host", host) + f"   host / device {np.median(host) / np.median(dev):.0f}", flush=True)
    scale = np.sqrt(np.outer(np.diag(h_gram), np.diag(h_gram)))
    print(f"  device against NumPy's order of summation: largest |difference| {np.abs(gram - h_gram).max() / scale.max():.1e} of "
          f"the diagonal, sums {np.abs(sums - h_sums).max():.1e} absolute", flush=True)
eng.close()
