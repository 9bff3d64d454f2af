#!/usr/bin/env python3
"""Linear maps of the stored rows (include/mlvdb_transform.h): N x 768 Gaussian rows in an l2 index, mapped to 128 and to 2
columns into a new namespace under the same ids.  Alternating in one process, per repetition and width:
  device   Index.transform(ns, M, shift=t, to=...): the fp64 tile kernel on the rows in HBM, one append on the device
  host     the route a user has without it: get_rows of all rows, fp64 X @ M.T - t in NumPy, add_arrays back up
  binarize the sibling kernel on the same matrix width (64 planes at the least: one code word), as its figure
Every repetition fills a fresh namespace, dropped afterwards.  The floor printed is rows x ld x (out_dim rounded up to the
64-column tile) FMAs over the vector fp64 rate of AMD's MI355X data sheet (78.6 TFLOP/s = 39.3 TFMA/s; data-sheet arithmetic,
not measured here).  A host clock around calls that end in a synchronise.  Run each GPU step of a job under `timeout`."""
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out-dims", type=int, nargs="+", default=[128, 2])
args = ap.parse_args()

from mlvectordb_amd import Index  # noqa: E402

N, D = args.rows, args.dim
FMA_PER_S, TILE, STEP = 39.3e12, 64, 250_000


def line(name, t):
    return f"  {name:8s}: median {np.median(t):9.2f} ms  min {min(t):9.2f}  max {max(t):9.2f}"


def drop(index, name):
    index._ns.pop(name).engine.close()


rng = np.random.default_rng(1)
index = Index(space="l2", device=0, capacity_hint=N, attributes={"sig": "bits128", "sig64": "bits64"})
for s in range(0, N, STEP):
    index.add_arrays(rng.standard_normal((min(STEP, N - s), D), dtype=np.float32), "ns")
ns = index._ns["ns"]
ids = ns.ids.raw[:N].copy()
ld = (D + 15) // 16 * 16
for K in args.out_dims:
    M = rng.standard_normal((K, D), dtype=np.float32)
    t = rng.standard_normal(K)
    nbits = (K + 63) // 64 * 64
    planes = np.zeros((nbits, D), np.float32)
    planes[:K] = M
    print(f"corpus {N} x {D} l2 -> {K} columns, {args.reps} alternated repetitions", flush=True)
    dev, host, sib = [], [], []
    for rep in range(args.reps + 1):  # (the first repetition warms every route up and is not counted)
        t0 = time.perf_counter()
        assert index.transform("ns", M, shift=t, to="dev") == N
        t1 = time.perf_counter()
        for s in range(0, N, STEP):  # (chunked: the fp64 copy of all rows at once would be 6 GB)
            x = ns.engine.get_rows(s, min(STEP, N - s)).astype(np.float64)
            index.add_arrays((x @ M.astype(np.float64).T - t).astype(np.float32), "host", ids=ids[s:s + STEP])
        t2 = time.perf_counter()
        assert index.binarize("ns", "sig" if nbits == 128 else "sig64", planes=planes) == N
        t3 = time.perf_counter()
        if rep == 0:  # the two routes agree up to NumPy's order of summation
            a, b = index._ns["dev"].engine.get_rows(0, 4096), index._ns["host"].engine.get_rows(0, 4096)
            print(f"  device against host, first 4096 rows: largest |difference| {np.abs(a - b).max():.1e}", flush=True)
        else:
            dev.append((t1 - t0) * 1e3)
            host.append((t2 - t1) * 1e3)
            sib.append((t3 - t2) * 1e3)
        drop(index, "dev")
        drop(index, "host")
    floor = N * ld * ((K + TILE - 1) // TILE * TILE) / FMA_PER_S * 1e3
    print(line("device", dev) + f"   fp64 FMA floor (data sheet) {floor:.2f} ms = {floor / np.median(dev):.1%} of the call", flush=True)
    print(line("host", host) + f"   host / device {np.median(host) / np.median(dev):.1f}", flush=True)
    print(line("binarize", sib) + f"   ({nbits} planes)", flush=True)
