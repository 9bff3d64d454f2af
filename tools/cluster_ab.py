#!/usr/bin/env python3
"""Clustering (include/mlvdb_cluster.h): spherical k-means of N x 768 cosine, k blobs of unit-norm centres with Gaussian noise
around them, from one stored row per blob, until no row moves or --iters iterations have run.

On one engine, timed one after the other per k:
  device   HipScanEngine.kmeans from k stored rows given as labels: assignment scans, ordered member lists and blocked sums
           on the rows in HBM, the cluster id written into an int64 column
  host     the route a user has without it: get_rows of all rows (the corpus over PCIe, "transfer"), Lloyd's algorithm in
           NumPy / OpenBLAS at the process's thread limit ("compute": normalised rows, one sgemm per iteration and chunk, the
           means by a sort and a segmented sum), set_attr of the labels ("write-back")
Both routes start from the same rows and must end with the same partition (asserted; the same number of iterations too).
Then one iteration against the exact search of the same k vectors on the same handle (strategy forced exact, top 1): the
assignment chain's scans do the same arithmetic, the rest of an iteration is state traffic, listing, sums and one wait.  The
engine's profiling events give the scan launches' share, and the assignment alone (mlvdb_assign_nearest: the same scans and
listing, no weights and no column sums) gives the sum stage's share by difference.  A host clock around calls that end in a synchronise.  Run each GPU
step of a job under `timeout`."""
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
ap.add_argument("--k", type=int, nargs="+", default=[16, 256])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--noise", type=float, default=0.06, help="per-component sigma around a unit-norm centre")
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D = args.rows, args.dim
PIECE = 50_000


def host_lloyd(x, seeds, iters):
    """Spherical k-means on the host: x float32 [n, d] (normalised here), from rows `seeds`."""
    xn = x / np.sqrt(np.einsum("ij,ij->i", x, x, dtype=np.float64))[:, None].astype(np.float32)
    c = xn[seeds].copy()
    prev = None
    for t in range(1, iters + 1):
        cn = c / np.sqrt(np.einsum("ij,ij->i", c, c, dtype=np.float64))[:, None].astype(np.float32)
        assign = np.empty(x.shape[0], np.int64)
        for s in range(0, x.shape[0], PIECE):
            assign[s:s + PIECE] = (xn[s:s + PIECE] @ cn.T).argmax(axis=1)
        order = np.argsort(assign, kind="stable")
        counts = np.bincount(assign, minlength=c.shape[0])
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        filled = counts > 0  # (reduceat over the clusters that have members only: an empty one has no segment to sum)
        sums = np.add.reduceat(xn[order], starts[filled], axis=0, dtype=np.float64)
        c[filled] = (sums / counts[filled, None]).astype(np.float32)
        done = t >= 2 and np.array_equal(assign, prev)
        prev = assign
        if done:
            break
    return assign, t


def med(t):
    return f"median {np.median(t):9.1f} ms  min {min(t):9.1f}  max {max(t):9.1f}"


for k in args.k:
    rng = np.random.default_rng(k)
    centres = rng.standard_normal((k, D)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1)[:, None]
    blob = rng.integers(k, size=N)
    eng = HipScanEngine(D, "cosine", device=0, capacity_hint=N)
    for s in range(0, N, 250_000):
        b = blob[s:s + 250_000]
        eng.append(centres[b] + np.float32(args.noise) * rng.standard_normal((b.size, D), dtype=np.float32))
    eng.define_attr(0, "int64")
    seeds = np.array([np.flatnonzero(blob == j)[0] for j in range(k)], dtype=np.int64)
    print(f"corpus {N} x {D} cosine, {k} blobs (noise {args.noise}), k = {k}, at most {args.iters} iterations, "
          f"{args.reps} repetitions", flush=True)

    dev, fetch, compute, write = [], [], [], []
    for rep in range(args.reps + 1):  # (the first repetition warms both routes up and is not counted)
        t0 = time.perf_counter()
        cent, sizes, costs, iterations, converged, matched = eng.kmeans(seeds, max_iterations=args.iters, assign_attr=0)
        t1 = time.perf_counter()
        column = eng.get_attr(0, 0, N)
        t2 = time.perf_counter()
        x = np.concatenate([eng.get_rows(s, min(250_000, N - s)) for s in range(0, N, 250_000)])
        t3 = time.perf_counter()
        assign, host_iterations = host_lloyd(x, seeds, args.iters)
        t4 = time.perf_counter()
        eng.set_attr(0, 0, assign.astype(np.int64))
        t5 = time.perf_counter()
        del x
        assert np.array_equal(column, assign), f"the routes disagree on {(column != assign).sum()} rows"
        assert iterations == host_iterations, (iterations, host_iterations)
        if rep:
            dev.append((t1 - t0) * 1e3)
            fetch.append((t3 - t2) * 1e3)
            compute.append((t4 - t3) * 1e3)
            write.append((t5 - t4) * 1e3)
    print(f"  the same partition on both routes, {iterations} iterations, converged {converged}, "
          f"sizes {int(sizes.min())}..{int(sizes.max())}", flush=True)
    total = [a + b + c for a, b, c in zip(fetch, compute, write)]
    print(f"  device            : {med(dev)}  per iteration {np.median(dev) / iterations:8.2f} ms", flush=True)
    print(f"  host   transfer   : {med(fetch)}", flush=True)
    print(f"  host   compute    : {med(compute)}  per iteration {np.median(compute) / iterations:8.2f} ms", flush=True)
    print(f"  host   write-back : {med(write)}", flush=True)
    print(f"  host   total      : {med(total)}  host / device {np.median(total) / np.median(dev):.1f}", flush=True)

    # one iteration against the exact search of the same k vectors (top 1) on the same handle
    eng.set_strategy("exact")
    q = eng.get_rows_at(seeds)
    one, search, scans, assign_only = [], [], [], []
    for rep in range(args.reps + 1):
        eng.set_profiling(True)
        eng.last_stats()
        t0 = time.perf_counter()
        eng.kmeans(seeds, max_iterations=1)
        t1 = time.perf_counter()
        st = eng.last_stats()
        eng.set_profiling(False)
        t2 = time.perf_counter()
        eng.search(q, 1)
        t3 = time.perf_counter()
        eng.assign_nearest(seeds)  # the same scans and listing, the cost slice alone: no weights, no column sums
        t4 = time.perf_counter()
        if rep:
            assign_only.append((t4 - t3) * 1e3)
            one.append((t1 - t0) * 1e3)
            search.append((t3 - t2) * 1e3)
            scans.append(float(st.get("scan_ms", float("nan"))))
    print(f"  one iteration     : {med(one)}  of which scan launches {np.median(scans):8.2f} ms "
          f"({int(st.get('scan_launches', 0))} launches)", flush=True)
    print(f"  assignment alone  : {med(assign_only)}  iteration - assignment (weights + column sums) "
          f"{np.median(one) - np.median(assign_only):8.2f} ms = {(np.median(one) - np.median(assign_only)) / np.median(one):.0%} of "
          f"an iteration; assignment - scans (listing, cost, the wait) {np.median(assign_only) - np.median(scans):8.2f} ms", flush=True)
    print(f"  exact search, k=1 : {med(search)}  iteration / search {np.median(one) / np.median(search):.2f}, "
          f"scans / search {np.median(scans) / np.median(search):.2f}", flush=True)
    eng.close()
