#!/usr/bin/env python3
"""k-means++ seeding (include/mlvdb_seed.h): N x 768 cosine, k blobs of unit-norm centres with Gaussian noise around them
(tools/cluster_ab.py's corpus), k seeds with the default trials per step.

1. Time, alternating on one engine:
     device   HipScanEngine.kmeans_seed: the scans, sum trees, picks and draws on the rows in HBM; k labels come back
     host     the route a user has without it: get_rows of all rows (the corpus over PCIe, "transfer"), greedy k-means++
              in NumPy / OpenBLAS at the process's thread limit ("compute": normalised rows, one sgemm per step for all
              trials, cumulative sums and searchsorted for the draws), the labels back (nothing to write: they are ids)
   The two routes draw from the same distribution with different arithmetic, so their picks differ; both potentials are
   printed.
2. Quality over --seeds seeds: mlvdb_kmeans (--iters iterations at most) from init "random" (k distinct live rows) against
   "k-means++" (the device's picks): the final cost (the sum of the clusters' costs) and the clusters left without members.
A host clock around calls that end in a synchronise.  Run each GPU step of a job under `timeout`."""
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
ap.add_argument("--k", type=int, default=256)
ap.add_argument("--iters", type=int, default=25)
ap.add_argument("--noise", type=float, default=0.06, help="per-component sigma around a unit-norm centre")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--seeds", type=int, default=5)
args = ap.parse_args()

from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D, K = args.rows, args.dim, args.k
TRIALS = min(8, 2 + int(np.floor(np.log(K))))
PIECE = 50_000


def host_seed(x, u):
    """Greedy k-means++ on the host: x float32 [n, d] (normalised here), weights 1 - cos clamped at 0."""
    xn = x / np.sqrt(np.einsum("ij,ij->i", x, x, dtype=np.float64))[:, None].astype(np.float32)

    def dist(rows):  # float64 [len(rows), n]
        out = np.empty((len(rows), xn.shape[0]))
        for s in range(0, xn.shape[0], PIECE):
            out[:, s:s + PIECE] = np.maximum(1.0 - (xn[rows] @ xn[s:s + PIECE].T), 0.0)
        return out

    picks = [int(u[0, 0] * xn.shape[0])]
    best = dist(picks)[0]
    pot = [best.sum()]
    for j in range(1, u.shape[0]):
        cum = np.cumsum(best)
        trial = np.minimum(np.searchsorted(cum, u[j] * cum[-1], side="right"), xn.shape[0] - 1)
        cand = np.minimum(dist(trial), best)
        phi = cand.sum(axis=1)
        w = int(phi.argmin())
        picks.append(int(trial[w]))
        best = cand[w]
        pot.append(phi[w])
    return np.array(picks), np.array(pot)


def med(t):
    return f"median {np.median(t):9.1f} ms  min {min(t):9.1f}  max {max(t):9.1f}"


rng = np.random.default_rng(K)
centres = rng.standard_normal((K, D)).astype(np.float32)
centres /= np.linalg.norm(centres, axis=1)[:, None]
blob = rng.integers(K, size=N)
eng = HipScanEngine(D, "cosine", device=0, capacity_hint=N)
for s in range(0, N, 250_000):
    b = blob[s:s + 250_000]
    eng.append(centres[b] + np.float32(args.noise) * rng.standard_normal((b.size, D), dtype=np.float32))
print(f"corpus {N} x {D} cosine, {K} blobs (noise {args.noise}), k = {K}, {TRIALS} trials per step, {args.reps} repetitions",
      flush=True)

dev, fetch, compute = [], [], []
for rep in range(args.reps + 1):  # (the first repetition warms both routes up and is not counted)
    u = np.random.default_rng(rep).random((K, 8))[:, :TRIALS]
    t0 = time.perf_counter()
    labels, pot, matched = eng.kmeans_seed(K, u)
    t1 = time.perf_counter()
    x = np.concatenate([eng.get_rows(s, min(250_000, N - s)) for s in range(0, N, 250_000)])
    t2 = time.perf_counter()
    host_labels, host_pot = host_seed(x, u)
    t3 = time.perf_counter()
    del x
    assert matched == N and np.unique(blob[labels]).size <= K
    if rep:
        dev.append((t1 - t0) * 1e3)
        fetch.append((t2 - t1) * 1e3)
        compute.append((t3 - t2) * 1e3)
    print(f"  rep {rep}: device potential {pot[-1]:.6g} over {np.unique(blob[labels]).size} blobs, host potential "
          f"{host_pot[-1]:.6g} over {np.unique(blob[host_labels]).size} blobs", flush=True)
total = [a + b for a, b in zip(fetch, compute)]
print(f"  device          : {med(dev)}  per step {np.median(dev) / K:8.3f} ms", flush=True)
print(f"  host   transfer : {med(fetch)}", flush=True)
print(f"  host   compute  : {med(compute)}  per step {np.median(compute) / K:8.3f} ms", flush=True)
print(f"  host   total    : {med(total)}  host / device {np.median(total) / np.median(dev):.1f}", flush=True)

live = np.arange(N)
for seed in range(args.seeds):
    start = {"random": np.sort(np.random.default_rng(seed).choice(live, K, replace=False)).astype(np.int64),
             "k-means++": eng.kmeans_seed(K, np.random.default_rng(seed).random((K, 8))[:, :TRIALS])[0]}
    for init, labels in start.items():
        t0 = time.perf_counter()
        cent, sizes, costs, iterations, converged, matched = eng.kmeans(labels, max_iterations=args.iters)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"  seed {seed} {init:10s}: cost {costs.sum():.6g}  empty clusters {int((sizes == 0).sum()):3d}  "
              f"iterations {iterations:2d} (converged {converged})  {ms:8.1f} ms", flush=True)
eng.close()
