#!/usr/bin/env python3
"""Similarity join (include/mlvdb_join.h): the self-join of N x 768 cosine (synth.py's bench corpus) in which about 1 % of the
rows are overwritten by copies of other rows perturbed by one part in 1e3 per component; the radius (1e-4) takes the planted
pairs and essentially nothing else (unrelated rows lie near distance 1).

On one Index, timed alternately:
  device   Index.join_within("ns", "cosine", radius): the left rows gathered in HBM, waves of 256 through the range chain,
           the scan of a wave starting at the tile of its first label
  host     the route it replaces, made of calls the parent commit has: per 256 rows fetch_values_by_id (the rows over PCIe)
           -> range_search_many (every wave scans all rows, every pair is found twice) -> b <= a stripped in NumPy
Both routes must give the same pair set (asserted).  Median and spread (max - min) of --iters repetitions each after
--warmup of both, a host clock around calls that end in a synchronise.  Run each GPU step of a job under `timeout`."""
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
ap.add_argument("--radius", type=float, default=1e-4)
ap.add_argument("--planted", type=float, default=0.01)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
args = ap.parse_args()

from mlvectordb_amd import Index, synth  # noqa: E402

N, D, R = args.rows, args.dim, args.radius
index = Index(space="cosine")
rng = np.random.default_rng(0)
tables, planted = [], 0
for first, piece in synth.iter_corpus(0, N, D, threads=16):
    piece = np.array(piece)
    m = int(piece.shape[0] * args.planted)
    if m and piece.shape[0] > 2 * m:
        picks = rng.choice(piece.shape[0], 2 * m, replace=False)  # m copies, each of a row that stays as it is
        src, dst = picks[:m], picks[m:]
        piece[dst] = piece[src] * (1 + np.float32(1e-3) * rng.standard_normal((m, D), dtype=np.float32))
        planted += m
    tables.append(index.add_arrays(piece, "ns"))
ids = np.concatenate(tables)
del tables
uuids = [UUID(bytes=b.tobytes()) for b in ids]
row_of = {u: i for i, u in enumerate(uuids)}
WAVE = 256


def device():
    hits = index.join_within("ns", "cosine", R)
    return set(zip(hits.left_labels.tolist(), hits.right_labels.tolist()))


def host():
    pairs = set()
    for s in range(0, N, WAVE):
        values = index.fetch_values_by_id("ns", uuids[s:s + WAVE])
        for a, hits in enumerate(index.range_search_many(values, R, "ns", "cosine", max_results=None), start=s):
            b = np.array([row_of[h.vector_id] for h in hits], dtype=np.int64)
            pairs.update((a, int(x)) for x in b[b > a])
    return pairs


waves = (N + WAVE - 1) // WAVE
print(f"corpus {N} x {D} cosine, {planted} perturbed copies planted, radius {R}; {waves} waves of {WAVE} left rows; "
      f"{args.iters} repetitions each after {args.warmup} warm-ups, timed alternately", flush=True)
for _ in range(args.warmup):
    d, h = device(), host()
assert d == h, f"the routes disagree: {len(d)} pairs on the device, {len(h)} on the host, {len(d ^ h)} in one only"
print(f"pairs: {len(d)} on both routes, the same set", flush=True)
dev, hst = [], []
for _ in range(args.iters):
    t0 = time.perf_counter()
    d = device()
    t1 = time.perf_counter()
    h = host()
    t2 = time.perf_counter()
    assert d == h
    dev.append((t1 - t0) * 1e3)
    hst.append((t2 - t1) * 1e3)
for name, t in (("device", dev), ("host", hst)):
    print(f"{name:6s}: median {np.median(t):10.2f} ms  min {min(t):10.2f}  max {max(t):10.2f}  spread {max(t) - min(t):9.2f} ms  "
          f"per wave {np.median(t) / waves:.3f} ms", flush=True)
gap, spread = float(np.median(hst) - np.median(dev)), max(max(dev) - min(dev), max(hst) - min(hst))
print(f"host - device {gap:10.2f} ms = {gap / max(spread, 1e-9):.1f} x the larger spread ({spread:.2f} ms): "
      f"{'resolved' if gap > 3 * spread else 'NOT resolved (needs more than 3 x)'}; host / device {np.median(hst) / np.median(dev):.2f}",
      flush=True)
index.close()
