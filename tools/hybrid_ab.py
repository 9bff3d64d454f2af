#!/usr/bin/env python3
"""Hybrid search at size (include/mlvdb_hybrid.h): --rows rows of --dim cosine components, each with a sparse vector of
about --row-len nonzeros out of --vocab terms (the workload of tools/sparse_ab.py), queries of a dense vector and about
--query-len terms.  For 1 / 8 / 64 / 256 queries at k = 10, fetch_dense = 100, fetch_sparse = 64, wall-clock p50 (min .. max)
over --iters calls of
  (a) the hybrid call, LINEAR (the completion launches run);
  (b) the hybrid call, RRF without components (they are skipped);
  (c) what the call replaces on the same build: search64 + search_batch_sparse + pair_distances for the rows the dense list
      lacks + the fusion in NumPy.  The sparse score of a row the sparse list lacks has no entry to come from: (c) leaves it
      at 0, so it does LESS than (a) -- its time is a lower bound of the caller-side pipeline;
  (d), (e) the two legs alone, to see what (a) adds to their sum.
The five are interleaved call by call within one process, so drift of the box hits them alike."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--vocab", type=int, default=30_522)
ap.add_argument("--row-len", type=int, default=64)
ap.add_argument("--query-len", type=int, default=32)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--fetch-dense", type=int, default=100)
ap.add_argument("--fetch-sparse", type=int, default=64)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
N, V, K, FD, FS = args.rows, args.vocab, args.k, args.fetch_dense, args.fetch_sparse


def vectors(rng, n, mean, most) -> W.SparseColumn:
    """n vectors of about ``mean`` (1..most) nonzeros: squared-uniform term draws, duplicates within a vector collapse."""
    lens = np.clip(rng.poisson(mean, n), 1, most)
    owner = np.repeat(np.arange(n, dtype=np.int64), lens)
    terms = np.minimum((V * rng.random(owner.size) ** 2).astype(np.int64), V - 1)
    key = np.unique(owner * V + terms)  # sorted by (vector, term), unique
    owner, terms = key // V, key % V
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(owner, minlength=n), out=offsets[1:])
    weights = rng.random(terms.size, dtype=np.float32) + np.float32(0.05)
    return W.SparseColumn(offsets, terms.astype(np.int32), weights, np.ones(n, dtype=np.uint8))


def host_fusion(eng, q, sq):
    """(c): the two legs, the distances the dense list lacks, LINEAR fusion and the top k per query in NumPy."""
    dl, _, dc, dd = eng.search64(q, FD)
    sl, _, sc, ss = eng.search_batch_sparse(0, sq, FS)
    sd = eng.pair_distances(q, np.where(sl >= 0, sl, 0))[0]
    out = np.full((q.shape[0], K), -1, dtype=np.int64)
    for i in range(q.shape[0]):
        score = dict(zip(sl[i, :sc[i]].tolist(), ss[i, :sc[i]].tolist()))
        dist = dict(zip(sl[i, :sc[i]].tolist(), sd[i, :sc[i]].tolist()))
        dist.update(zip(dl[i, :dc[i]].tolist(), dd[i, :dc[i]].tolist()))
        lab = np.fromiter(dist, dtype=np.int64, count=len(dist))
        fused = np.array([score.get(int(l), 0.0) for l in lab]) - np.array([dist[int(l)] for l in lab])
        top = lab[np.lexsort((lab, -fused))][:K]
        out[i, :top.size] = top
    return out


rng = np.random.default_rng(0)
eng = HipScanEngine(args.dim, "cosine", device=0, capacity_hint=N)
eng.define_attr(0, "sparse")
step = 100_000
for first in range(0, N, step):
    n = min(step, N - first)
    eng.append(rng.standard_normal((n, args.dim), dtype=np.float32))
    eng.set_attr_sparse(0, first, vectors(rng, n, args.row_len, 255))
print(f"{N} rows x {args.dim} cosine, vocabulary {V}, k {K}, fetch_dense {FD}, fetch_sparse {FS}, {args.iters} calls each", flush=True)
for nq in (1, 8, 64, 256):
    q = rng.standard_normal((nq, args.dim), dtype=np.float32)
    sq = vectors(rng, nq, args.query_len, 1024)
    calls = {
        "a hybrid linear": lambda: eng.search_hybrid(q, 0, sq, K, FD, FS, method="linear"),
        "b hybrid rrf": lambda: eng.search_hybrid(q, 0, sq, K, FD, FS, method="rrf"),
        "c legs + host": lambda: host_fusion(eng, q, sq),
        "d dense leg": lambda: eng.search64(q, FD),
        "e sparse leg": lambda: eng.search_batch_sparse(0, sq, FS),
    }
    times = {name: [] for name in calls}
    for fn in calls.values():  # warm-up: workspaces, shadows, code objects
        fn()
    for _ in range(args.iters):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, t in times.items():
        print(f"nq {nq:4d}  {name:16s} p50 {med[name] * 1e3:9.3f} ms  ({min(t) * 1e3:.3f} .. {max(t) * 1e3:.3f})", flush=True)
    print(f"nq {nq:4d}  a - (d + e) = {(med['a hybrid linear'] - med['d dense leg'] - med['e sparse leg']) * 1e3:+.3f} ms, "
          f"a - b = {(med['a hybrid linear'] - med['b hybrid rrf']) * 1e3:+.3f} ms, "
          f"a / c = {med['a hybrid linear'] / med['c legs + host']:.2f}", flush=True)
eng.close()
