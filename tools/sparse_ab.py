#!/usr/bin/env python3
"""Sparse vector search at size (include/mlvdb_sparse.h): --rows rows whose sparse vectors hold about --row-len nonzeros
out of a vocabulary of --vocab terms (a skewed draw: a few terms are common, most are rare), queries of about --query-len
terms drawn the same way.  Wall-clock p50 per call of search_batch_sparse, the host's share included (tile packing, the
uploads, the answers' copy back), for 1 / 8 / 64 / 256 queries at k = 10, and next to it the bytes the scan must move --
8 * (summed row lengths) + 12 * rows per tile pass, times the call's tiles -- divided by that time, against the 8 TB/s of
HBM.  Whether the LDS lookups or HBM bound the kernel is what this is for; a later tile of another query rereads the rows
from L2 / MALL where they fit, so the figure can pass the HBM roof.  The kernel reads the column, the norms and the pool,
never the rows: --dim only sizes the corpus."""
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
ap.add_argument("--dim", type=int, default=16)
ap.add_argument("--vocab", type=int, default=30_522)
ap.add_argument("--row-len", type=int, default=64)
ap.add_argument("--query-len", type=int, default=32)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
N, V = args.rows, args.vocab
QT, MAX_UNION = 8, 1024  # kSparseQT, kSparseMaxUnion


def p50(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


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


def tiles(q: W.SparseColumn) -> int:
    """The tiles the library packs these queries into: greedily, <= QT queries and <= MAX_UNION terms in their union."""
    count, size, union = 0, 0, set()
    for i in range(len(q)):
        t = set(q.terms[q.offsets[i]:q.offsets[i + 1]].tolist())
        if size and (size == QT or len(union | t) > MAX_UNION):
            count, size, union = count + 1, 0, set()
        union |= t
        size += 1
    return count + 1


rng = np.random.default_rng(0)
eng = HipScanEngine(args.dim, "ip", device=0, capacity_hint=N)
eng.define_attr(0, "sparse")
step = 100_000
for first in range(0, N, step):
    n = min(step, N - first)
    eng.append(rng.standard_normal((n, args.dim), dtype=np.float32))
    eng.set_attr_sparse(0, first, vectors(rng, n, args.row_len, 255))
used, live = eng.list_stats(0)
per_pass = 8 * live + 12 * N
print(f"{N} rows, vocabulary {V}, {live / N:.1f} nonzeros per row, pool {used} elements, {per_pass / 1e6:.1f} MB per tile pass",
      flush=True)
for nq in (1, 8, 64, 256):
    q = vectors(rng, nq, args.query_len, 1024)
    nt = tiles(q)
    med, lo, hi = p50(lambda: eng.search_batch_sparse(0, q, args.k), args.iters)
    print(f"nq {nq:4d}  {nt:3d} tiles  p50 {med * 1e3:9.3f} ms  ({lo * 1e3:.3f} .. {hi * 1e3:.3f})  "
          f"{nt * per_pass / med / 1e12:6.3f} TB/s of the 8 TB/s roof  {nq / med:10.0f} queries/s", flush=True)
eng.close()
