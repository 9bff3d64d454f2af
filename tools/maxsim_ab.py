#!/usr/bin/env python3
"""Late-interaction search (include/mlvdb_maxsim.h): N x 768 cosine (synth.py's bench corpus), one query of T = 32 tokens,
k = 10.

Document columns: label // S for S rows per document (--doc-sizes; contiguous chunks of a document; a column of more than
2^20 documents is refused by the call: the tool says so and goes on), one skewed column -- the 10-row column in which a single
document also holds a random 1 % of the rows -- and the 10-row column with its rows scattered over the corpus (a random
permutation).  Per
column the p50 of
  yardstick         the same T tokens as T plain queries through search() with the exact strategy on the same handle: the
                    exact scan of the same rows with the top-k lists as its sink, k = 10, the same number of 8-query passes
  maxsim            search_maxsim without matches, and its ratio to the yardstick; `scan` is the scan kernel's own time from
                    the handle's statistics, `rest` everything else of the call (documents, row -> document pass, presetting
                    the cells, ranking, copies)
  documents         facet_values() of the same column at max_values 2^20 on its own: the call's document stage (device pass,
                    the copy of the G codes and their sort on the host); `rest` also holds the host's table of G codes
  matches           what want_matches adds (the member stage over T x k pairs)
Run each GPU step of a job under `timeout`."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--tokens", type=int, default=32)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--doc-sizes", default="1,10,100,10000")
ap.add_argument("--no-skewed", action="store_true")
ap.add_argument("--no-scattered", action="store_true")
args = ap.parse_args()

from mlvectordb_amd import synth  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine, MaxSimOverflow  # noqa: E402

N, D, K, T = args.rows, args.dim, args.k, args.tokens


def p50(fn, iters):
    fn()
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


eng = HipScanEngine(D, "cosine", device=0, capacity_hint=N)
for _, rows in synth.iter_corpus(0, N, D, threads=16):
    eng.append(rows)
del rows
eng.define_attr(0, "int64")
labels = np.arange(N, dtype=np.int64)
tokens = synth.queries(T, D)
offsets = np.array([0, T], np.int64)
print(f"corpus {N} x {D} cosine, T={T}, k={K}", flush=True)

eng.set_strategy("exact")
yard = p50(lambda: eng.search(tokens, K), args.iters)
eng.set_strategy("auto")
print(f"{'yardstick (exact scan, top-k)':34s}: {yard:9.3f} ms", flush=True)

columns = [(f"{s} rows/document", labels // int(s)) for s in args.doc_sizes.split(",")]
if not args.no_skewed:
    skew = labels // 10
    skew[np.random.default_rng(0).choice(N, N // 100, replace=False)] = -7
    columns.append(("skewed (one document = 1 %)", skew))
if not args.no_scattered:
    columns.append(("10 rows/document, scattered", np.random.default_rng(1).permutation(labels // 10)))
eng.set_profiling(True)
for name, col in columns:
    eng.set_attr(0, 0, col)
    try:
        grp, _, cnt, _, _, _ = eng.search_maxsim(tokens, offsets, K, 0)
    except MaxSimOverflow as e:
        print(f"{name:34s}: refused ({e})", flush=True)
        continue
    ndocs = int(np.unique(col).size)
    eng.last_stats()
    t = p50(lambda: eng.search_maxsim(tokens, offsets, K, 0), args.iters)
    scan = eng.last_stats()["scan_ms"] / (args.iters + 1)
    tm = p50(lambda: eng.search_maxsim(tokens, offsets, K, 0, want_matches=True), args.iters)
    td = p50(lambda: eng.facet_values(0, 1 << 20), args.iters)
    eng.last_stats()
    print(f"{name:34s}: G {ndocs:8d}  maxsim {t:9.3f} ms  x{t / yard:5.2f} of the yardstick  scan {scan:9.3f} ms  "
          f"x{scan / yard:5.2f}  rest {t - scan:8.3f} ms  documents {td:8.3f} ms  matches add {tm - t:8.3f} ms  "
          f"documents returned {int(cnt[0])}", flush=True)
eng.close()
