#!/usr/bin/env python3
"""Metadata-filtered kNN waves: N x 768 cosine, k = 10, 256-query waves, at several selectivities.  Per selectivity, the
p50 wave time of
  unfiltered      eng.search(q, k)
  where (device)  eng.search(q, k, where=program): predicate kernel + masked search, the mask never leaves the device
  host mask       eng.search(q, k, mask=...): the mask built on the host beforehand (outside the timer), copied per call
and whether the where wave's ids equal the exact scan's under the same filter.  Then the QueryProcessor wave on a smaller
ArrayStorage corpus (--qp-rows): a Python callable `where` (host path) against the same filter as a dict (device path).
The predicate kernel's own time: run this under `rocprofv3 --kernel-trace --stats` (where_eval_kernel in the stats)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from mlvectordb_amd import ArrayStorage, Index, QueryProcessor, synth  # noqa: E402
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--selectivities", default="1,0.5,0.1,0.01,0.001")
ap.add_argument("--qp-rows", type=int, default=1_000_000, help="QueryProcessor corpus (0: skip)")
ap.add_argument("--qp-iters", type=int, default=3)
args = ap.parse_args()
N, D, K, B = args.rows, args.dim, args.k, args.batch
SCHEMA = {"sel": "int"}  # sel = label % 1000: {"sel": {"$lt": 1000 s}} matches a fraction s of the rows


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
sel = np.arange(N, dtype=np.int64) % 1000
eng.define_attr(0, "int64")
eng.set_attr(0, 0, sel)
q = synth.queries(B, D)
print(f"corpus {N} x {D} cosine, k={K}, batch {B}", flush=True)
base = p50(lambda: eng.search(q, K), args.iters)
print(f"unfiltered wave: {base:.3f} ms", flush=True)
for s in [float(x) for x in args.selectivities.split(",")]:
    f = {"sel": {"$lt": int(round(1000 * s))}}
    prog = W.compile_where(f, SCHEMA)
    mask = (sel < int(round(1000 * s))).astype(np.uint8)
    t_where = p50(lambda: eng.search(q, K, where=prog), args.iters)
    t_host = p50(lambda: eng.search(q, K, mask=mask), args.iters)
    lab, _, _ = eng.search(q, K, where=prog)
    hl, _, _ = eng.search(q, K, mask=mask)
    eng.set_strategy("exact")
    el, _, _ = eng.search(q, K, where=prog)
    eng.set_strategy("auto")
    print(f"selectivity {s:6.3%}: where {t_where:.3f} ms  host mask {t_host:.3f} ms  (delta {t_where - t_host:+.3f})  "
          f"ids == exact scan: {bool(np.array_equal(lab, el))}  == host mask: {bool(np.array_equal(lab, hl))}  "
          f"stats {eng.last_stats()['fallback_queries']} fallbacks", flush=True)
eng.close()

if args.qp_rows:
    n = args.qp_rows
    index = Index(space="cosine", attributes={"genre": "str", "year": "int"}, capacity_hint=n)
    qp = QueryProcessor(ArrayStorage(), index)
    rng = np.random.default_rng(0)
    genres = np.array(["jazz", "blues", "rock", "pop", "folk"])
    g = genres[rng.integers(len(genres), size=n)].tolist()
    y = rng.integers(1950, 2025, size=n).tolist()
    metas = [{"genre": a, "year": b} for a, b in zip(g, y)]
    qp.upsert_arrays(synth.corpus_rows(0, n, D), "ns", metadata=metas)
    f = {"genre": "jazz", "year": {"$gte": 2000}}
    pred = lambda m: m.get("genre") == "jazz" and m.get("year", -1) >= 2000  # noqa: E731
    t_dict = p50(lambda: qp.find_similar_many(q, K, "ns", where=f), args.qp_iters)
    t_call = p50(lambda: qp.find_similar_many(q, K, "ns", where=pred), args.qp_iters)
    same = [[h["id"] for h in r] for r in qp.find_similar_many(q, K, "ns", where=f)] == \
        [[h["id"] for h in r] for r in qp.find_similar_many(q, K, "ns", where=pred)]
    print(f"QueryProcessor {n} rows, {B}-query wave: callable where {t_call:.1f} ms  dict where {t_dict:.2f} ms  "
          f"same hits: {same}", flush=True)
