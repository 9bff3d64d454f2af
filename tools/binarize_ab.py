#!/usr/bin/env python3
"""Bit codes from the stored rows (include/mlvdb_project.h): N x 768 Gaussian rows in an ip index, --bits SimHash planes.
Alternating on one engine, per repetition:
  device   HipScanEngine.bits_project: the register-blocked fp64 tile kernel on the rows in HBM, codes written in place
  sign     the same call in sign mode (one bit per component), the bandwidth-bound kernel
  assign   the yardstick for the same arithmetic on the older kernels: assign_nearest of the same rows to --bits raw
           centroids (ip): bits / 8 launches of assign_scan_kernel at the same FMA count (plus its member listing)
  host     the route a user has without the call: get_rows of all rows, one sgemm and packbits in NumPy, bits_set back
           (--host-reps of them: it takes seconds)
The floor printed is rows x ld x bits FMAs over the vector fp64 rate of AMD's MI355X data sheet (78.6 TFLOP/s = 39.3 TFMA/s;
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
ap.add_argument("--bits", type=int, nargs="+", default=[256])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-reps", type=int, default=1)
args = ap.parse_args()

from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

N, D = args.rows, args.dim
FMA_PER_S = 39.3e12
SIG, WIDE = 0, 1


def line(name, t):
    return f"  {name:8s}: median {np.median(t):9.2f} ms  min {min(t):9.2f}  max {max(t):9.2f}"


rng = np.random.default_rng(1)
eng = HipScanEngine(D, "ip", device=0, capacity_hint=N)
for s in range(0, N, 250_000):
    eng.append(rng.standard_normal((min(250_000, N - s), D), dtype=np.float32))
eng.define_attr(SIG, "bits")
eng.define_attr(WIDE, "bits")
sign_bits = (D + 63) // 64 * 64
for nbits in args.bits:
    planes = np.random.default_rng(nbits).standard_normal((nbits, D)).astype(np.float32)
    print(f"corpus {N} x {D} ip, {nbits} planes, {args.reps} alternated repetitions", flush=True)
    dev, sign, assign = [], [], []
    for rep in range(args.reps + 1):  # (the first repetition warms every route up and is not counted)
        t0 = time.perf_counter()
        assert eng.bits_project(SIG, planes, nbits) == N
        t1 = time.perf_counter()
        assert eng.bits_project(WIDE, None, sign_bits) == N
        t2 = time.perf_counter()
        done = eng.assign_nearest(None, planes)[2] if nbits <= 1024 else N
        t3 = time.perf_counter()
        assert done == N
        if rep:
            dev.append((t1 - t0) * 1e3)
            sign.append((t2 - t1) * 1e3)
            assign.append((t3 - t2) * 1e3)
        if rep % 4 == 3:
            eng.compact()  # (no row is tombstoned: the identity, and the pools shed the overwritten codes)
    floor = N * ((D + 15) // 16 * 16) * nbits / FMA_PER_S * 1e3
    print(line("device", dev) + f"   fp64 FMA floor {floor:.2f} ms = {floor / np.median(dev):.1%} of the call", flush=True)
    print(line("sign", sign) + f"   {N * D * 4 / np.median(sign) / 1e9:.2f} TB/s of rows", flush=True)
    if nbits <= 1024:
        print(line("assign", assign) + f"   assign / device {np.median(assign) / np.median(dev):.2f}", flush=True)
    host = []
    for rep in range(args.host_reps):
        t0 = time.perf_counter()
        x = np.concatenate([eng.get_rows(s, min(250_000, N - s)) for s in range(0, N, 250_000)])
        words = np.ascontiguousarray(np.packbits(x @ planes.T > 0, axis=1, bitorder="little")).view("<u8").astype(np.uint64)
        eng.bits_set(SIG, 0, W.BitsColumn(words, np.ones(N, np.uint8)))
        host.append((time.perf_counter() - t0) * 1e3)
        del x
    if host:
        print(line("host", host) + f"   host / device {np.median(host) / np.median(dev):.0f}", flush=True)
        got = eng.bits_get(SIG, 0, 4096)[1].reshape(4096, -1)
        eng.bits_project(SIG, planes, nbits)
        same = eng.bits_get(SIG, 0, 4096)[1].reshape(4096, -1)
        diff = sum(bin(int(v)).count("1") for v in (got ^ same).ravel())
        print(f"  fp32 sgemm against the fp64 contract over 4,096 rows: {diff} of {4096 * nbits} bits differ", flush=True)
eng.close()
