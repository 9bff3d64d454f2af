#!/usr/bin/env python3
"""Updates and deletes by filter on an N x 64 index with one int64 "tenant" column of 40 values (include/mlvdb_mutate.h).

  step update   per-call time of update_where -- one predicate column, one assignment -- at 100 %, 2.5 % and one-row
                selectivity, against where_count of the same filter in the same process: the floor, one pass and no stores.
  step remove   remove_where of one tenant on twin A (tombstone_where: one native call) against the composition
                where_labels + tombstone on twin B, alternating tenant by tenant in one process.  Each deletion is
                destructive, so every tenant is used once per twin.

Without --step both run, each as a child process under its own time limit; the first failure stops the tool.  Every time is
a host clock around a call that ends in a device synchronisation; medians with the 10th / 90th percentile and the range."""
import argparse
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--tenants", type=int, default=40)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--step", choices=["update", "remove"])
ap.add_argument("--step-timeout", type=int, default=240, help="seconds each step may take")
args = ap.parse_args()
N, D, T = args.rows, args.dim, args.tenants

if args.step is None:
    for step in ("update", "remove"):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, __file__, "--step", step, "--rows", str(N),
               "--dim", str(D), "--tenants", str(T), "--iters", str(args.iters)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"step {step} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

from mlvectordb_amd import _native, synth  # noqa: E402
from mlvectordb_amd import where as W  # noqa: E402
from mlvectordb_amd.engine import HipScanEngine  # noqa: E402

SCHEMA = {"tenant": "int", "flag": "int"}


def spread(ms):
    ms = np.asarray(ms) * 1e3
    return (f"median {np.median(ms):.3f} ms  p10 {np.percentile(ms, 10):.3f}  p90 {np.percentile(ms, 90):.3f}  "
            f"min {ms.min():.3f}  max {ms.max():.3f}  (n={ms.size})")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def build(tenant, twins=1):
    engines = [HipScanEngine(D, "cosine", device=0, capacity_hint=N) for _ in range(twins)]
    for _, rows in synth.iter_corpus(0, N, D, threads=16):
        for eng in engines:
            eng.append(rows)
    for eng in engines:
        eng.define_attr(0, "int64")
        eng.define_attr(1, "int64")
        eng.set_attr(0, 0, tenant)
    return engines


tenant = (np.arange(N, dtype=np.int64) * 2654435761 >> 7) % T  # 40 tenants of ~2.5 % each, interleaved
print(f"index {N} x {D}, {T} tenants", flush=True)

if args.step == "update":
    tenant[N // 2] = T  # one row of a tenant of its own
    eng, = build(tenant)
    cases = [("100 %", {"tenant": {"$gte": 0}}), (f"{100 / T:.1f} %", {"tenant": 3}), ("one row", {"tenant": T})]
    for name, f in cases:
        prog = W.compile_where(f, SCHEMA)
        want = int((tenant >= 0).sum() if "$gte" in str(f) else (tenant == f["tenant"]).sum())
        for _ in range(5):  # warm both
            assert eng.where_count(prog) == want
            assert eng.update_where(prog, [(1, _native.SET_ASSIGN, 0)]) == (want, 0)
        t_count, t_assign, t_add = [], [], []
        for i in range(args.iters):  # alternating, in one process
            t_count.append(timed(lambda: eng.where_count(prog))[0])
            t_assign.append(timed(lambda: eng.update_where(prog, [(1, _native.SET_ASSIGN, i)]))[0])
            t_add.append(timed(lambda: eng.update_where(prog, [(1, _native.SET_ADD, 1)]))[0])
        flag = eng.get_attr(1, 0, N)
        hit = (tenant >= 0) if "$gte" in str(f) else (tenant == f["tenant"])
        assert (flag[hit] == args.iters).all(), "the last assignment + its increment did not land on the matching rows"
        print(f"selectivity {name} ({want} rows)", flush=True)
        print(f"  where_count (floor: one pass, no stores)   {spread(t_count)}", flush=True)
        print(f"  update_where, one ASSIGN (one pass)        {spread(t_assign)}", flush=True)
        print(f"  update_where, one ADD (count pass + store) {spread(t_add)}", flush=True)
    eng.close()
else:
    a, b = build(tenant, twins=2)
    t_fused, t_comp = [], []
    for t in range(T):
        prog = W.compile_where({"tenant": t}, SCHEMA)
        want = np.flatnonzero(tenant == t)
        first, second = (("a", "b"), ("b", "a"))[t % 2]  # who goes first alternates too
        for which in (first, second):
            if which == "a":
                dt, got = timed(lambda: a.tombstone_where(prog))
                t_fused.append(dt)
            else:
                dt, got = timed(lambda: b.tombstone(b.where_labels(prog)))
                t_comp.append(dt)
                got = want if got == want.size else None
            assert got is not None and np.array_equal(got, want), f"tenant {t}, twin {which}"
        assert a.counts() == b.counts()
    # the first tenant of each twin carries the first launches: reported apart from the steady state
    print(f"remove_where of one tenant (~{N // T} rows), {T - 2} tenants after two warm-ups each", flush=True)
    print(f"  tombstone_where (twin A)               {spread(t_fused[2:])}", flush=True)
    print(f"  where_labels + tombstone (twin B)      {spread(t_comp[2:])}", flush=True)
    print(f"  first two calls: fused {t_fused[0] * 1e3:.3f} / {t_fused[1] * 1e3:.3f} ms, "
          f"composition {t_comp[0] * 1e3:.3f} / {t_comp[1] * 1e3:.3f} ms", flush=True)
    a.close()
    b.close()
