"""Metadata filters on the MI355X at their limits: the single-program and the per-query kernels against the NumPy
evaluator (tests/where_helpers.py: eval_program) on hostile column values, raw programs at the validated limits, row counts
that only large indexes reach, many columns and set tables in one call, the largest dynamic-LDS requests, and the gathered
kernel at every query-tile width.  kNN answers are checked against the fp64 oracle over the matching rows and, bit for
bit, against one single-program call per query."""
import numpy as np
import pytest

from mlvectordb_amd import Index, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from mlvectordb_amd.vector import Vector
from oracle import exact_scan
from tests.conftest import dump_mismatch
from tests.where_helpers import (SCHEMA, eval_program, hostile_columns, program_depth, py_match, random_filter,
                                 random_metadata, random_raw_program)

pytestmark = pytest.mark.gpu

ALWAYS = 1 << 30  # WHERE_GATHER that gathers every program when k <= 64


def _hostile_engine(rng, n, d, kinds, space="l2"):
    """n random rows with the columns `kinds` (attr -> kind) of hostile values; ~10 % of the rows tombstoned."""
    rows = rng.standard_normal((n, d), dtype=np.float32)
    eng = HipScanEngine(d, space, device=0)
    eng.append(rows)
    cols = hostile_columns(rng, n, kinds)
    for a, kind in kinds.items():
        eng.define_attr(a, kind)
        eng.set_attr(a, 0, cols[a])
    tomb = rng.random(n) < 0.1
    eng.tombstone(np.flatnonzero(tomb))
    return eng, rows, cols, tomb


def _kinds(rng, attrs):
    """Column kinds for `attrs`, both kinds present whenever there are two columns or more."""
    kinds = {int(a): ("int64", "float64")[i % 2] for i, a in enumerate(attrs)}
    return {a: kinds[a] for a in rng.permutation(list(kinds)).tolist()}


def _dump_program(tag, prog, cols, rows_at, **extra):
    dump_mismatch(tag, ops=prog.ops, set=prog.set, rows_at=rows_at,
                  **{f"col{a}": c[rows_at] for a, c in cols.items()}, **extra)


# ---------------------------------------------------------------- (a) seeded raw-program fuzz, both kernels
# Row counts: a single row, one wave short / exact / over, a few waves; 1,048,577 rows is one past the 4096 x 256 rows of
# the single-program kernel's grid (its grid-stride loop's second pass) and cuts the per-query kernels' rows into
# 320-row segments with a ragged last one; 262,145 rows gives 128-row segments.
FUZZ_ROWS = (1, 63, 64, 65, 257, 1_048_577, 1, 63, 64, 65, 257, 1_048_577, 4097, 262_145, 64, 1)


@pytest.mark.parametrize("seed", range(16))
def test_raw_program_fuzz_equals_numpy(seed):
    n = FUZZ_ROWS[seed]
    rng = np.random.default_rng(5000 + seed)
    ncols = 16 if seed % 4 == 0 or n > 1_000_000 else int(rng.integers(1, 17))
    kinds = _kinds(rng, rng.choice(W.MAX_ATTRS, ncols, replace=False))
    eng, _, cols, tomb = _hostile_engine(rng, n, 3, kinds)
    try:
        for a, kind in kinds.items():  # the columns hold the pools bit for bit (NaN payloads, -0.0, subnormals)
            back = eng.get_attr(a, 0, n, np.float64 if kind == "float64" else np.int64)
            assert np.array_equal(back.view(np.int64), cols[a].view(np.int64)), f"attr {a}"
        # up to 64 programs, at most 1024 ops in all (one per-query call): the first reaches stack depth 32 in 64 ops,
        # the second is 64 ops as well, the rest are short or 64 ops
        programs, budget = [], W.EACH_MAX_OPS
        while len(programs) < W.EACH_MAX_PROGRAMS:
            j = len(programs)
            size = 64 if j < 2 or rng.random() < 0.15 else int(rng.integers(1, 24))
            if size > budget:
                break
            programs.append(random_raw_program(rng, kinds, size, deep=(j == 0 or rng.random() < 0.1)))
            budget -= size
        assert program_depth(programs[0]) == W.MAX_DEPTH and programs[0].ops.size == programs[1].ops.size == W.MAX_OPS
        want = [eval_program(p, cols, n) & ~tomb for p in programs]
        counts = [int(w.sum()) for w in want]
        got = eng.count_each(programs)
        if got.tolist() != counts:
            bad = int(np.flatnonzero(got != np.array(counts))[0])
            dump_mismatch(f"where_limits_fuzz_each_{seed}", got=got, want=np.array(counts))
            pytest.fail(f"seed {seed} (n={n}): count_each of program {bad}: {got[bad]}, NumPy {counts[bad]}")
        for j, (p, w) in enumerate(zip(programs, want)):
            c = eng.where_count(p)
            lab = eng.where_labels(p)
            ref = np.flatnonzero(w)
            if c != counts[j] or not np.array_equal(lab, ref):
                diff = np.setxor1d(lab, ref)[:64]
                _dump_program(f"where_limits_fuzz_{seed}_{j}", p, cols, diff, got=lab, want=ref)
                pytest.fail(f"seed {seed} (n={n}) program {j}: where_count {c} / {lab.size} labels, NumPy {counts[j]}")
        # the pools must exercise the programs: across the seed, some programs match nothing and some match rows
        if n > 1000:
            assert min(counts) == 0 < max(counts), counts
    finally:
        eng.close()


# ---------------------------------------------------------------- (b) per-query kNN, many columns and set tables
def _check_each(eng, rows, qs, k, programs, of, masks, space, tag):
    """search_each against the fp64 oracle over each query's matching rows, and bit for bit against one
    search64(where=program) per program (search64 without a filter for the queries of no program) -> routes."""
    lab, dist, cnt, d64, routes = eng.search_each(qs, k, programs, of, want64=True, return_routes=True)
    for p in range(-1, len(programs)):
        sel = np.flatnonzero(of == p)
        if not sel.size:
            continue
        sl, sd, sc, s64 = eng.search64(qs[sel], k, where=None if p < 0 else programs[p])
        same = np.array_equal(lab[sel], sl) and np.array_equal(cnt[sel], sc) and np.array_equal(dist[sel], sd) and \
            np.array_equal(d64[sel].view(np.int64), s64.view(np.int64))
        idx = np.flatnonzero(masks[p])
        ol, od, oc = exact_scan.knn(qs[sel], rows[idx], k, space)
        ol = np.append(idx, -1)[ol]  # positions among the matching rows -> labels (padding -1 stays -1)
        exact = np.array_equal(lab[sel], ol) and np.array_equal(cnt[sel], oc) and \
            np.allclose(dist[sel], od, atol=1e-5, rtol=0)
        if not (same and exact):
            dump_mismatch(f"where_limits_{tag}_p{p}", lab=lab[sel], sl=sl, ol=ol, cnt=cnt[sel], sc=sc, oc=oc,
                          d64=d64[sel], s64=s64, od=od)
        assert same, f"{tag} program {p} (route {routes[p] if p >= 0 else '-'}): differs from the single calls"
        assert exact, f"{tag} program {p} (route {routes[p] if p >= 0 else '-'}): differs from the oracle"
    return routes


def test_per_query_knn_over_many_columns_and_set_tables():
    rng = np.random.default_rng(64)
    n, d, space = 20_000, 48, "l2"
    kinds = _kinds(rng, np.arange(12))  # 6 int64 and 6 float64 columns
    eng, rows, cols, tomb = _hostile_engine(rng, n, d, kinds, space)
    try:
        # 64 programs of 4..16 ops (<= 1024 in all), each with its own set table, no two of the same length
        programs, seen = [], set()
        while len(programs) < W.EACH_MAX_PROGRAMS:
            p = random_raw_program(rng, kinds, int(rng.integers(4, 17)), p_in=0.35)
            if p.set.size not in seen and (p.ops["op"] == W.IN).any():
                seen.add(p.set.size)
                programs.append(p)
        assert sum(p.ops.size for p in programs) <= W.EACH_MAX_OPS
        used = {int(a) for p in programs for o, a in zip(p.ops["op"], p.ops["attr"]) if W.EQ <= o <= W.EXISTS}
        assert used == set(kinds), used
        masks = {p: eval_program(prog, cols, n) & ~tomb for p, prog in enumerate(programs)}
        masks[-1] = ~tomb
        matching = [int(masks[p].sum()) for p in range(len(programs))]
        assert sum(m > 0 for m in matching) >= 16 and 0 in matching, matching
        of = np.concatenate([np.repeat(np.arange(len(programs), dtype=np.int32), 2), np.full(6, -1, np.int32)])
        of = of[rng.permutation(of.size)]
        qs = rng.standard_normal((of.size, d), dtype=np.float32)
        assert eng.count_each(programs).tolist() == matching
        for gather in (0, ALWAYS):
            eng.set_tuning(WHERE_GATHER=gather)
            for k in (10, 64):
                routes = _check_each(eng, rows, qs, k, programs, of, masks, space, f"many_{gather}_{k}")
                want = [_native.ROUTE_NONE if m == 0 else _native.ROUTE_SCAN if gather == 0 else _native.ROUTE_GATHER
                        for m in matching]
                assert routes.tolist() == want, (gather, k)
    finally:
        eng.close()


# ---------------------------------------------------------------- (c) the evaluation kernel's largest LDS
def test_evaluation_lds_grows_within_one_process():
    """1024 ops over 8 columns needs 49,424 B of dynamic LDS, 1024 ops over 16 columns 65,808 B (the most a call can ask
    for): the larger call comes second, after the kernel was configured for a call above 48 KiB."""
    rng = np.random.default_rng(1024)
    n = 5000
    kinds = _kinds(rng, np.arange(W.MAX_ATTRS))
    eng, rows, cols, tomb = _hostile_engine(rng, n, 8, kinds)
    try:
        for width in (8, 16):
            sub = {a: kinds[a] for a in list(kinds)[:width]}
            programs = [random_raw_program(rng, sub, W.MAX_OPS, deep=(j % 4 == 0), p_in=0.3) for j in range(16)]
            used = {int(a) for p in programs for o, a in zip(p.ops["op"], p.ops["attr"]) if W.EQ <= o <= W.EXISTS}
            assert used == set(sub) and sum(p.ops.size for p in programs) == W.EACH_MAX_OPS
            want = [int((eval_program(p, cols, n) & ~tomb).sum()) for p in programs]
            got = eng.count_each(programs).tolist()
            assert got == want, f"{width} columns"
            of = np.arange(16, dtype=np.int32)
            qs = rng.standard_normal((16, 8), dtype=np.float32)
            masks = {p: eval_program(prog, cols, n) & ~tomb for p, prog in enumerate(programs)}
            eng.set_tuning(WHERE_GATHER=ALWAYS)
            _check_each(eng, rows, qs, 5, programs, of, masks, "l2", f"lds_{width}")
    finally:
        eng.close()


# ---------------------------------------------------------------- (d) the gathered kernel at every tile width
MANY = 64 * 64 + 404  # live matches of the widest program: past 64 chunks of 64 rows


def _gather_step(space, d, k, seed):
    """One index of width d: programs that match nothing, fewer than k, exactly k and MANY rows, 1..5 queries each, all
    gathered; against the oracle and the single calls."""
    rng = np.random.default_rng(seed)
    fewer = k // 2 if k > 1 else 0
    sizes = {10: MANY + 300, 11: fewer, 12: k, 13: 1500}  # group -> rows (group 10: 300 of them tombstoned)
    group = np.concatenate([np.full(m, g, np.int64) for g, m in sizes.items()])
    group = group[rng.permutation(group.size)]
    n = group.size
    rows = rng.standard_normal((n, d), dtype=np.float32)
    score = rng.standard_normal(n)
    score[rng.random(n) < 0.2] = np.nan
    eng = HipScanEngine(d, space, device=0)
    try:
        eng.append(rows)
        eng.define_attr(0, "int64")
        eng.define_attr(5, "float64")
        eng.set_attr(0, 0, group)
        eng.set_attr(5, 0, score)
        tomb = np.zeros(n, bool)
        tomb[rng.choice(np.flatnonzero(group == 10), 300, replace=False)] = True
        tomb[rng.choice(np.flatnonzero(group == 13), 100, replace=False)] = True
        eng.tombstone(np.flatnonzero(tomb))
        cols = {0: group, 5: score}
        op = lambda o, attr=0, a=0, b=0: (o, attr, a, b)  # noqa: E731
        none_set = np.zeros(0, np.int64)
        programs = [
            W.Program(np.array([op(W.EQ, 0, 99)], W.OP_DTYPE), none_set),                       # nothing
            W.Program(np.array([op(W.EQ, 0, 11)], W.OP_DTYPE), none_set),                       # fewer than k
            W.Program(np.array([op(W.IN, 0, 1, 1)], W.OP_DTYPE), np.array([9, 12], np.int64)),  # exactly k
            W.Program(np.array([op(W.GE, 0, 10), op(W.LE, 0, 10), op(W.AND)], W.OP_DTYPE), none_set),  # MANY
            W.Program(np.array([op(W.EQ, 0, 13), op(W.LT, 5, W.float_bits(0.25)), op(W.AND)], W.OP_DTYPE), none_set),
        ]
        masks = {p: eval_program(prog, cols, n) & ~tomb for p, prog in enumerate(programs)}
        masks[-1] = ~tomb
        assert [int(masks[p].sum()) for p in range(4)] == [0, fewer, k, MANY]
        nq_of = rng.integers(1, 6, len(programs))
        of = np.concatenate([np.full(m, p, np.int32) for p, m in enumerate(nq_of)] + [np.full(2, -1, np.int32)])
        of = of[rng.permutation(of.size)]
        qs = rng.standard_normal((of.size, d), dtype=np.float32)
        eng.set_tuning(WHERE_GATHER=ALWAYS)
        routes = _check_each(eng, rows, qs, k, programs, of, masks, space, f"gather_{space}_{d}_{k}")
        want = [_native.ROUTE_GATHER if masks[p].any() else _native.ROUTE_NONE for p in range(len(programs))]
        assert routes.tolist() == want
    finally:
        eng.close()


# Within each band of the query tile (4 queries up to ld 2048, 2 up to 4096, 1 up to 8192) one space, so that both
# widths run the same kernel instance: first an ld above 1536 (more than 48 KiB of LDS), then the band's widest.
@pytest.mark.parametrize("space,steps", [
    ("l2", ((1600, 7), (2048, 64))),     # qt = 4
    ("cosine", ((3100, 63), (4096, 1))),  # qt = 2
    ("ip", ((6200, 64), (8192, 7))),      # qt = 1
], ids=["qt4", "qt2", "qt1"])
def test_gathered_kernel_at_every_tile_width(space, steps):
    for d, k in steps:
        _gather_step(space, d, k, seed=d + k)


@pytest.mark.parametrize("space,d,k", [("l2", 1, 63), ("cosine", 17, 1), ("ip", 130, 64), ("l2", 130, 7)])
def test_gathered_kernel_pads_narrow_rows(space, d, k):
    _gather_step(space, d, k, seed=d * 7 + k)


# ---------------------------------------------------------------- (e) dict filters, from the Index to the device
def test_dict_filters_through_the_index_equal_the_dict_semantics():
    rng = np.random.default_rng(200)
    d, n = 8, 4000
    index = Index(space="l2", attributes=SCHEMA)
    try:
        vecs = [Vector(values=rng.standard_normal(d).astype(np.float32), metadata=m) for m in random_metadata(rng, n)]
        index.add(vecs[:2500], "ns")
        index.add(vecs[2500:], "ns")
        gone = {v.id for v in vecs[::9]}
        index.remove(list(gone), "ns")
        live = [v for v in vecs if v.id not in gone]
        filters = [random_filter(rng) for _ in range(200)]
        wants = []
        for f in filters:
            want = [v.id for v in live if py_match(f, v.metadata)]
            assert index.query_by_metadata("ns", f) == want, f
            assert index.count("ns", f) == len(want), f
            wants.append(len(want))
        assert index.count_many("ns", filters) == wants
        assert 0 in wants and len(live) in wants and any(0 < w < len(live) for w in wants)
    finally:
        index.close()
