"""Inputs and comparisons for the magnitude tests (tests/test_magnitudes_host.py, tests/test_gpu_magnitudes.py and, for the
search families built on the primitives, tests/test_magnitudes_families_host.py, tests/test_gpu_magnitudes_families.py):
corpora whose components span the whole finite float32 range, every one built from a seed, and the bars an answer is held to.

The reference of every comparison is oracle.exact_scan (fp64 from the fp32 inputs: no finite float32 input overflows it).
Nothing here needs a GPU.
"""
from __future__ import annotations

import functools
import json
import os
import types

import numpy as np

from mlvectordb_amd import where as W
from oracle import exact_scan
from tests.helpers import SCORE_ATOL, deleted_mask, make_case

SPACES = ("l2", "cosine", "ip")
F32_MAX = np.finfo(np.float32).max
FP64_RTOL = 1e-12  # tests/test_gpu_parity.py::test_device_pointer_entry_and_fp64_distances, scaled by the summed terms below

# the magnitude window of the filter path (DESIGN "Magnitudes"; csrc/internal.h: norm_window_lo / _hi): norms of non-zero rows
FILTER_WINDOW = {"cosine": (2.0 ** -100, 2.0 ** 120), "ip": (2.0 ** -63, 2.0 ** 90), "l2": (2.0 ** -63, 2.0 ** 48)}


def inside_filter_window(rows, space: str) -> bool:
    """Do the fp64 norms of all non-zero rows lie inside the window of ``space``, with a float's rounding to spare?"""
    lo, hi = FILTER_WINDOW[space]
    r = np.asarray(rows, dtype=np.float64)
    norms = np.sqrt(np.einsum("ij,ij->i", r, r))
    nz = norms[norms > 0]
    return nz.size == 0 or bool(nz.min() >= lo * (1 + 1e-6) and nz.max() <= hi * (1 - 1e-6))


def queries_leaving_window(qs, rows, space: str) -> np.ndarray:
    """Which queries the filter path hands to its exact fallback on an index inside the window (csrc/kernels_filter.hip:
    query_leaves_window): a non-zero query whose norm lies outside the window, and a cosine / ip query whose largest possible
    score against the index (ip: |q| max|x|) is below 2**-24, where ``1 - s`` ties rows the filter tells apart."""
    lo, hi = FILTER_WINDOW[space]
    q = np.asarray(qs, dtype=np.float64)
    r = np.asarray(rows, dtype=np.float64)
    qn = np.sqrt(np.einsum("ij,ij->i", q, q))
    xmax = float(np.sqrt(np.einsum("ij,ij->i", r, r)).max(initial=0.0))
    out = (qn < lo) | (qn > hi)
    if space == "ip":
        out |= qn * xmax < 2.0 ** -24
    elif space == "cosine":
        out |= (qn / (qn + 1e-30)) * (xmax / (xmax + 1e-30)) < 2.0 ** -24
    return out & (qn > 0)


# ---------------------------------------------------------------- odd queries on an ordinary index
MIXED_SEED, MIXED_N, MIXED_ORDINARY = 31, 3000, 8
MIXED_DIMS = (64, 100, 256)
MIXED_KS = (10, 100)
MIXED_ODD = ("x 2**-140", "x 2**120", "FLT_MAX component")
MIXED_ODD_AT = (1, 4, 9)  # where the odd queries stand in the batch of eleven
MIXED_ODD_ONLY = ((0,), (1,), (2,), (0, 1), (1, 2))  # the batches of one and two odd queries, by their index in MIXED_ODD


@functools.lru_cache(maxsize=4)
def mixed_inputs(d: int):
    """An N(0,1) index (3000 rows, duplicates, 5 % tombstoned: inside every window) and a batch of eleven queries: eight ordinary
    ones and, at positions 1, 4 and 9, an N(0,1) query x 2**-140, one x 2**120 and one with a component set to FLT_MAX -- each
    outside the window of every space, each sharing its pass with ordinary queries.  Returns (rows, qs, deleted)."""
    rows, base = make_case(MIXED_SEED, MIXED_N, d, MIXED_ORDINARY + len(MIXED_ODD), dup=True)
    odd = base[MIXED_ORDINARY:].copy()
    odd[0] *= pow2(-140)
    odd[1] *= pow2(120)
    odd[2, 3 % d] = F32_MAX
    qs = np.insert(base[:MIXED_ORDINARY], [MIXED_ODD_AT[i] - i for i in range(len(MIXED_ODD))], odd, axis=0)
    assert all(np.array_equal(qs[at], odd[i]) for i, at in enumerate(MIXED_ODD_AT))
    deleted = deleted_mask(MIXED_SEED, MIXED_N, 0.05)
    assert np.isfinite(rows).all() and np.isfinite(qs).all()
    for a in (rows, qs, deleted):
        a.setflags(write=False)
    return rows, qs, deleted


def mixed_radius(d: int, space: str) -> float:
    """The range radius of the mixed batch: the mean 10th-nearest distance of its ordinary queries."""
    rows, qs, deleted = mixed_inputs(d)
    ordinary = np.delete(np.arange(qs.shape[0]), MIXED_ODD_AT)
    return range_radius(qs[ordinary], rows, space, deleted)


# ---------------------------------------------------------------- uniform scale: the whole corpus in other units
UNIFORM_EXPONENTS = (-140, -126, -100, -64, -40, -20, 40, 63, 64, 100, 124)
UNIFORM_DIMS = (64, 100, 256)
UNIFORM_SEED, UNIFORM_N, UNIFORM_NQ, UNIFORM_K, UNIFORM_BIG_K = 7, 3000, 70, 10, 100
UNIFORM_BATCHES = (2, 12, 70)  # the 1-2-query chain, the narrow kernel, a pass of 8 query tiles
# range: the spaces and scales at which a radius is a float32
RANGE_EXPONENTS = {"cosine": UNIFORM_EXPONENTS, "l2": (-70, -64, -40, 40, 60), "ip": (-20, 20)}
# d = 64 (bf16 body) and 256 (int8-only index); l2 at 2**60 only at d = 64: over 256 columns the 10th-nearest distance,
# about 2 d 2**120, is past FLT_MAX and no float32 radius exists
RANGE_CASES = tuple((d, s, e) for d in (64, 256) for s in ("cosine", "l2", "ip") for e in RANGE_EXPONENTS[s]
                    if not (d == 256 and s == "l2" and e == 60))
RANGE_NQ = 12
RANGE_MAX_HITS = 16_384


def pow2(e: int) -> np.float32:
    """float32(2)**e, subnormal below e = -126 (ldexp: no pow() in the way)."""
    v = np.ldexp(np.float32(1), int(e)).astype(np.float32)
    assert v > 0 and np.isfinite(v), f"2**{e} is no positive finite float32"
    return v


def uniform_case(seed: int, n: int, d: int, nq: int, e: int):
    """tests.helpers.make_case(seed, n, d, nq, dup=True) with rows and queries multiplied by float32(2)**e: exact unless a
    product leaves the normal range (then it is rounded to a subnormal, or the assertion fires)."""
    rows, qs = make_case(seed, n, d, nq, dup=True)
    s = pow2(e)
    with np.errstate(over="ignore"):  # (an overflow is caught by the assertion below)
        rows, qs = rows * s, qs * s
    assert rows.dtype == np.float32 and qs.dtype == np.float32
    assert np.isfinite(rows).all() and np.isfinite(qs).all(), f"2**{e}: the scaled inputs are not finite"
    return rows, qs


@functools.lru_cache(maxsize=4)
def uniform_inputs(d: int, e: int):
    """The uniform case of (d, e) as both test files use it: (rows, qs, deleted), 5 % tombstones."""
    rows, qs = uniform_case(UNIFORM_SEED, UNIFORM_N, d, UNIFORM_NQ, e)
    deleted = deleted_mask(UNIFORM_SEED, UNIFORM_N, 0.05)
    for a in (rows, qs, deleted):
        a.setflags(write=False)
    return rows, qs, deleted


def row_mask_for(n: int) -> np.ndarray:
    """The row mask of the masked calls: two rows in three allowed."""
    return (np.arange(n) % 3 != 1).astype(np.uint8)


def range_radius(qs, rows, space, deleted=None) -> float:
    """fp32 of the oracle's mean 10th-nearest fp64 distance over the live rows (as tests/test_gpu_parity.py takes it)."""
    live = rows if deleted is None else rows[~deleted]
    with np.errstate(over="ignore"):
        dm = exact_scan.exact_distances(qs, live, space)
        radius = np.float32(np.sort(dm, axis=1)[:, 9].mean())
    assert np.isfinite(radius), f"the radius {radius!r} is no finite float32"
    return float(radius)


# ---------------------------------------------------------------- ladder: every scale in one corpus
LADDER = (-140, -126, -100, -64, -30, 0, 30, 63, 100, 124)
LADDER_N, LADDER_K, LADDER_PLANTED, LADDER_RUN = 4096, 10, 12, 512
LADDER_DIMS = (64, 100, 256)
LADDER_LAYOUTS = ("interleaved", "blocks")
LADDER_SEED = 11


def planted_rows(j: int) -> np.ndarray:
    """Labels of the twelve rows planted next to ladder query j."""
    return 100 + 31 * (LADDER_PLANTED * j + np.arange(LADDER_PLANTED))


def ladder_case(seed: int, d: int, layout: str):
    """4096 N(0,1) rows scaled by 2**LADDER[.]: "interleaved" -- row i by LADDER[i % 10], so every 16-row panel and every 8-row
    scale group spans the ladder; "blocks" -- runs of 512 rows per exponent (run r by LADDER[r % 10]), homogeneous groups.
    Query j = N(0,1) * 2**LADDER[j]; twelve rows q_j + 2**LADDER[j] * 0.05 (t + 1) N(0,1), t = 0..11, overwrite the rows
    100 + 31 (12 j + t)."""
    assert layout in LADDER_LAYOUTS
    rng = np.random.default_rng(seed)
    n = LADDER_N
    rows = rng.standard_normal((n, d), dtype=np.float32)
    i = np.arange(n)
    rung = i % len(LADDER) if layout == "interleaved" else (i // LADDER_RUN) % len(LADDER)
    scale = np.array([pow2(e) for e in LADDER], dtype=np.float32)
    rows *= scale[rung][:, None]
    qs = rng.standard_normal((len(LADDER), d), dtype=np.float32) * scale[:, None]
    for j in range(len(LADDER)):
        for t, r in enumerate(planted_rows(j)):
            noise = rng.standard_normal(d) * (0.05 * (t + 1))
            rows[r] = (qs[j].astype(np.float64) + float(scale[j]) * noise).astype(np.float32)
    assert np.isfinite(rows).all() and np.isfinite(qs).all(), "ladder: the inputs are not finite"
    return rows, qs


@functools.lru_cache(maxsize=4)
def ladder_inputs(d: int, layout: str):
    rows, qs = ladder_case(LADDER_SEED, d, layout)
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs


# ---------------------------------------------------------------- edge rows: single components at the ends of float32
EDGE_N_PLAIN = 4096
EDGE_DIMS = (64, 256)
EDGE_SEED = 23
EDGE_KINDS = ("+FLT_MAX", "-FLT_MAX", "+3.39e38", "-3.39e38", "+3.40e38", "-3.40e38", "2**-149", "2**-126", "2**124 N(0,1)")
EDGE_VALUES = (F32_MAX, -F32_MAX, np.float32(3.39e38), np.float32(-3.39e38), np.float32(3.40e38), np.float32(-3.40e38),
               pow2(-149), pow2(-126))
EDGE_N = EDGE_N_PLAIN + len(EDGE_KINDS)  # the last 16-row panel holds the nine edge rows and nothing else
EDGE_ORDINARY_QUERIES = 6


def edge_rows_case(seed: int, d: int):
    """4096 N(0,1) rows and nine edge rows: eight N(0,1) rows with one component (a column of its own per kind) set to
    +-FLT_MAX, +-3.39e38 (the largest values bf16 still rounds to a finite number are just above), +-3.40e38 (bf16: inf),
    2**-149, 2**-126, and a row 2**124 N(0,1), doubled until its norm exceeds FLT_MAX (d = 64: 2**126).  Each edge row stands
    three times: in the first panel (rows 1..9), in the last, partial panel (rows 4096..4104: 4096 is a multiple of the
    16-row panel, so the nine are appended behind it) and at the even rows 2000..2016, whose odd neighbours are tombstoned.
    Queries: six ordinary ones, each edge row of the first panel queried back, ordinary ones x 2**-140 and x 2**120.
    Returns (rows, qs, deleted, edge_labels [3, 9])."""
    rng = np.random.default_rng(seed)
    n = EDGE_N
    rows = rng.standard_normal((n, d), dtype=np.float32)
    nk = len(EDGE_KINDS)
    edge = rng.standard_normal((nk, d), dtype=np.float32)
    cols = (5 + 7 * np.arange(nk)) % d
    for kind, v in enumerate(EDGE_VALUES):
        edge[kind, cols[kind]] = v
    e = 124
    big = edge[nk - 1].astype(np.float64)
    while np.sqrt((np.ldexp(big, e) ** 2).sum()) <= float(F32_MAX):
        e += 1
    with np.errstate(over="ignore"):
        edge[nk - 1] = np.ldexp(big, e).astype(np.float32)
    places = np.stack([1 + np.arange(nk), EDGE_N_PLAIN + np.arange(nk), 2000 + 2 * np.arange(nk)])
    for p in places:
        rows[p] = edge
    deleted = deleted_mask(seed, n, 0.02)
    deleted[places.ravel()] = False
    deleted[places[2] + 1] = True
    qs = rng.standard_normal((EDGE_ORDINARY_QUERIES + nk + 2, d), dtype=np.float32)
    qs[EDGE_ORDINARY_QUERIES:EDGE_ORDINARY_QUERIES + nk] = edge
    qs[-2] *= pow2(-140)
    qs[-1] *= pow2(120)
    assert np.isfinite(rows).all() and np.isfinite(qs).all(), "edge rows: the inputs are not finite"
    assert np.sqrt((edge[nk - 1].astype(np.float64) ** 2).sum()) > float(F32_MAX), "edge rows: the big row's norm fits fp32"
    return rows, qs, deleted, places


@functools.lru_cache(maxsize=2)
def edge_inputs(d: int):
    rows, qs, deleted, places = edge_rows_case(EDGE_SEED, d)
    for a in (rows, qs, deleted, places):
        a.setflags(write=False)
    return rows, qs, deleted, places


# ---------------------------------------------------------------- the oracle's own sensitivity
def _column_orders(d: int):
    return (np.arange(d), np.arange(d)[::-1], np.random.default_rng(d).permutation(d))


def oracle_is_stable(qs, rows, k: int, space: str, deleted=None) -> bool:
    """True when the oracle's k + 1 nearest labels do not depend on the order of summation: oracle.exact_scan.knn on the inputs
    as given, with the columns reversed and with the columns under a seeded permutation returns the same labels three times.
    (Exact fp64 ties are fine: they fall to the labels in the oracle and on the device alike.)"""
    qs, rows = np.asarray(qs), np.asarray(rows)
    answers = []
    with np.errstate(over="ignore"):
        for order in _column_orders(rows.shape[1]):
            answers.append(exact_scan.knn(qs[:, order], rows[:, order], k + 1, space, deleted=deleted)[0])
    return all(np.array_equal(answers[0], a) for a in answers[1:])


def oracle_range_is_stable(qs, rows, radius: float, space: str, deleted=None) -> bool:
    """oracle_is_stable for oracle.exact_scan.range_query at ``radius``: the same labels in the same order three times."""
    qs, rows = np.asarray(qs), np.asarray(rows)
    answers = []
    with np.errstate(over="ignore"):
        for order in _column_orders(rows.shape[1]):
            answers.append([w[0] for w in exact_scan.range_query(qs[:, order], rows[:, order], radius, space, deleted=deleted)])
    return all(len(a) == len(answers[0]) and all(np.array_equal(x, y) for x, y in zip(answers[0], a)) for a in answers[1:])


def oracle_knn(qs, rows, k, space, deleted=None):
    with np.errstate(over="ignore"):  # an fp64 distance above FLT_MAX is +-inf as a float32
        return exact_scan.knn(qs, rows, k, space, deleted=deleted)


def oracle_range(qs, rows, radius, space, deleted=None):
    with np.errstate(over="ignore"):
        return exact_scan.range_query(qs, rows, radius, space, deleted=deleted)


# ---------------------------------------------------------------- comparisons
def rel_errors(got, want) -> np.ndarray:
    """|got - want| / max(1, |want|) elementwise; 0 where both are the same infinity, inf where only one is infinite."""
    g64, w64 = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.where(g64 == w64, 0.0, np.abs(g64 - w64)) / np.maximum(1.0, np.abs(w64))
    return np.where(np.isnan(err), np.inf, err)


def assert_knn_matches_rel(got, want, tag: str):
    """tests.helpers.assert_knn_matches with the distance bar of assert_range_matches: labels and counts equal (a mismatch is
    dumped the same way); |got - want| <= SCORE_ATOL * max(1, |want|), equal infinities equal, a finite value against an
    infinite one not.  Only label -1 is padding: a real row whose fp32 distance is +inf keeps its label and is counted."""
    gl, gd, gc = got
    wl, wd, wc = want
    if not (np.array_equal(gl, wl) and np.array_equal(gc, wc)):
        from tests.conftest import dump_mismatch

        dump_mismatch(tag.replace("/", "_"), got_labels=gl, want_labels=wl, got_dist=gd, want_dist=wd, got_counts=gc,
                      want_counts=wc)
        bad = np.nonzero((gl != wl).any(axis=1) | (np.asarray(gc) != np.asarray(wc)))[0]
        b = bad[0]
        raise AssertionError(f"{tag}: ids differ for {bad.size} of {gl.shape[0]} queries, first {bad[:5]}: got {gl[b]} want "
                             f"{wl[b]} (d got {gd[b]} want {wd[b]}, counts got {gc[b]} want {wc[b]})")
    pad = wl < 0
    assert np.all(np.isposinf(gd[pad])), f"{tag}: padding distances are not +inf"
    err = rel_errors(gd[~pad], wd[~pad])
    if err.size and not err.max() <= SCORE_ATOL:
        j = int(np.argmax(err))
        raise AssertionError(f"{tag}: distance of label {wl[~pad][j]} is {gd[~pad][j]!r}, the oracle's {wd[~pad][j]!r}")


def fp64_bar(qs, rows, labels, want64, space: str) -> np.ndarray:
    """The allowed |error| of an fp64 distance, per (query, label): 1e-12 x the size of the summed terms -- cosine 1, l2
    max(1, distance), ip max(1, sum_i |q_i x_i|).  ``labels`` [nq, m] >= 0."""
    if space == "cosine":
        return np.full(want64.shape, FP64_RTOL)
    if space == "l2":
        return FP64_RTOL * np.maximum(1.0, want64)
    q = np.abs(np.asarray(qs, dtype=np.float64))
    out = np.empty(want64.shape)
    for i in range(q.shape[0]):
        out[i] = np.abs(np.asarray(rows[labels[i]], dtype=np.float64)) @ q[i]
    return FP64_RTOL * np.maximum(1.0, out)


def assert_fp64_matches(got64, got32, qs, rows, labels, space: str, tag: str):
    """fp64 distances of the pairs (qs[i], rows[labels[i, j]]) against oracle.exact_scan under fp64_bar; label -1 must give +inf.
    The fp32 face must be float32(fp64 face) to within 1 ulp, or the same infinity."""
    labels = np.asarray(labels)
    real = labels >= 0
    safe = np.where(real, labels, 0)
    with np.errstate(over="ignore"):
        full = exact_scan.exact_distances(qs, rows, space)
    want = np.take_along_axis(full, safe, axis=1)
    assert np.all(np.isposinf(got64[~real])), f"{tag}: label -1 does not give +inf"
    assert np.isfinite(got64[real]).all(), f"{tag}: an fp64 distance of finite inputs is not finite"
    err = np.abs(got64 - want)
    bar = fp64_bar(qs, rows, safe, want, space)
    bad = real & ~(err <= bar)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError(f"{tag}: query {i}, label {labels[i, j]}: fp64 distance {got64[i, j]!r}, the oracle's {want[i, j]!r} "
                             f"(|error| {err[i, j]:.3e}, allowed {bar[i, j]:.3e}; {int(bad.sum())} pairs over the bar)")
    if got32 is not None:
        assert_fp32_face(got64, got32, tag)


def assert_fp32_face(got64, got32, tag: str):
    """The fp32 face of a distance is float32(its fp64 face) to within 1 ulp between finite values; an infinity (a rounding
    beyond FLT_MAX, padding) only equals itself -- FLT_MAX against +inf is a finite value against an infinite one."""
    with np.errstate(over="ignore"):
        r32 = np.asarray(got64, dtype=np.float64).astype(np.float32)
    g32 = np.asarray(got32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        near = (g32 == np.nextafter(r32, np.float32(np.inf))) | (g32 == np.nextafter(r32, np.float32(-np.inf)))
        ok = (g32 == r32) | (near & np.isfinite(g32) & np.isfinite(r32))
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError(f"{tag}: at {at}: fp32 distance {g32[at]!r} is not float32 of the fp64 distance {np.asarray(got64)[at]!r}")


# ---------------------------------------------------------------- the engine under test and the route it took
def open_engine(rows, space, strategy, deleted=None):
    from mlvectordb_amd.engine import HipScanEngine

    eng = HipScanEngine(rows.shape[1], space, device=0, strategy=strategy)
    try:
        for part in np.array_split(rows, [rows.shape[0] * 5 // 8 + 3]):  # two pieces, the first ends inside a panel
            eng.append(part)
        if deleted is not None and deleted.any():
            assert eng.tombstone(np.nonzero(deleted)[0]) == int(deleted.sum())
        eng.last_stats()
    except Exception:
        eng.close()
        raise
    return eng


def record(eng, tag: str, rows, strategy: str, qs=None) -> dict:
    """The route of the call just made, kept in the route log.  A forced-filter call on an index inside the filter path's
    magnitude window (magnitude_helpers.inside_filter_window) must report the filter route: the code before the magnitude
    fixes reported it for every such call of this file, and nothing about those indexes calls for the exact scan.  (The
    window is the fix's own: the issue asked for the assertion wherever the filter route was reported before, and three
    families that were answered correctly on it -- uniform l2 at 2**-100, ip at 2**100 and 2**124 where right, cosine at 2**124
    with d = 64 and 100 -- lie outside the window, run the exact scan now and carry no route assertion.)  Outside the window the
    route is free.  Inside it the exact fallback is held too (``qs``: the call's queries): none for a batch of queries the
    filter serves, at least the queries magnitude_helpers.queries_leaving_window names otherwise -- so the filter route
    cannot quietly become the exact scan."""
    st = eng.last_stats()
    path = os.environ.get("MLVDB_ROUTE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"tag": tag, "strategy_used": st["strategy_used"], "bound_dtype": st["bound_dtype"],
                                "fallback_queries": st["fallback_queries"]}) + "\n")
    if strategy == "filter" and inside_filter_window(rows, eng.space):
        assert st["strategy_used"] == 2, f"{tag}: the forced filter strategy was served by route {st['strategy_used']}"
        if qs is not None:
            leaving = int(queries_leaving_window(qs, rows, eng.space).sum())
            if leaving == 0:
                assert st["fallback_queries"] == 0, f"{tag}: {st['fallback_queries']} queries fell back to the exact scan"
            else:  # (a range call may run twice: the statistics accumulate)
                assert st["fallback_queries"] >= leaving, f"{tag}: {st['fallback_queries']} fallbacks, {leaving} queries leave the window"
    if strategy == "exact":
        assert st["strategy_used"] == 1, f"{tag}: the forced exact strategy was served by route {st['strategy_used']}"
    return st


# ---------------------------------------------------------------- the search families built on the primitives
# The matrix of tests/test_magnitudes_families_host.py and tests/test_gpu_magnitudes_families.py: every family x corpus x
# space (x strategy on the device).  The corpora are the seeded ones above; the attribute columns are pure functions of the
# label, so every scale of the ladder and every edge row lands in groups it shares with ordinary rows.
FAMILY_STRATEGIES = ("exact", "filter")
FAMILY_EXPONENTS = (-140, -64, 40, 124)
FAMILY_CORPORA = tuple((f"U{e}", d) for e in FAMILY_EXPONENTS for d in (64, 100)) + (
    ("ladder", 64), ("ladder", 100), ("edge", 64), ("mixed", 64), ("mixed", 256))
FAMILIES = ("each", "range_each", "distinct", "grouped", "mmr", "like", "maxsim", "hybrid")
FAMILY_NQ = 12                 # the first 12 queries of a uniform corpus
GROUP, BUCKET, SPARSE = 0, 1, 2  # the attribute columns of every family engine
GROUP_MOD, GROUP_ABSENT_MOD, BUCKET_MOD = 37, 11, 4  # 37 is coprime with the ladder's period of 10
FILTER_SCHEMA = {"group": "int", "bucket": "int"}  # (declaration order: attribute i is column i)
FILTERS = ({"bucket": 0}, {"bucket": {"$in": [1, 2]}}, {"group": {"$lt": 3}})
PROGRAM_CYCLE = (0, 2, 1, -1)  # query i runs under FILTERS[PROGRAM_CYCLE[i % 4]]: the odd queries of ``mixed`` (1, 4, 9) fall
                               # under "group < 3" (the gathered route) and "bucket == 0" (the scan route)
GATHERED_PROGRAM = 2
WHERE_GATHER_DEFAULT = 150     # csrc/internal.h; include/mlvdb_where_each.h states the rule route_plan restates
EACH_K, DISTINCT_K, GROUPED_K, GROUPED_SIZE, MAXSIM_K, HYBRID_K, HYBRID_FETCH, LIKE_K = 10, 10, 5, 3, 5, 10, 32, 10
MMR_K, MMR_FETCH, MMR_BIG_FETCH, MMR_LAMBDAS = 10, 100, 1024, (0.5, 0.0)
DISTINCT_LIST = 64             # L = max(64, DISTINCT_OVERSAMPLE x k) at k = 10 and the default oversampling of 4
LIKE_WEIGHTS = ((0.5, 0.5), (1.0, -0.5))
LIKE_WEIGHTS_EDGE = ((0.25, 0.25),)
MAXSIM_LENGTHS = (4, 1, 8)
SPARSE_VOCAB, SPARSE_MAX_NNZ, SPARSE_SEED = 64, 16, 53
EDGE_EXCLUDED_CAP = 3          # on ``edge`` at most one query in three may be left out of the id comparison
DEVICE_KS = (10, 64, 100, 1024)


def range_each_has_radius(corpus: str, space: str) -> bool:
    """Does a float32 radius exist for ``range_each`` on this corpus?  Cosine: always; l2 / ip: the uniform corpora at the
    exponents of RANGE_EXPONENTS, and ``mixed`` (its ordinary queries give the radius).  On ``ladder`` and ``edge`` the mean
    10th-nearest l2 / ip distance is beyond FLT_MAX."""
    if space == "cosine" or corpus == "mixed":
        return True
    return corpus.startswith("U") and int(corpus[1:]) in RANGE_EXPONENTS[space]


def family_cells():
    """(family, corpus, d, space) of every cell both files run."""
    return [(f, c, d, s) for f in FAMILIES for c, d in FAMILY_CORPORA for s in SPACES
            if f != "range_each" or range_each_has_radius(c, s)]


def family_columns(n: int):
    """(group, bucket) int64 columns of rows 0..n-1."""
    label = np.arange(n, dtype=np.int64)
    group = np.where(label % GROUP_ABSENT_MOD == 5, W.INT64_ABSENT, label % GROUP_MOD)
    return group, label % BUCKET_MOD


def sparse_rows(n: int):
    """Row i's sparse vector: ``None`` for about one row in ten, else up to 16 of 64 terms with N(0,1) float32 weights."""
    rng = np.random.default_rng(SPARSE_SEED)
    out = []
    for _ in range(n):
        if rng.random() < 0.1:
            out.append(None)
            continue
        terms = rng.choice(SPARSE_VOCAB, size=int(rng.integers(0, SPARSE_MAX_NNZ + 1)), replace=False)
        out.append({int(t): float(np.float32(rng.standard_normal()) or np.float32(1)) for t in terms.tolist()})
    return out


def sparse_queries(nq: int):
    rng = np.random.default_rng(SPARSE_SEED + 1)
    return [{int(t): float(np.float32(rng.standard_normal()) or np.float32(1))
             for t in rng.choice(SPARSE_VOCAB, size=int(rng.integers(3, 9)), replace=False).tolist()} for _ in range(nq)]


# ladder_case's seed per d.  d = 64: LADDER_SEED, the corpus of the kNN tests.  d = 100: under LADDER_SEED the 100 nearest rows of the
# 2**100 rung's query (MMR's candidates at fetch_k = 100; the kNN tests stop at k = 10) hold two rows of the 2**63 rung whose l2
# distances differ by 3e-12 of themselves, and their order follows the order of summation: another seed, held to every
# precondition by tests/test_magnitudes_families_host.py
FAMILY_LADDER_SEED = {64: LADDER_SEED, 100: LADDER_SEED + 1}


@functools.lru_cache(maxsize=None)
def family_ladder_inputs(d: int):
    rows, qs = ladder_case(FAMILY_LADDER_SEED[d], d, "interleaved")
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs


@functools.lru_cache(maxsize=None)
def family_case(corpus: str, d: int):
    """Everything a family call on ``corpus`` needs, read-only: rows, qs, deleted, the columns, the compiled programs and
    ``program_of_query``, the sparse column and queries (as ``where.SparseColumn``), the like examples (two stored live
    labels per query; on ``edge`` the first nine queries take an edge row of the first panel as their first example) and the
    token rows of the three late-interaction queries."""
    from tests.sparse_helpers import sparse_csr

    if corpus.startswith("U"):
        rows, qs, deleted = uniform_inputs(d, int(corpus[1:]))
        qs = qs[:FAMILY_NQ]
    elif corpus == "ladder":
        rows, qs = family_ladder_inputs(d)
        deleted = np.zeros(rows.shape[0], dtype=bool)
    elif corpus == "edge":
        rows, qs, deleted, places = edge_inputs(d)
    else:
        assert corpus == "mixed"
        rows, qs, deleted = mixed_inputs(d)
    n, nq = rows.shape[0], qs.shape[0]
    c = types.SimpleNamespace(corpus=corpus, d=d, rows=rows, qs=qs, deleted=deleted, n=n, nq=nq)
    c.group, c.bucket = family_columns(n)
    c.programs = [W.compile_where(f, FILTER_SCHEMA) for f in FILTERS]
    c.program_of_query = np.array([PROGRAM_CYCLE[i % len(PROGRAM_CYCLE)] for i in range(nq)], dtype=np.int32)
    c.sparse_list = sparse_rows(n)
    c.sparse = sparse_csr(c.sparse_list)
    c.sparse_queries = sparse_csr(sparse_queries(nq))
    rng = np.random.default_rng(1000 + d)
    live = np.flatnonzero(~deleted)
    ex = np.stack([rng.choice(live, size=2, replace=False) for _ in range(nq)]).astype(np.int64)
    if corpus == "edge":
        ex[:len(EDGE_KINDS), 0] = places[0]
        assert (ex[:, 0] != ex[:, 1]).all()
    c.like_labels = ex.ravel()
    c.like_offsets = 2 * np.arange(nq + 1, dtype=np.int64)
    c.like_weights = LIKE_WEIGHTS_EDGE if corpus == "edge" else LIKE_WEIGHTS
    c.token_of = np.arange(sum(MAXSIM_LENGTHS)) % nq  # token t of the late-interaction call is query token_of[t]
    c.token_offsets = np.concatenate([[0], np.cumsum(MAXSIM_LENGTHS)]).astype(np.int64)
    c.odd = np.array(MIXED_ODD_AT if corpus == "mixed" else (), dtype=np.int64)
    return c


def family_radius(c, space: str) -> float:
    """The radius of the case's ``range_each`` call: range_radius over its queries (``mixed``: over the ordinary ones)."""
    if c.corpus == "mixed":
        return mixed_radius(c.d, space)
    return range_radius(c.qs, c.rows, space, c.deleted)


def route_plan(matches: int, queries: int, live: int, gather: int = WHERE_GATHER_DEFAULT) -> str:
    """include/mlvdb_where_each.h: GATHER when matches x ceil(queries / 4) x 1000 <= live rows x WHERE_GATHER (k <= 64)."""
    if matches == 0:
        return "none"
    return "gather" if matches * -(-queries // 4) * 1000 <= live * gather else "scan"


def distinct_list_short(c, space: str):
    """The queries distinct's list pass cannot finish: their DISTINCT_LIST nearest live rows hold fewer than
    DISTINCT_K present groups, so the grouped scan serves them and they count as ``fallback_queries``."""
    lab = oracle_knn(c.qs, c.rows, DISTINCT_LIST, space, c.deleted)[0]
    out = []
    for i in range(c.nq):
        g = c.group[lab[i][lab[i] >= 0]]
        if np.unique(g[g != W.INT64_ABSENT]).size < DISTINCT_K:
            out.append(i)
    return out


def mmr_distances(v, rows, space: str) -> np.ndarray:
    """fp64 distances of one float32 vector to ``rows``: oracle.exact_scan.exact_distances on a [1, d] query -- a function
    of the bits of ``v`` and ``rows`` alone, whatever role ``v`` plays."""
    return exact_scan.exact_distances(np.asarray(v, dtype=np.float32)[None], rows, space)[0]


def family_model_class():
    """The model engine with every family's entry (tests/*_helpers.py), in NumPy fp64."""
    from tests.grouped_helpers import GroupedOracleEngine
    from tests.hybrid_helpers import HybridOracleEngine
    from tests.like_helpers import LikeOracleEngine
    from tests.maxsim_helpers import MaxSimOracleEngine
    from tests.mmr_helpers import MmrOracleEngine
    from tests.where_helpers import EachOracleEngine, EachRangeOracleEngine

    class FamilyModel(HybridOracleEngine, GroupedOracleEngine, MmrOracleEngine, LikeOracleEngine, MaxSimOracleEngine,
                      EachOracleEngine, EachRangeOracleEngine):
        def search_mmr(self, queries, k, fetch_k, lam, where=None, want64=False):
            """MmrOracleEngine.search_mmr with both distances of the objective from one routine on one shape: d(q, i) and
            D(s, i) are ``mmr_distances`` of one vector against the candidates' rows.  A query that is a stored row (every
            corpus here queries rows back) then has d(q, i) = D(c_0, i) bit for bit, as on the device and in exact
            arithmetic, and at lambda = 0.5 every objective ties at exactly 0 and falls to the position; taken from matrix
            products of different shapes the two differ in the last bit and rounding alone picks.  Only the picked rows'
            D(s, .) are computed (mmr_select asks for no other): at fetch_k = 1024 the whole matrix is a hundred times the
            work."""
            from tests.mmr_helpers import mmr_from_candidates

            queries = np.asarray(queries, dtype=np.float32)
            cl, cd32, cc, cd64 = self.search64(queries, fetch_k, where=where)
            cd64 = cd64.copy()
            for i in range(cl.shape[0]):
                cd64[i, :cc[i]] = mmr_distances(queries[i], self._rows[cl[i, :cc[i]]], self.space)

            def pair_rows(_, cands):
                return lambda s: mmr_distances(self._rows[cands[s]], self._rows[cands], self.space)

            out, _ = mmr_from_candidates(cl, cd32, cc, cd64, pair_rows, k, lam)
            return out if want64 else out[:3] + (None,) + out[4:]

    return FamilyModel


def fill_engine(eng, c, order=None, sparse=True):
    """Rows (two appends, as open_engine splits them; columns permuted by ``order``), the tombstones and the attribute
    columns of ``c`` into a model engine -- or the columns alone into a device engine open_engine has filled."""
    if eng.counts()[0] == 0:
        rows = c.rows if order is None else np.ascontiguousarray(c.rows[:, order])
        for part in np.array_split(rows, [c.n * 5 // 8 + 3]):
            eng.append(part)
        if c.deleted.any():
            assert eng.tombstone(np.flatnonzero(c.deleted)) == int(c.deleted.sum())
    eng.define_attr(GROUP, "int64")
    eng.define_attr(BUCKET, "int64")
    eng.set_attr(GROUP, 0, c.group)
    eng.set_attr(BUCKET, 0, c.bucket)
    if sparse:
        eng.define_attr(SPARSE, "sparse")
        eng.set_attr_sparse(SPARSE, 0, c.sparse)
    return eng


def family_model(c, space: str, order=None):
    return fill_engine(family_model_class()(c.d, space), c, order)


def family_variants(family: str, c, space: str, order=None):
    """The calls of one cell: [(name, tuning, call)], ``call(engine)`` the same for the model and the device engine (their
    entries share a signature); ``tuning``: what ``set_tuning`` takes on the device for this variant (the model has no
    routes).  ``order`` permutes the columns of everything that holds vector components."""
    from tests.hybrid_helpers import METHODS

    q = c.qs if order is None else np.ascontiguousarray(c.qs[:, order])
    if family == "each":
        return [("k10", {}, lambda e: e.search_each(q, EACH_K, c.programs, c.program_of_query, want64=True, return_routes=True))]
    if family == "range_each":
        r = family_radius(c, space)
        return [(f"r{r!r}", {}, lambda e: e.range_each(q, r, 64, c.programs, c.program_of_query, return_routes=True))]
    if family == "distinct":
        call = lambda e: e.search_distinct(q, DISTINCT_K, GROUP, want64=True)  # noqa: E731
        return [("list", {}, call), ("scan", {"DISTINCT_OVERSAMPLE": 0}, call)]
    if family == "grouped":
        return [("k5g3", {}, lambda e: e.search_grouped(q, GROUPED_K, GROUPED_SIZE, GROUP, want64=True))]
    if family == "mmr":
        out = [(f"f{MMR_FETCH}/lam{lam}", {}, lambda e, lam=lam: e.search_mmr(q, MMR_K, MMR_FETCH, lam, want64=True))
               for lam in MMR_LAMBDAS]
        if (c.corpus, c.d) == ("mixed", 256):  # the big-k passes, with the odd queries, on the device route
            out.append((f"f{MMR_BIG_FETCH}/lam0.5", {}, lambda e: e.search_mmr(q, MMR_K, MMR_BIG_FETCH, 0.5, want64=True)))
        return out
    if family == "like":
        out = []
        for w in c.like_weights:
            weights = np.tile(np.array(w, dtype=np.float64), c.nq)
            for base in (None, q) if space == "cosine" else (None,):
                out.append((f"w{w[0]},{w[1]}" + ("/base" if base is not None else ""), {},
                            lambda e, weights=weights, base=base: e.search_like(
                                c.like_labels, weights, c.like_offsets, LIKE_K, base=base, exclude=True, want64=True,
                                want_queries=True)))
        return out
    if family == "maxsim":
        toks = np.ascontiguousarray(q[c.token_of])
        return [("k5", {}, lambda e: e.search_maxsim(toks, c.token_offsets, MAXSIM_K, GROUP, want_matches=True))]
    assert family == "hybrid"
    return [(m, {}, lambda e, m=m: e.search_hybrid(q, SPARSE, c.sparse_queries, HYBRID_K, HYBRID_FETCH, HYBRID_FETCH, method=m,
                                                   components=True)) for m in METHODS]


def family_ids(family: str, c, out):
    """Per query, the part of a family's answer that is ids: labels, counts, groups, group counts, pick ranks, match labels,
    list ranks.  A list of tuples of arrays, one per query."""
    if family == "each":
        return [(out[0][i], out[2][i]) for i in range(c.nq)]
    if family == "range_each":
        return [(np.asarray(out[0][i][0]),) for i in range(c.nq)]
    if family == "distinct":  # (labels, d32, counts, d64, groups)
        return [(out[0][i], out[2][i], out[4][i]) for i in range(c.nq)]
    if family == "grouped":   # (labels, d32, counts, group counts, d64, groups)
        return [(out[0][i], out[2][i], out[3][i], out[5][i]) for i in range(c.nq)]
    if family == "mmr":       # (labels, d32, counts, d64, rank, objective)
        return [(out[0][i], out[2][i], out[4][i]) for i in range(c.nq)]
    if family == "like":
        return [(out[0][i], out[2][i]) for i in range(c.nq)]
    if family == "maxsim":    # (groups, s32, counts, s64, match labels, match d64): a query owns its tokens' match rows
        off = c.token_offsets
        return [(out[0][i], out[2][i], out[4][off[i]:off[i + 1]]) for i in range(len(MAXSIM_LENGTHS))]
    assert family == "hybrid"  # (labels, fused, counts, d64, s64, rank dense, rank sparse)
    return [(out[0][i], out[2][i], out[5][i], out[6][i]) for i in range(c.nq)]


def ids_differ(a, b):
    """The queries at which two ``family_ids`` lists differ."""
    assert len(a) == len(b)
    return [i for i, (x, y) in enumerate(zip(a, b))
            if not all(np.shape(u) == np.shape(v) and np.array_equal(u, v) for u, v in zip(x, y))]


@functools.lru_cache(maxsize=None)
def family_expected(family: str, corpus: str, d: int, space: str):
    """{variant: the model's answer} of one cell (columns in their own order)."""
    c = family_case(corpus, d)
    with np.errstate(over="ignore"):
        model = family_model(c, space)
        return {name: call(model) for name, _, call in family_variants(family, c, space)}


@functools.lru_cache(maxsize=None)
def family_unstable(family: str, corpus: str, d: int, space: str):
    """{variant: the queries whose ids in the model's answer depend on the order of summation}: the model run on the inputs
    as given, with the columns reversed and under a seeded permutation (oracle_is_stable's three orders), per family."""
    c = family_case(corpus, d)
    want = family_expected(family, corpus, d, space)
    out = {name: set() for name in want}
    with np.errstate(over="ignore"):
        for order in _column_orders(d)[1:]:
            model = family_model(c, space, order)
            for name, _, call in family_variants(family, c, space, order):
                out[name] |= set(ids_differ(family_ids(family, c, want[name]), family_ids(family, c, call(model))))
    return {name: sorted(v) for name, v in out.items()}


def family_excluded(family: str, corpus: str, d: int, space: str):
    """{variant: queries left out of the id comparison on the device}.  Only ``edge`` may have any (queried-back FLT_MAX
    rows, where terms cancel); tests/test_magnitudes_families_host.py holds every other corpus to none, and ``edge`` to at
    most one query in three."""
    if corpus != "edge":
        return {name: [] for name in family_expected(family, corpus, d, space)}
    return family_unstable(family, corpus, d, space)


def family_fp64_bar(qs, rows, labels, want64, space: str) -> np.ndarray:
    """fp64_bar with l2 in units of its own terms: FP64_RTOL x (|q| + |x|)**2, norms in fp64 (every term of the sum is below
    it; fp64_bar's floor of 1 is no term, and would make the bar vacuous at 2**-280).  FP64_RTOL = 1e-12 is over 35 x the
    worst-case rounding of a 256-term fp64 sum, 256 x 2**-53 = 2.8e-14.  Cosine and ip keep their bars: the 1 of ``1 - s``
    is a term."""
    if space != "l2":
        return fp64_bar(qs, rows, labels, want64, space)
    q = np.asarray(qs, dtype=np.float64)
    qn = np.sqrt(np.einsum("ij,ij->i", q, q))
    x = np.asarray(rows, dtype=np.float64)
    xn = np.sqrt(np.einsum("ij,ij->i", x, x))
    return FP64_RTOL * (qn[:, None] + xn[labels]) ** 2


def assert_family_fp64(got64, got32, qs, rows, labels, space: str, tag: str):
    """assert_fp64_matches under family_fp64_bar, for ``labels`` [nq, ...] of any trailing shape: an fp64 distance of a real
    pair is finite and within the bar of the oracle's, label -1 gives +inf (padding is the label's business alone), and the
    fp32 face (when given) is the rounded fp64 one."""
    nq = np.shape(qs)[0]
    labels = np.asarray(labels).reshape(nq, -1)
    got64 = np.asarray(got64).reshape(nq, -1)
    real = labels >= 0
    safe = np.where(real, labels, 0)
    with np.errstate(over="ignore"):
        full = exact_scan.exact_distances(qs, rows, space)
    want = np.take_along_axis(full, safe, axis=1)
    assert np.all(np.isposinf(got64[~real])), f"{tag}: label -1 does not give +inf"
    assert np.isfinite(got64[real]).all(), f"{tag}: an fp64 distance of finite inputs is not finite"
    err = np.abs(got64 - want)
    bar = family_fp64_bar(qs, rows, safe, want, space)
    bad = real & ~(err <= bar)
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError(f"{tag}: query {i}, label {labels[i, j]}: fp64 distance {got64[i, j]!r}, the oracle's {want[i, j]!r} "
                             f"(|error| {err[i, j]:.3e}, allowed {bar[i, j]:.3e}; {int(bad.sum())} pairs over the bar)")
    if got32 is not None:
        assert_fp32_face(got64, np.asarray(got32).reshape(nq, -1), tag)


def assert_family_ids(family: str, c, got, want, excluded, tag: str):
    """The ids of ``got`` equal the model's for every query not in ``excluded``."""
    bad = [i for i in ids_differ(family_ids(family, c, got), family_ids(family, c, want)) if i not in set(excluded)]
    if bad:
        from tests.conftest import dump_mismatch

        i = bad[0]
        g, w = family_ids(family, c, got)[i], family_ids(family, c, want)[i]
        dump_mismatch(tag.replace("/", "_"), query=np.int64(i), **{f"got{j}": np.asarray(a) for j, a in enumerate(g)},
                      **{f"want{j}": np.asarray(a) for j, a in enumerate(w)})
        raise AssertionError(f"{tag}: ids differ from the model's for queries {bad} (left out: {list(excluded)}); query {i}: "
                             f"got {[np.asarray(a).tolist() for a in g]} want {[np.asarray(a).tolist() for a in w]}")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------- sparse weights at the ends of float32
SPARSE_EDGE_N, SPARSE_EDGE_NQ, SPARSE_EDGE_K, SPARSE_EDGE_SEED = 600, 14, 10, 71
SPARSE_EPS = 2 * 255 * 2.0 ** -53  # tests/test_gpu_sparse.py: reordering the fp64 additions, in units of sum |wq wr|


SPARSE_EDGE_PLAIN_TERMS = 48  # terms from here on never take one of the fixed values: scores over them do not tie


def _edge_weight(rng, term: int) -> float:
    kind = int(rng.integers(0, 8)) if term < SPARSE_EDGE_PLAIN_TERMS else int(rng.integers(5, 7))
    n01 = np.float32(rng.standard_normal()) or np.float32(1)
    with np.errstate(under="ignore"):
        w = np.float32((F32_MAX, -F32_MAX, pow2(-149), pow2(-126), n01 * pow2(-140), n01 * pow2(120), n01, -pow2(-149))[kind])
    return float(w) if w != 0 and np.isfinite(w) else float(pow2(-149))


def sparse_ranks_apart(scores, mass, lab, cand) -> np.ndarray:
    """bool [nq]: is the model's ranking of a query's first ``lab.shape[1] - 1`` rows beyond what reordering the additions can
    change?  ``scores`` / ``mass`` [nq, n] from sparse_helpers.dense_scores, ``lab`` [nq, k + 1] the model's ranked labels
    (every slot filled), ``cand`` bool [n] the rows with a vector.  True when every listed score is above the next one by
    more than the two rows' bounds (SPARSE_EPS x mass), and the k-th is above every unlisted row's score plus its bound."""
    out = np.zeros(scores.shape[0], dtype=bool)
    for q in range(scores.shape[0]):
        top = lab[q, :-1]
        s, b = scores[q], SPARSE_EPS * mass[q]
        rest = np.setdiff1d(np.flatnonzero(cand), top)
        apart = (s[top][:-1] - s[top][1:] > b[top][:-1] + b[top][1:]).all()
        out[q] = apart and s[top[-1]] - b[top[-1]] > (s[rest] + b[rest]).max()
    return out


def sparse_edge_case():
    """(rows, queries) as lists of ``None`` / dicts term -> weight over 64 terms, <= 16 nonzeros each: weights +-FLT_MAX,
    +-2**-149, 2**-126, N(0,1) x 2**-140 (subnormal), N(0,1) x 2**120 and plain N(0,1), mixed within one vector.  The fixed
    values tie whole runs of rows exactly (FLT_MAX x FLT_MAX beside terms below its last bit), so the terms from
    SPARSE_EDGE_PLAIN_TERMS on hold N(0,1) and N(0,1) x 2**120 alone and the last six queries use only those: their rankings
    are beyond the reordering bound (sparse_ranks_apart) and are compared id for id."""
    rng = np.random.default_rng(SPARSE_EDGE_SEED)

    def vector(lo, first_term=0):
        terms = first_term + rng.choice(SPARSE_VOCAB - first_term, size=int(rng.integers(lo, SPARSE_MAX_NNZ + 1)), replace=False)
        return {int(t): _edge_weight(rng, int(t)) for t in terms.tolist()}

    rows = [None if rng.random() < 0.1 else vector(0) for _ in range(SPARSE_EDGE_N)]
    queries = [vector(2) for _ in range(SPARSE_EDGE_NQ - 6)] + [vector(3, SPARSE_EDGE_PLAIN_TERMS) for _ in range(6)]
    return rows, queries
