"""Inputs and comparisons for the magnitude tests (tests/test_magnitudes_host.py, tests/test_gpu_magnitudes.py): corpora
whose components span the whole finite float32 range, every one built from a seed, and the bars an answer is held to.

The reference of every comparison is oracle.exact_scan (fp64 from the fp32 inputs: no finite float32 input overflows it).
Nothing here needs a GPU.
"""
from __future__ import annotations

import functools

import numpy as np

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
