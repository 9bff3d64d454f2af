"""Plain range search (mlvdb_range_batch_packed, HipScanEngine.range) against the NumPy oracle at the limits of its kernels.

The reference is always oracle.exact_scan.range_query / exact_distances (fp64), never the engine's other strategy; every case
builds its inputs from a seed and asserts its preconditions on the oracle alone before the first GPU call.  Sizes are the
smallest at which the named edge exists (DESIGN section 5.6 lists the limits pinned here):

* exact_range_kernel: query tiles of 4 / 2 / 1 (by row width), the qsel indirection of flagged queries;
* range_rank_kernel: work items of 32 hits, lists padded to multiples of 64, more than kCandCap = 8192 hits -> paged exact kNN;
* more than kRangeCandCap = 65536 candidates -> exact range scan, then paging; MLVDB_MAX_TOPK_PAGED = 16384 hits returned,
  MLVDB_ERR_OVERFLOW / MLVDB_ERR_UNSUPPORTED;
* `dist <= radius` on the fp64 distance against double(float radius), rows exactly on the radius;
* the fp16 mid shadow (attach_mid) through appends, tombstones, compact and reset.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.helpers import assert_range_matches, deleted_mask

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = 6  # include/mlvdb_hip.h: MLVDB_ERR_UNSUPPORTED
CAND_CAP = 8192          # internal.h: kCandCap
RANGE_CAND_CAP = 65536   # internal.h: kRangeCandCap
PAGED = _native.MAX_TOPK_PAGED
F32_MAX = float(np.finfo(np.float32).max)
STRATEGY_CODE = {"exact": 1, "filter": 2}


def open_engine(rows, space, strategy, deleted=None, pieces=1):
    eng = HipScanEngine(rows.shape[1], space, device=0, strategy=strategy)
    try:
        for part in np.array_split(rows, pieces):
            eng.append(part)
        if deleted is not None and deleted.any():
            assert eng.tombstone(np.nonzero(deleted)[0]) == int(deleted.sum())
    except Exception:
        eng.close()
        raise
    return eng


def sizes_of(want) -> np.ndarray:
    return np.array([len(w[0]) for w in want], dtype=np.int64)


def cut(want, cap: int):
    return [(wl[:cap], wd[:cap]) for wl, wd in want]


def packed_call(eng, qs, radius, capacity, total):
    """One mlvdb_range_batch_packed call -> (status, hits per query, counts, offsets); total = 0: a counting call (NULL outputs)."""
    nq = qs.shape[0]
    qs = np.ascontiguousarray(qs, dtype=np.float32)
    lab = np.full(max(total, 1), -9, dtype=np.int64)
    dist = np.zeros(max(total, 1), dtype=np.float32)
    off = np.full(nq + 1, -1, dtype=np.int64)
    cnt = np.full(nq, -1, dtype=np.int64)
    rc = eng._lib.mlvdb_range_batch_packed(eng.handle, qs.ctypes.data, nq, C.c_float(radius), capacity, total,
                                           lab.ctypes.data if total else None, dist.ctypes.data if total else None,
                                           off.ctypes.data, cnt.ctypes.data)
    hits = [(lab[off[i]:off[i + 1]], dist[off[i]:off[i + 1]]) for i in range(nq)] if total else None
    return rc, hits, cnt, off


# ---------------------------------------------------------------- 1. hit counts at the edges of ranking and paging
EDGE_COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193]


@pytest.mark.parametrize("strategy", ["exact", "filter"])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
@pytest.mark.parametrize("d", [64, 100])
def test_hit_counts_at_the_edges_of_ranking_and_paging(d, space, strategy):
    """Query 0 gets exactly m hits for every m around a 32-hit work item, a 64-entry padding step, the 256 hits of eight
    items and kCandCap = 8192 (8193: flagged by range_rank_kernel, served by the paged exact kNN); the radius lies halfway
    between its m-th and (m + 1)-th distance.  Every hit through the resizing wrapper, the first 32 truncated, and the counts
    and layout of a counting call."""
    rng = np.random.default_rng(1234 + d)
    rows = rng.standard_normal((12000, d), dtype=np.float32)
    qs = rng.standard_normal((3, d), dtype=np.float32)
    s = np.sort(exact_scan.exact_distances(qs[:1], rows, space)[0])
    cases = []
    for m in EDGE_COUNTS:
        radius = np.float32((s[m - 1] + s[m]) / 2) if m else np.nextafter(np.float32(s[0]), np.float32(-np.inf))
        want = exact_scan.range_query(qs, rows, float(radius), space)
        assert len(want[0][0]) == m, f"precondition: the oracle has {len(want[0][0])} hits for query 0, not {m}"
        cases.append((m, float(radius), want))
    eng = open_engine(rows, space, strategy)
    try:
        for m, radius, want in cases:
            tag = f"edges/{space}/{strategy}/d{d}/m{m}"
            sizes = sizes_of(want)
            eng.last_stats()  # (the statistics accumulate between reads)
            assert_range_matches(eng.range(qs, radius, 64), want, tag)
            # 8192 hits are still ranked by range_rank_kernel; only a longer list sends its query to the paged exact kNN
            paged = eng.last_stats()["fallback_queries"]
            assert (paged > 0) == (sizes.max() > CAND_CAP), f"{tag}: {paged} queries fell back, hit counts {sizes}"
            assert_range_matches(eng.range(qs, radius, 32, truncate=True), cut(want, 32), tag + "/truncated")
            rc, _, cnt, off = packed_call(eng, qs, radius, 32, 0)
            assert np.array_equal(cnt, sizes), f"{tag}: counting call: {cnt} vs {sizes}"
            assert off[3] == np.minimum(sizes, 32).sum(), f"{tag}: counting call: offsets {off}"
            assert rc == (_native.ERR_OVERFLOW if sizes.max() > 0 else _native.OK), (tag, rc)
        assert eng.last_stats()["strategy_used"] == STRATEGY_CODE[strategy]
    finally:
        eng.close()


# ---------------------------------------------------------------- 2. lists that overflow, and the two error statuses
@functools.lru_cache(maxsize=None)
def overflow_inputs():
    """80,001 rows x 64, 10 % tombstoned.  (a) runs on all of them: a query with more than kRangeCandCap = 65,536 hits needs that
    many LIVE rows, which 70,001 rows less 10 % (63,000) cannot give; (b) runs on the first 70,001, where every list fits its
    65,536 slots but not the 8,192 one block ranks."""
    n, d = 80_001, 64
    rng = np.random.default_rng(2024)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    deleted = deleted_mask(2024, n, 0.1)
    stored = int(np.nonzero(~deleted)[0][17])
    qs = np.zeros((4, d), dtype=np.float32)
    qs[1] = rows[stored]
    qs[2:] = 3.0 * rng.standard_normal((2, d), dtype=np.float32)
    dm = exact_scan.exact_distances(qs, rows[~deleted], "l2")
    # (a): the zero query takes all but its 200 farthest live rows
    radius_a = float(np.float32(np.sort(dm[0])[-200]))
    want_a = exact_scan.range_query(qs, rows, radius_a, "l2", deleted=deleted)
    nb = 70_001
    want_b = exact_scan.range_query(qs, rows[:nb], F32_MAX, "l2", deleted=deleted[:nb])
    return rows, deleted, qs, radius_a, want_a, nb, want_b


@pytest.mark.parametrize("strategy", ["exact", "filter"])
@pytest.mark.parametrize("part", ["a", "b"])
def test_lists_that_overflow_and_the_two_error_statuses(part, strategy):
    """(a) hit counts orders of magnitude apart in one pass: more than 65,536 (exact range scan for the flagged query, which
    stays flagged, then paging), one stored row, under 100; (b) radius = the largest float: every live row for every query.
    Exact counts, the nearest min(count, 16384) hits, MLVDB_ERR_OVERFLOW with the nearest 100 at capacity 100,
    MLVDB_ERR_UNSUPPORTED with the nearest 16384 at capacity 20,000."""
    rows, deleted, qs, radius_a, want_a, nb, want_b = overflow_inputs()
    if part == "a":
        radius, want, n = radius_a, want_a, rows.shape[0]
        sizes = sizes_of(want)
        assert sizes[0] > RANGE_CAND_CAP and 1 <= sizes[1] and (sizes[2:] < 100).all(), f"precondition: counts {sizes}"
    else:
        radius, want, n = F32_MAX, want_b, nb
        sizes = sizes_of(want)
        live = n - int(deleted[:n].sum())
        assert (sizes == live).all() and CAND_CAP < live <= RANGE_CAND_CAP, f"precondition: counts {sizes}, {live} live rows"
    tag = f"overflow/{part}/{strategy}"
    eng = open_engine(rows[:n], "l2", strategy, deleted[:n], pieces=2)
    try:
        eng.last_stats()
        assert_range_matches(eng.range(qs, radius, 64), cut(want, PAGED), tag)
        st = eng.last_stats()
        assert st["strategy_used"] == STRATEGY_CODE[strategy], st
        if part == "a" and strategy == "filter":
            assert st["fallback_queries"] > 0, st
        rc, hits, cnt, off = packed_call(eng, qs, radius, 100, 400)
        assert rc == _native.ERR_OVERFLOW and np.array_equal(cnt, sizes), (tag, rc, cnt, sizes)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.minimum(sizes, 100))]))
        assert_range_matches(hits, cut(want, 100), tag + "/capacity 100")
        rc, hits, cnt, off = packed_call(eng, qs, radius, 20_000, 4 * PAGED)
        assert rc == ERR_UNSUPPORTED and np.array_equal(cnt, sizes), (tag, rc, cnt, sizes)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.minimum(sizes, PAGED))]))
        assert_range_matches(hits, cut(want, PAGED), tag + "/capacity 20000")
        rc, _, cnt, off = packed_call(eng, qs, radius, 20_000, 0)
        assert rc == _native.ERR_OVERFLOW and np.array_equal(cnt, sizes) and off[4] == np.minimum(sizes, PAGED).sum()
    finally:
        eng.close()


# ---------------------------------------------------------------- 3. rows exactly on the radius, ties between different rows
def integer_case(n, d, nq):
    rng = np.random.default_rng(7)
    rows = rng.integers(-2, 3, (n, d)).astype(np.float32)
    qs = rng.integers(-2, 3, (nq, d)).astype(np.float32)
    return rows, qs


@pytest.mark.parametrize("space", ["l2", "ip"])
@pytest.mark.parametrize("d,strategy", [(24, "exact"), (64, "exact"), (64, "filter")])
def test_rows_exactly_on_the_radius_are_hits(d, strategy, space):
    """Integer-valued rows and queries: every l2 / ip distance is an exact integer in fp64 whatever the summation order, so
    the kernels and the oracle must agree bit for bit on `<=`.  The radius is query 0's 41st smallest distance: rows exactly
    on it for every query (inclusive), equal distances among different rows ordered by label, distances equal to the last
    bit.  (ip: the radius is negative.)  d = 64: the 41st smallest lies so far out in the tail that 2 rows share it (l2) and
    one query has none on it; the 201st is shared by 15 or more, and by 7 or more for every query."""
    rows, qs = integer_case(5000, d, 6)
    dm = exact_scan.exact_distances(qs, rows, space)
    assert np.array_equal(dm, np.rint(dm)), "precondition: integer distances"
    radius = float(np.sort(dm[0])[40 if d == 24 else 200])
    assert float(np.float32(radius)) == radius
    on = (dm == radius).sum(axis=1)
    assert on[0] >= 10 and on.min() >= 1, f"precondition: rows exactly on the radius per query: {on}"
    want = exact_scan.range_query(qs, rows, radius, space)
    eng = open_engine(rows, space, strategy)
    try:
        got = eng.range(qs, radius, 64)
        assert eng.last_stats()["strategy_used"] == STRATEGY_CODE[strategy] or (strategy == "filter" and d < 64)
    finally:
        eng.close()
    tag = f"on-radius/{space}/{strategy}/d{d}"
    assert_range_matches(got, want, tag)
    for i, ((gl, gd), (wl, wd)) in enumerate(zip(got, want)):
        assert np.array_equal(gd, wd), f"{tag}: query {i}: distances differ in the last bit"


@pytest.mark.parametrize("strategy", ["exact", "filter"])
def test_radius_zero_returns_the_stored_row_and_its_duplicates(strategy):
    """l2, a query equal to a stored row that has two exact duplicates: radius 0.0 and -0.0 return exactly the three labels in
    label order, radius -1.0 nothing."""
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((5000, 64), dtype=np.float32)
    dups = [611, 2048, 4999]
    rows[dups[1]] = rows[dups[0]]
    rows[dups[2]] = rows[dups[0]]
    qs = rng.standard_normal((3, 64), dtype=np.float32)
    qs[1] = rows[dups[0]]
    wants = {r: exact_scan.range_query(qs, rows, r, "l2") for r in (0.0, -1.0)}
    assert [w[0].tolist() for w in wants[0.0]] == [[], dups, []] and sizes_of(wants[-1.0]).sum() == 0, "precondition"
    eng = open_engine(rows, "l2", strategy)
    try:
        for radius, key in ((0.0, 0.0), (-0.0, 0.0), (-1.0, -1.0)):
            got = eng.range(qs, radius, 64)
            assert_range_matches(got, wants[key], f"radius {radius!r}/{strategy}")
            if key == 0.0:
                assert got[1][0].tolist() == dups and not got[1][1].any()
    finally:
        eng.close()


@pytest.mark.parametrize("strategy", ["exact", "filter"])
def test_a_tie_group_across_the_8192nd_hit(strategy):
    """l2 on integer rows (20,000 of them: 5,000 rows hold no 8192 hits): the radius is query 0's 8192nd smallest distance and
    rows at that very distance continue beyond the 8192nd -- the query has more than kCandCap hits (paged exact kNN), and a
    capacity of 8192 cuts inside the tie group, where the label alone decides."""
    rows, qs = integer_case(20_000, 64, 3)
    s = np.sort(exact_scan.exact_distances(qs[:1], rows, "l2")[0])
    radius = float(s[CAND_CAP - 1])
    assert s[CAND_CAP] == radius and s[CAND_CAP - 2] == radius and float(np.float32(radius)) == radius, "precondition: ties"
    want = exact_scan.range_query(qs, rows, radius, "l2")
    assert len(want[0][0]) > CAND_CAP
    eng = open_engine(rows, "l2", strategy)
    try:
        assert_range_matches(eng.range(qs, radius, 64), want, f"tie-8192/{strategy}")
        assert_range_matches(eng.range(qs, radius, CAND_CAP, truncate=True), cut(want, CAND_CAP), f"tie-8192/{strategy}/cut")
    finally:
        eng.close()


# ---------------------------------------------------------------- 4. pass and query-tile edges
BATCH_SIZES = [1, 3, 4, 5, 8, 255, 256, 257, 513]


@functools.lru_cache(maxsize=None)
def batch_inputs(space):
    """6,000 rows x 128 drawn around 12 centres, 10 % tombstoned; 513 queries, the first two placed so that every batch holds a
    query deep inside a cluster and one far from every row.  One radius for all batches: the one that gives the 513 queries
    10 hits each on average."""
    n, d, nq = 6000, 128, 513
    rng = np.random.default_rng(4040)
    centres = rng.standard_normal((12, d), dtype=np.float32)
    rows = centres[rng.integers(0, 12, n)] * rng.random((n, 1), dtype=np.float32) + rng.standard_normal((n, d), dtype=np.float32)
    deleted = deleted_mask(4040, n, 0.1)
    qs = centres[rng.integers(0, 12, nq)] * rng.random((nq, 1), dtype=np.float32) + rng.standard_normal((nq, d), dtype=np.float32)
    qs[0] = centres[0]
    qs[1] = -centres[0] + 3.0 * rng.standard_normal(d, dtype=np.float32)
    dm = exact_scan.exact_distances(qs, rows[~deleted], space)
    radius = float(np.float32(np.partition(dm.ravel(), 10 * nq)[10 * nq]))
    want = exact_scan.range_query(qs, rows, radius, space, deleted=deleted)
    return rows, deleted, qs, radius, want


@pytest.mark.parametrize("strategy", ["exact", "filter"])
@pytest.mark.parametrize("space", ["cosine", "l2"])
@pytest.mark.parametrize("nq", BATCH_SIZES)
def test_pass_and_query_tile_edges(nq, space, strategy):
    """Batches around the exact scan's 4-query tile and the 256-query pass (513: two full passes and one query).  Query 0 has 30
    hits or more and query 1 none, so every batch of two or more holds an empty list beside a long one."""
    rows, deleted, qs, radius, want = batch_inputs(space)
    want, qs = want[:nq], qs[:nq]
    sizes = sizes_of(want)
    assert sizes[0] >= 30 and (nq == 1 or sizes[1] == 0), f"precondition: hits of queries 0, 1: {sizes[:2]}"
    assert 8 <= sizes_of(batch_inputs(space)[4]).mean() <= 12, "precondition: about 10 hits per query"
    eng = open_engine(rows, space, strategy, deleted)
    try:
        got = eng.range(qs, radius, 64)
        assert eng.last_stats()["strategy_used"] == STRATEGY_CODE[strategy]
    finally:
        eng.close()
    assert_range_matches(got, want, f"batch/{space}/{strategy}/nq{nq}")
    assert np.array_equal(got.offsets, np.concatenate([[0], np.cumsum(sizes)]))


# ---------------------------------------------------------------- 4b. the tail of the exact range scan's walk
# exact_range_kernel streams 16 x 2 rows per wave step and 16 x 2 x 8 = 256 per block step (panel_walk.h); the exact kNN
# tiles' block steps are 256 and 512 rows, and tests/test_gpu_knn_limits.py holds them to the same totals.
TAIL_COUNTS = [1, 15, 17, 255, 257, 511, 513]


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
@pytest.mark.parametrize("n", TAIL_COUNTS)
def test_exact_range_walk_tail_with_the_last_row_tombstoned(n, space):
    """The last row is a copy of query 0, well inside the radius, and tombstoned (where there is more than one row); the radius
    is the median distance, so about half the rows of every total are hits.  Batches of 1, 2, 3, 4 and 8 queries: full and
    half-filled tiles of four.  No fp64 distance lies within 1e-9 (relative) of the radius or of the next one of its query."""
    d = 20
    rng = np.random.default_rng(8800 + n)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((8, d), dtype=np.float32)
    deleted = np.zeros(n, dtype=bool)
    if n > 1:
        rows[n - 1] = qs[0]
        deleted[n - 1] = True
    dm = exact_scan.exact_distances(qs, rows, space)
    radius = float(np.float32(np.median(dm[:, ~deleted])))
    assert n == 1 or dm[0, n - 1] < radius, "precondition: the tombstoned row would be a hit"
    assert (np.abs(dm - radius) > 1e-9 * np.maximum(np.abs(dm), abs(radius))).all(), "precondition: a distance on the radius"
    srt = np.sort(dm[:, ~deleted], axis=1)
    assert (np.diff(srt, axis=1) > 1e-9 * np.abs(srt[:, 1:])).all(), "precondition: an accidental near-tie -- choose another seed"
    want = exact_scan.range_query(qs, rows, radius, space, deleted=deleted)
    assert n == 1 or sizes_of(want).sum() >= 2, "precondition: hits"
    eng = open_engine(rows, space, "exact", deleted)
    try:
        for nq in (1, 2, 3, 4, 8):
            got = eng.range(qs[:nq], radius, 64)
            assert eng.last_stats()["strategy_used"] == 1
            assert_range_matches(got, want[:nq], f"tail/exact/{space}/n{n}/nq{nq}")
            assert np.array_equal(got.offsets, np.concatenate([[0], np.cumsum(sizes_of(want[:nq]))]))
    finally:
        eng.close()


# ---------------------------------------------------------------- 5. wide rows
def wide_case(seed, n, d, nq, space):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    dm = exact_scan.exact_distances(qs, rows, space)
    radius = float(np.float32(np.sort(dm, axis=1)[:, 9].mean()))
    want = exact_scan.range_query(qs, rows, radius, space)
    return rows, qs, radius, want


@pytest.mark.parametrize("space", ["l2", "cosine"])
@pytest.mark.parametrize("d", [1536, 1552, 2048, 4096, 5120, 5136, 8192])
def test_wide_rows_through_the_exact_range_scan(d, space):
    """exact_range_kernel keeps its query tile in LDS as fp64: 8 bytes x ld per query.  The dims sit at and just past the widths
    at which four queries take 48 KiB (the default dynamic limit), 64 KiB and 160 KiB (all a CU has), up to the 8192 an index
    accepts.  700 rows (no multiple of 16 or 32), 5 queries (a full tile of four and one more)."""
    rows, qs, radius, want = wide_case(5000 + d, 700, d, 5, space)
    assert sizes_of(want).sum() >= 20, "precondition: hits"
    eng = open_engine(rows, space, "exact")
    try:
        got = eng.range(qs, radius, 64)
        assert eng.last_stats()["strategy_used"] == 1
    finally:
        eng.close()
    assert_range_matches(got, want, f"wide/exact/{space}/d{d}")


@pytest.mark.parametrize("space", ["l2", "cosine"])
@pytest.mark.parametrize("d", [4096, 8192])
def test_wide_rows_through_the_filter(d, space):
    rows, qs, radius, want = wide_case(6000 + d, 3000, d, 5, space)
    assert 20 <= sizes_of(want).sum() and sizes_of(want).max() < CAND_CAP, "precondition: hits, no list overflows"
    eng = open_engine(rows, space, "filter", pieces=2)
    try:
        got = eng.range(qs, radius, 64)
        st = eng.last_stats()
        assert st["strategy_used"] == 2 and st["fallback_queries"] == 0, st
    finally:
        eng.close()
    assert_range_matches(got, want, f"wide/filter/{space}/d{d}")


def test_widest_rows_reach_the_exact_range_scan_from_a_filter_pass():
    """d = 8192, filter strategy, radius = the largest float (every row hits for every query): the queries a filter pass flags
    are redone by launch_exact_range_scan with a qsel list.  70,001 such rows are 2.3 GB and half a minute of oracle; 3,000 rows
    reach the same launch because an l2 pass takes a query whose int8 image is useless (here one 100 x and one 1000 x off the
    others' scale) off the filter and flags it like a list overflow (filter_l2_offsets_kernel)."""
    n, d = 3000, 8192
    rng = np.random.default_rng(8192)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((8, d), dtype=np.float32)
    qs[2] *= 100.0
    qs[5] *= 1e-3
    want = exact_scan.range_query(qs, rows, F32_MAX, "l2")
    assert (sizes_of(want) == n).all(), "precondition: every row hits"
    eng = open_engine(rows, "l2", "filter")
    try:
        eng.last_stats()
        got = eng.range(qs, F32_MAX, 64)
        st = eng.last_stats()
        assert st["strategy_used"] == 2 and st["fallback_queries"] >= 1, st
    finally:
        eng.close()
    assert_range_matches(got, want, "wide/filter-overflow/l2/d8192")


# ---------------------------------------------------------------- 6. the fp16 mid shadow follows the index
@functools.lru_cache(maxsize=None)
def shadow_sequence(space):
    """Inputs and the oracle's answer after every step of: append 20,000 -> append 10,007 -> tombstone the hits of query 0 ->
    compact -> reset, append 4,000."""
    d, n1, n2, n3 = 192, 20_000, 10_007, 4_000
    rng = np.random.default_rng(606)
    rows = rng.standard_normal((n1 + n2, d), dtype=np.float32)
    qs = rng.standard_normal((24, d), dtype=np.float32)
    dm = exact_scan.exact_distances(qs, rows, space)
    radius = float(np.float32(np.median(np.sort(dm, axis=1)[:, 39])))  # half the queries have 40 hits or more on the 30,007 rows
    w1 = exact_scan.range_query(qs, rows[:n1], radius, space)
    w2 = exact_scan.range_query(qs, rows, radius, space)
    dead = np.zeros(n1 + n2, dtype=bool)
    dead[w2[0][0]] = True
    w3 = exact_scan.range_query(qs, rows, radius, space, deleted=dead)
    w4 = exact_scan.range_query(qs, rows[~dead], radius, space)
    w5 = exact_scan.range_query(qs, rows[:n3], radius, space)
    assert 20 <= np.median(sizes_of(w2)) <= 80 and dead.any(), "precondition: about 40 hits per query, query 0 has some"
    assert sum(int((w[0] >= n1).sum()) for w in w2) >= 100, "precondition: hits among the rows the shadow is extended by"
    assert min(sizes_of(w).sum() for w in (w1, w3, w4, w5)) > 0, "precondition: hits at every step"
    return rows, qs, radius, dead, (w1, w2, w3, w4, w5), (n1, n3)


@pytest.mark.parametrize("shadow", [1, 0])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_mid_shadow_follows_appends_tombstones_compact_and_reset(space, shadow):
    """attach_mid builds the fp16 shadow at the first range call, extends it from l2_rows at the next (the last 16-row panel is
    shared between the two appends and the capacity regrows), and rebuilds it after compact and reset.  Every step against the
    oracle on the rows live at that step; L2_SHADOW=0 (no mid bounds at all) must give the same ids."""
    rows, qs, radius, dead, (w1, w2, w3, w4, w5), (n1, n3) = shadow_sequence(space)
    eng = HipScanEngine(rows.shape[1], space, device=0, strategy="filter")
    try:
        eng.set_tuning(L2_SHADOW=shadow)
        tag = f"mid-shadow={shadow}/{space}"
        eng.append(rows[:n1])
        assert_range_matches(eng.range(qs, radius, 64), w1, tag + "/built")
        assert eng.last_stats()["strategy_used"] == 2
        eng.append(rows[n1:])
        assert_range_matches(eng.range(qs, radius, 64), w2, tag + "/extended")
        assert eng.tombstone(np.nonzero(dead)[0]) == int(dead.sum())
        assert_range_matches(eng.range(qs, radius, 64), w3, tag + "/tombstoned")
        old = eng.compact()
        assert np.array_equal(old, np.nonzero(~dead)[0])
        assert_range_matches(eng.range(qs, radius, 64), w4, tag + "/compacted")
        eng.reset()
        eng.append(rows[:n3])
        assert_range_matches(eng.range(qs, radius, 64), w5, tag + "/reset")
        assert eng.last_stats()["strategy_used"] == 2
    finally:
        eng.close()


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_mid_shadow_with_a_huge_row_and_an_outlier_component(space):
    """shadow16_rows_kernel converts a row to fp16 with one scale per row.  A row scaled by 1e12 and a row with one 40-sigma
    component, each once in the rows the first range call converts and once in the rows the second call extends the shadow
    by; query 0 sits next to the first outlier row, query 1 next to the second, queries 2 and 3 point along the huge rows."""
    d, n1, n = 192, 10_000, 20_000
    rng = np.random.default_rng(616)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((24, d), dtype=np.float32)
    huge, odd = (5_005, 15_005), (5_009, 15_009)
    for j, (hg, od) in enumerate(zip(huge, odd)):
        rows[od, 3 + j] = 40.0
        qs[j] = rows[od] + 0.1 * qs[j]
        qs[2 + j] = rows[hg] + 0.1 * qs[2 + j]
        rows[hg] *= np.float32(1e12)
    typical = np.arange(4, 24)
    dm = exact_scan.exact_distances(qs, rows, space)
    radius = float(np.float32(np.sort(dm[typical], axis=1)[:, 39].mean()))
    w1 = exact_scan.range_query(qs, rows[:n1], radius, space)
    w2 = exact_scan.range_query(qs, rows, radius, space)
    assert odd[0] in w1[0][0] and odd[0] in w2[0][0] and odd[1] in w2[1][0], "precondition: the outlier rows are hits"
    if space != "l2":  # (l2: a row 1e12 long is within no radius of a query of length 14)
        assert huge[0] in w1[2][0] and huge[1] in w2[3][0], "precondition: the huge rows are hits"
    eng = HipScanEngine(d, space, device=0, strategy="filter")
    try:
        eng.append(rows[:n1])
        assert_range_matches(eng.range(qs, radius, 64), w1, f"mid-hostile/{space}/built")
        eng.append(rows[n1:])
        assert_range_matches(eng.range(qs, radius, 64), w2, f"mid-hostile/{space}/extended")
    finally:
        eng.close()


# ---------------------------------------------------------------- 7. scale extremes through range
@pytest.mark.parametrize("strategy", ["exact", "filter"])
@pytest.mark.parametrize("space", ["cosine", "l2", "ip"])
def test_zero_rows_zero_queries_and_scale_extremes_through_range(space, strategy):
    """The inputs of test_gpu_parity.test_zero_rows_zero_queries_and_scale_extremes: a zero row, a 1e-18 row, a 1e12 row, a zero
    query and a 1e-15 query; the radius is the mean 8th-nearest distance of the well-scaled queries."""
    rng = np.random.default_rng(41)
    rows = rng.standard_normal((3000, 64)).astype(np.float32)
    rows[5] = 0.0
    rows[6] *= 1e-18
    rows[7] *= 1e12
    qs = rng.standard_normal((12, 64)).astype(np.float32)
    qs[1] = 0.0
    qs[2] *= 1e-15
    well = np.delete(np.arange(12), [1, 2])
    dm = exact_scan.exact_distances(qs[well], rows, space)
    radius = float(np.float32(np.sort(dm, axis=1)[:, 7].mean()))
    want = exact_scan.range_query(qs, rows, radius, space)
    assert sizes_of(want)[well].sum() >= 20, "precondition: hits"
    eng = open_engine(rows, space, strategy)
    try:
        got = eng.range(qs, radius, 64)
    finally:
        eng.close()
    assert_range_matches(got, want, f"extremes/{space}/{strategy}")
