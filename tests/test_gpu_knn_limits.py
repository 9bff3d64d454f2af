"""Plain kNN (mlvdb_search_batch, HipScanEngine.search) against the NumPy oracle at the limits of its kernels.

The reference is always oracle.exact_scan.knn / exact_distances (fp64), never the engine's other strategy; every case builds
its inputs from a seed and asserts its preconditions on the oracle alone before the first GPU call.  Ids and counts are
bit-exact, fp32 distances within tests.helpers.SCORE_ATOL.  Intended ties are bit-identical duplicate rows; at every cut a
case depends on (rank k | k + 1, a page edge) the two fp64 distances are bit-equal or more than 1e-9 relative apart
(knn_limits_helpers.assert_cuts).  Sizes are the smallest at which the named edge exists (DESIGN sections 5.1, 5.4 and 5.5
list the limits pinned here):

* A. exact_scan_kernel / exact_merge_kernel: the query tiles 8 / 4 / 2 / 1 by batch and by row width (plan_exact halves the
  tile while its fp64 image is above 64 KiB), row counts around panels, wave tasks and blocks, k = 1 .. 64 with tie groups
  across rank k, the 64-entry pages of top_k > 64 up to MLVDB_MAX_TOPK_PAGED, and a call of more query tiles (65,537) than
  one grid takes in its y dimension.  At a tile of one query (ld > 4096) the same limit is 65,535 queries -- more than 1 GB of
  queries, so it has no GPU case: run_exact derives its slabs from the number of query TILES, which covers it.
  (Queries of one plain call all see the same live rows, so "one query exhausted beside one that is not" cannot be built
  here; the range limits file reaches run_paged_exact with a query selection.)
* B. the k <= 64 filter pass with SEED_ROWS=1, ROUND1=6, ROUND2=7: a dense seed on rows [0, 768) and scan rounds
  [768, 4608), [4608, 5376), [5376, total) -- all three rounds, and the refines between them, on 6,200 rows.
* C. the routes by top_k (64 | 65, 1024 | 1025, 16384 | 16385, live > k) and big-k passes with many rounds (BIGK_BUDGET).
"""
import functools

import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd.engine import HipScanEngine
from tests import knn_limits_helpers as H
from tests.helpers import assert_knn_matches, deleted_mask, make_case

pytestmark = pytest.mark.gpu

SPACES = ["l2", "cosine", "ip"]
ERR_UNSUPPORTED = 6  # include/mlvdb_hip.h: MLVDB_ERR_UNSUPPORTED
PAGED = _native.MAX_TOPK_PAGED
PAGE = _native.MAX_TOPK


def open_engine(rows, space, strategy, deleted=None, pieces=1, **knobs):
    eng = HipScanEngine(rows.shape[1], space, device=0, strategy=strategy)
    try:
        if knobs:
            eng.set_tuning(**knobs)
        for part in np.array_split(rows, pieces):
            eng.append(part)
        if deleted is not None and deleted.any():
            assert eng.tombstone(np.nonzero(deleted)[0]) == int(deleted.sum())
    except Exception:
        eng.close()
        raise
    return eng


def search(eng, qs, k):
    """One search -> (answer, the statistics of this call alone: they accumulate between reads)."""
    eng.last_stats()
    got = eng.search(qs, k)
    return got, eng.last_stats()


def scaled_case(seed, n, d, nq):
    """Rows and queries scaled by 1 / sqrt(d): l2 distances stay O(1) at any width and the absolute bar applies as it stands."""
    rng = np.random.default_rng(seed)
    s = np.float32(1.0 / np.sqrt(d))
    return rng.standard_normal((n, d), dtype=np.float32) * s, rng.standard_normal((nq, d), dtype=np.float32) * s, rng


# ================================================================ A. the exact scan
@pytest.mark.parametrize("space", SPACES)
def test_exact_query_tile_by_batch(space):
    """nq = 1 .. 17 at d = 100: the QT = 1 / 2 / 4 / 8 bodies with full and ragged last tiles (9 = 8 + 1, 17 = 8 + 8 + 1); 1,037
    rows, tombstones, the duplicate rows of make_case(dup=True) (query 0 is one of three identical rows)."""
    rows, qs = make_case(6, 1037, 100, 17, dup=True)
    deleted = deleted_mask(6, 1037, 0.1)
    k = 7
    H.assert_cuts(qs, rows, space, [k], deleted, "batch tiles")
    want = H.oracle_knn(qs, rows, k, space, deleted)
    eng = open_engine(rows, space, "exact", deleted, pieces=3)
    try:
        for nq in (1, 2, 3, 4, 5, 7, 8, 9, 17):
            got, st = search(eng, qs[:nq], k)
            assert st["strategy_used"] == 1 and st["scan_launches"] == 1, st
            # (rows_scanned counts every row once per query tile: the tile the launch really took)
            assert st["rows_scanned"] == 1037 * H.plan_exact(1037, H.layout_ld(100), nq).nqtiles, (nq, st)
            assert_knn_matches(got, tuple(w[:nq] for w in want), f"exact-batch/{space}/nq{nq}")
    finally:
        eng.close()


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("d", [1024, 1025, 2048, 2049, 4096, 4097, 8192])
def test_exact_query_tile_by_row_width(d, space):
    """plan_exact halves the query tile while QT x ld x 8 B is above 64 KiB: the widths at and just past each halving, each with
    9, 3 and 1 queries.  1,003 rows, 10 % tombstoned; rows 495 | 496 (a 16-row panel edge) are bit-identical and nearest to
    query 0."""
    n, k = 1003, 10
    rows, qs, rng = scaled_case(7000 + d, n, d, 9)
    deleted = deleted_mask(7000 + d, n, 0.1)
    deleted[[495, 496]] = False
    H.plant_pair(rows, qs, space, 0, 495, 496, rng)
    ld = H.layout_ld(d)
    tiles = [H.plan_exact(n, ld, nq).qt for nq in (9, 3, 1)]
    assert tiles == [8 if ld <= 1024 else 4 if ld <= 2048 else 2 if ld <= 4096 else 1,
                     2 if ld <= 4096 else 1, 1], f"precondition: query tiles {tiles} at ld {ld}"
    assert all(H.plan_exact(n, ld, nq).lds_bytes <= 64 * 1024 for nq in (9, 3, 1)), "precondition: the plan fits 64 KiB of LDS"
    srt, lab = H.assert_cuts(qs, rows, space, [1, 2, k], deleted, f"wide d{d}")
    assert lab[0, :2].tolist() == [495, 496] and srt[0, 0] == srt[0, 1], "precondition: the duplicated pair leads query 0"
    want = H.oracle_knn(qs, rows, k, space, deleted, slab=3)
    eng = open_engine(rows, space, "exact", deleted)
    try:
        for nq in (9, 3, 1):
            got, st = search(eng, qs[:nq], k)
            assert st["strategy_used"] == 1, st
            # rows_scanned counts every row once per query tile: the launch took the halved tile, not a wider one
            assert st["rows_scanned"] == n * H.plan_exact(n, ld, nq).nqtiles, f"d{d}/nq{nq}: {st}, {H.plan_exact(n, ld, nq)}"
            assert_knn_matches(got, tuple(w[:nq] for w in want), f"exact-wide/{space}/d{d}/nq{nq}")
    finally:
        eng.close()


# 16 x PW x NW rows per block: 512 for (PW, NW) = (2, 16) [QT 1, 2] and (4, 8) [QT 4], 256 for (2, 8) [QT 8].
# 1,100 rows are 69 panels: 35 tasks of two panels for 16 or 8 waves (3 / 5 blocks), 18 tasks of four for 8 waves (3 blocks) --
# plan_exact gives every query tile of 2, 4 and 9 queries more than one block, so exact_merge_kernel folds nblk x k partial
# entries, and the last row belongs to another block and another wave than row 0.
ROW_COUNTS = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1100]


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_exact_row_counts_around_panels_tasks_and_blocks(n, space):
    """Rows 0 and n - 1 are bit-identical and nearest to query 0: from 255 rows on they belong to different waves, at 1,100 to
    different blocks.  Batches of 2, 4 and 9 queries: every (PW, NW) pair of kExactTiles."""
    d, k = 24, 5
    rng = np.random.default_rng(7100 + n)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((9, d), dtype=np.float32)
    deleted = np.zeros(n, dtype=bool)
    if n >= 31:
        deleted[[3, n // 2]] = True
    if n >= 2:
        H.plant_pair(rows, qs, space, 0, 0, n - 1, rng)
    for nq in (2, 4, 9):
        plan = H.plan_exact(n, H.layout_ld(d), nq)
        (b0, w0), (b1, w1) = H.exact_owner(0, plan), H.exact_owner(n - 1, plan)
        assert n < 255 or (b0, w0) != (b1, w1), "precondition: the two copies are scored by different waves"
        assert n < 1100 or (plan.nblk > 1 and b0 != b1 and w0 != w1), f"precondition: {plan}: several blocks per query tile"
    srt, lab = H.assert_cuts(qs, rows, space, [1, 2, k], deleted, f"rows n{n}")
    if n >= 2:
        assert lab[0, :2].tolist() == [0, n - 1] and srt[0, 0] == srt[0, 1], "precondition: the duplicated pair leads query 0"
    want = H.oracle_knn(qs, rows, k, space, deleted)
    assert (want[2] == min(k, n - int(deleted.sum()))).all()
    eng = open_engine(rows, space, "exact", deleted)
    try:
        for nq in (2, 4, 9):
            got, st = search(eng, qs[:nq], k)
            assert st["strategy_used"] == 1, st
            assert_knn_matches(got, tuple(w[:nq] for w in want), f"exact-rows/{space}/n{n}/nq{nq}")
    finally:
        eng.close()


# The tail of the streamed walk (panel_walk.h): totals at and around one wave step (16 x PW rows) and one block step of each
# tile (16 x PW x NW rows, above), the last row tombstoned -- a case the counts above leave out: their last row is live.
TAIL_COUNTS = [1, 15, 17, 255, 257, 511, 513]


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", TAIL_COUNTS)
def test_exact_walk_tail_with_the_last_row_tombstoned(n, space):
    """The last row is the nearest of query 0 and tombstoned (where there is more than one row): a walk that scored it as live,
    or one that stopped a panel short, returns other ids.  Batches of 1, 2, 3, 4 and 8 queries: every tile, and the half-filled
    tile of 4."""
    d, k = 20, 3
    rng = np.random.default_rng(7900 + n)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((8, d), dtype=np.float32)
    deleted = np.zeros(n, dtype=bool)
    if n > 1:
        H.plant(rows, qs, space, [(0, n - 1)], rng)
        H.assert_rank0(qs, rows, space, [(0, n - 1)])
        deleted[n - 1] = True
    H.assert_cuts(qs, rows, space, [1, 2, k], deleted, f"tail n{n}")
    want = H.oracle_knn(qs, rows, k, space, deleted)
    assert (want[2] == min(k, n - int(deleted.sum()))).all()
    assert n == 1 or not (want[0] == n - 1).any(), "precondition: the oracle leaves the tombstoned row out"
    eng = open_engine(rows, space, "exact", deleted)
    try:
        for nq in (1, 2, 3, 4, 8):
            got, st = search(eng, qs[:nq], k)
            assert st["strategy_used"] == 1, st
            assert_knn_matches(got, tuple(w[:nq] for w in want), f"exact-tail/{space}/n{n}/nq{nq}")
    finally:
        eng.close()


@pytest.mark.parametrize("space", SPACES)
def test_exact_k_with_tie_groups_across_rank_k(space):
    """200 live rows of 230: three identical rows at ranks 0-2 of query 0 (the cuts k = 1 and 2 lie inside), four at ranks 62-65
    of query 1 (k = 63 and 64); 40 live rows of 50 with k = 64: padding, counts = 40."""
    n, d = 230, 32
    rng = np.random.default_rng(7200)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((6, d), dtype=np.float32)
    deleted = np.zeros(n, dtype=bool)
    deleted[rng.choice(n, 30, replace=False)] = True
    first3 = np.nonzero(~deleted)[0][[10, 90, 170]]
    H.plant_pair(rows, qs, space, 0, first3[0], first3[1], rng)
    rows[first3[2]] = rows[first3[0]]
    group = H.plant_tie_group(rows, qs, space, 1, 62, 4, deleted)
    srt, lab = H.assert_cuts(qs, rows, space, [1, 2, 3, 62, 63, 64, 66], deleted, "k")
    assert lab[0, :3].tolist() == first3.tolist() and srt[0, 0] == srt[0, 2], "precondition: ranks 0-2 of query 0 tie"
    assert lab[1, 62:66].tolist() == group.tolist() and srt[1, 62] == srt[1, 65] and srt[1, 61] < srt[1, 62] < srt[1, 66], \
        "precondition: ranks 62-65 of query 1 tie, and only those"
    eng = open_engine(rows, space, "exact", deleted)
    try:
        for k in (1, 2, 63, 64):
            got, st = search(eng, qs, k)
            assert st["strategy_used"] == 1, st
            assert_knn_matches(got, H.oracle_knn(qs, rows, k, space, deleted), f"exact-k/{space}/k{k}")
    finally:
        eng.close()
    few_deleted = np.zeros(50, dtype=bool)
    few_deleted[::5] = True
    want = H.oracle_knn(qs, rows[:50], 64, space, few_deleted)
    assert (want[2] == 40).all() and (want[0][:, 40:] == -1).all()
    eng = open_engine(rows[:50], space, "exact", few_deleted)
    try:
        got, _ = search(eng, qs, 64)
        assert_knn_matches(got, want, f"exact-k/{space}/40 live rows")
    finally:
        eng.close()


@pytest.mark.parametrize("space", SPACES)
def test_paged_topk_with_tie_groups_across_page_edges(space):
    """run_paged_exact returns 64 entries per page, the next page strictly after the cursor (distance, label) of the last: five
    identical rows at ranks 62-66 of query 0 and five at ranks 126-130 lie across the first two page edges."""
    n, d = 500, 24
    rng = np.random.default_rng(7300)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((5, d), dtype=np.float32)
    deleted = deleted_mask(7300, n, 0.1)
    g2 = H.plant_tie_group(rows, qs, space, 0, 126, 5, deleted)
    g1 = H.plant_tie_group(rows, qs, space, 0, 62, 5, deleted)
    srt, lab = H.assert_cuts(qs, rows, space, [62, 64, 65, 67, 126, 128, 129, 131], deleted, "paged ties")
    assert lab[0, 62:67].tolist() == g1.tolist() and srt[0, 62] == srt[0, 66] and srt[0, 61] < srt[0, 62] < srt[0, 67]
    assert lab[0, 126:131].tolist() == g2.tolist() and srt[0, 126] == srt[0, 130] and srt[0, 125] < srt[0, 126] < srt[0, 131]
    eng = open_engine(rows, space, "exact", deleted)
    try:
        for k in (65, 128, 129):
            got, st = search(eng, qs, k)
            assert st["strategy_used"] == 1 and st["scan_launches"] == -(-k // PAGE), st
            assert_knn_matches(got, H.oracle_knn(qs, rows, k, space, deleted), f"paged-ties/{space}/k{k}")
    finally:
        eng.close()


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("live", [64, 65, 100])
def test_paged_topk_beyond_the_live_rows(live, space):
    """k = 129 (three pages) on 64, 65 and 100 live rows: a query exhausted on page 0 / 1 must find nothing on the later pages
    (its cursor is parked at +inf), the answer is padded and counts = the live rows."""
    n, d, k = live + 20, 24, 129
    rng = np.random.default_rng(7400 + live)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((5, d), dtype=np.float32)
    deleted = np.zeros(n, dtype=bool)
    deleted[rng.choice(n, 20, replace=False)] = True
    H.assert_cuts(qs, rows, space, [64], deleted, "paged exhausted")
    want = H.oracle_knn(qs, rows, k, space, deleted)
    assert (want[2] == live).all() and (want[0][:, live:] == -1).all()
    eng = open_engine(rows, space, "exact", deleted)
    try:
        got, st = search(eng, qs, k)
        assert st["strategy_used"] == 1 and st["scan_launches"] == 3, st
        assert_knn_matches(got, want, f"paged-exhausted/{space}/live{live}")
    finally:
        eng.close()


@pytest.mark.parametrize("space", SPACES)
def test_paged_topk_at_its_maximum_and_one_beyond(space):
    """k = MLVDB_MAX_TOPK_PAGED = 16,384 on 20,000 x 16: 256 pages against the oracle's whole ranking, every page edge a cut;
    k = 16,385: MLVDB_ERR_UNSUPPORTED and the outputs untouched."""
    rows, qs, _ = scaled_case(7500, 20_000, 16, 2)
    H.assert_cuts(qs, rows, space, range(PAGE, PAGED + 1, PAGE), None, "paged maximum")
    want = H.oracle_knn(qs, rows, PAGED, space)
    eng = open_engine(rows, space, "auto")
    try:
        got, st = search(eng, qs, PAGED)
        assert st["strategy_used"] == 1 and st["scan_launches"] == PAGED // PAGE, st
        assert_knn_matches(got, want, f"paged-max/{space}")
        k = PAGED + 1
        lab = np.full((2, k), -9, dtype=np.int64)
        dist = np.full((2, k), -9.0, dtype=np.float32)
        cnt = np.full(2, -9, dtype=np.int32)
        rc = eng._lib.mlvdb_search_batch(eng.handle, qs.ctypes.data, 2, k, lab.ctypes.data, dist.ctypes.data, cnt.ctypes.data)
        assert rc == ERR_UNSUPPORTED, rc
        assert (lab == -9).all() and (dist == -9.0).all() and (cnt == -9).all(), "a refused call wrote to its outputs"
    finally:
        eng.close()


def test_exact_scan_of_more_query_tiles_than_one_grid_takes():
    """MLVDB_STRATEGY_AUTO sends any index of under 32,768 rows to the exact scan whatever nq is: 8 x 65,535 + 16 = 524,296
    queries are 65,537 tiles of eight, more than a grid's y dimension is documented to take (65,535).  64 rows x 8, k = 2; the
    oracle goes in slabs.  Every query's answer, and by name the first, the last and those on both sides of query 524,280."""
    n, d, k = 64, 8, 2
    edge = 8 * 65_535
    nq = edge + 16
    rng = np.random.default_rng(7600)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    assert H.plan_exact(n, H.layout_ld(d), nq).nqtiles == 65_537
    wl, wd, w64 = H.oracle_topk_dense(qs, rows, k, "cosine")
    ok = H.gap_ok(w64[:, 0], w64[:, 1]) & H.gap_ok(w64[:, 1], w64[:, 2])
    assert ok.all(), f"precondition: accidental near-tie for queries {np.nonzero(~ok)[0][:5]} -- choose another seed"
    eng = open_engine(rows, "cosine", "auto")
    try:
        (gl, gd, gc), st = search(eng, qs, k)
        assert st["strategy_used"] == 1 and st["scan_launches"] >= 1, st
    finally:
        eng.close()
    for i in (0, edge - 1, edge, nq - 1):
        assert gl[i].tolist() == wl[i].tolist() and gc[i] == k, f"query {i}: got {gl[i]} (count {gc[i]}), the oracle has {wl[i]}"
    assert_knn_matches((gl, gd, gc), (wl, wd, np.full(nq, k, dtype=np.int32)), "exact-many-tiles")


# ================================================================ B. the k <= 64 filter pass at its round boundaries
SHORT_ROUNDS = dict(SEED_ROWS=1, ROUND1=6, ROUND2=7)  # seed [0, 768), rounds [768, 4608) [4608, 5376) [5376, total)
BOUNDARIES = (768, 4608, 5376)
# one boundary row per space is tombstoned: it holds the nearest copy of its query all the same, and a live copy stands beside it
DEAD_BOUNDARY_ROW = {"l2": (4607, 4606), "cosine": (768, 769), "ip": (5375, 5374)}


@functools.lru_cache(maxsize=4)
def boundary_case(total, d, space):
    """12 queries on `total` rows, 5 % tombstoned.  Queries 0-7: a near copy at rows 0, 767, 768, 4607, 4608, 5375, 5376 and
    total - 1 (those that exist); queries 8-10: a bit-identical pair at rows b - 3 and b + 2 of each boundary b (where b + 2
    exists); query 11 has nothing planted.  -> rows, qs, deleted, placements, pairs, the oracle's answer for k = 10."""
    rng = np.random.default_rng(9000 + 7 * total + d)
    rows = rng.standard_normal((total, d), dtype=np.float32)
    qs = rng.standard_normal((12, d), dtype=np.float32)
    deleted = deleted_mask(9000 + total + d, total, 0.05)
    planted = []
    for r in (0, 767, 768, 4607, 4608, 5375, 5376, total - 1):
        if r < total and r not in planted:
            planted.append(r)
    placements = list(enumerate(planted))
    deleted[planted] = False
    H.plant(rows, qs, space, placements, rng)
    dead, stand_in = DEAD_BOUNDARY_ROW[space]
    has_dead = dead in planted and stand_in < total and stand_in not in planted
    if has_dead:
        q = planted.index(dead)
        rows[dead] = H.near_copy(qs[q], space, rng, eps=0.005)
        deleted[dead] = True
        deleted[stand_in] = False
        placements[q] = (q, stand_in)
        H.plant(rows, qs, space, [placements[q]], rng)
    pairs = []
    for j, b in enumerate(BOUNDARIES):
        if b + 2 < total and b + 2 not in planted:
            H.plant_pair(rows, qs, space, 8 + j, b - 3, b + 2, rng)
            deleted[[b - 3, b + 2]] = False
            pairs.append((8 + j, b - 3, b + 2))
    H.assert_rank0(qs, rows, space, placements, deleted)
    srt, lab = H.assert_cuts(qs, rows, space, [1, 2, 10], deleted, f"boundaries total {total}")
    for q, ra, rb in pairs:
        assert lab[q, :2].tolist() == [ra, rb] and srt[q, 0] == srt[q, 1], "precondition: the pair across the boundary leads"
    if total == 6200:
        assert has_dead and deleted[dead] and (planted.index(dead), stand_in) in placements, "precondition: a boundary row is tombstoned"
    return rows, qs, deleted, placements, pairs, H.oracle_knn(qs, rows, 10, space, deleted)


def assert_rounds(st, passes, tag):
    """passes: the rounds [(b, e), ..] of every pass of the call (knn_limits_helpers.filter_rounds / filter_call_rounds)."""
    assert st["strategy_used"] == 2, (tag, st)
    launches, scanned = sum(len(r) for r in passes), sum(e - b for r in passes for b, e in r)
    assert st["scan_launches"] == launches, f"{tag}: {st['scan_launches']} scan launches, passes of rounds {passes} expected"
    assert st["rows_scanned"] == scanned, f"{tag}: {st['rows_scanned']} rows scanned, passes of rounds {passes} expected"


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("d", [256, 100, 64])
@pytest.mark.parametrize("total", [767, 768, 769, 4607, 4608, 4609, 5375, 5376, 5377, 6200])
def test_filter_pass_at_its_round_boundaries(total, d, space):
    """The native int8 shadow (d = 256), the zero-padded one (100) and the bf16 body (64), with the last row one below, at and
    above every round boundary.  scan_launches = the non-empty rounds of run_filter_pass: the keys took effect."""
    rows, qs, deleted, _, _, want = boundary_case(total, d, space)
    rounds = H.filter_rounds(total, 1, 6, 7)
    assert len(rounds) == sum(total > b for b in BOUNDARIES)
    eng = open_engine(rows, space, "filter", deleted, pieces=2, **SHORT_ROUNDS)
    try:
        got, st = search(eng, qs, 10)
    finally:
        eng.close()
    assert_rounds(st, [rounds], f"rounds/{space}/d{d}/n{total}")
    assert_knn_matches(got, want, f"rounds/{space}/d{d}/n{total}")


@pytest.mark.parametrize("space", SPACES)
def test_filter_pass_under_other_pass_structure_knobs(space):
    """The 6,200-row corpus again: REFINE_PICKS = 16 and 48 (the refine between the rounds scores fewer / more picks), SEED_ROWS=5
    ROUND1=6 ROUND2=6 (a second round of no rows), and 1 and 2 queries under SMALL_BATCH=0 with the short rounds (the exact
    prefix seed, so the first round starts at row 0, and the fused finish)."""
    total = 6200
    rows, qs, deleted, _, _, want = boundary_case(total, 256, space)
    eng = open_engine(rows, space, "filter", deleted, pieces=2, **SHORT_ROUNDS)
    try:
        for picks in (16, 48):
            eng.set_tuning(REFINE_PICKS=picks)
            got, st = search(eng, qs, 10)
            assert_rounds(st, [H.filter_rounds(total, 1, 6, 7)], f"picks{picks}/{space}")
            assert_knn_matches(got, want, f"picks{picks}/{space}")
        eng.set_tuning(REFINE_PICKS=0, SEED_ROWS=5, ROUND1=6, ROUND2=6)
        rounds = H.filter_rounds(total, 5, 6, 6)
        assert rounds == [(3840, 4608), (4608, total)]
        got, st = search(eng, qs, 10)
        assert_rounds(st, [rounds], f"empty-round/{space}")
        assert_knn_matches(got, want, f"empty-round/{space}")
        eng.set_tuning(SMALL_BATCH=0, **SHORT_ROUNDS)
        rounds = H.filter_rounds(total, 1, 6, 7, prefix_seed=True)
        assert rounds == [(0, 4608), (4608, 5376), (5376, total)]
        for nq in (1, 2):
            got, st = search(eng, qs[:nq], 10)
            assert st["bound_dtype"] == 2, st  # the int8 shadow served the pass: the small-batch seed and finish apply
            assert_rounds(st, [rounds], f"small/{space}/nq{nq}")
            assert_knn_matches(got, tuple(w[:nq] for w in want), f"small/{space}/nq{nq}")
    finally:
        eng.close()


@functools.lru_cache(maxsize=1)
def pass_case(space):
    """6,200 x 256 and 513 queries; the last query of each 256-query pass and the first of the next (254 | 255 | 256 | 257,
    511 | 512) query a row planted at a round boundary, query 0 row 0 and query 1 the last row."""
    total, d, nq = 6200, 256, 513
    rng = np.random.default_rng(9500)
    rows = rng.standard_normal((total, d), dtype=np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    deleted = deleted_mask(9500, total, 0.05)
    placements = [(0, 0), (1, total - 1), (254, 767), (255, 768), (256, 4607), (257, 4608), (511, 5375), (512, 5376)]
    deleted[[r for _, r in placements]] = False
    H.plant(rows, qs, space, placements, rng)
    H.assert_rank0(qs, rows, space, placements, deleted)
    H.assert_cuts(qs, rows, space, [10], deleted, "passes")
    return rows, qs, deleted, H.oracle_knn(qs, rows, 10, space, deleted, slab=128)


@pytest.mark.parametrize("space", SPACES)
def test_filter_query_passes_with_short_rounds(space):
    """255 / 256 / 257 / 513 queries: q0 offsets every output of the second and third pass; scan_launches = passes x rounds.
    (The one-query last pass of 257 and 513 takes the exact prefix seed: its first round starts at row 0.)"""
    rows, qs, deleted, want = pass_case(space)
    eng = open_engine(rows, space, "filter", deleted, pieces=2, **SHORT_ROUNDS)
    try:
        for nq in (255, 256, 257, 513):
            passes = H.filter_call_rounds(rows.shape[0], nq, 1, 6, 7, int8=True)
            assert len(passes) == -(-nq // H.FILTER_QUERIES) and all(len(r) == 3 for r in passes)
            got, st = search(eng, qs[:nq], 10)
            assert st["bound_dtype"] == 2, st  # (the int8 shadow serves d = 256: what filter_call_rounds was told)
            assert_rounds(st, passes, f"passes/{space}/nq{nq}")
            assert_knn_matches(got, tuple(w[:nq] for w in want), f"passes/{space}/nq{nq}")
    finally:
        eng.close()


# ================================================================ C. routes by k, big-k passes with many rounds
def assert_no_huge_tie_group(srt, k):
    """fallback_queries == 0 is asserted only where no tie group above 8,192 rows reaches into the top k: here no distance of
    the first k + 1 ranks repeats more than a few times."""
    head = srt[:, :k + 1]
    assert (np.diff(head, axis=1) == 0).sum(axis=1).max() < 8, "precondition: no large tie group"


@functools.lru_cache(maxsize=1)
def route_case(space):
    rows, qs = make_case(9600, 40_000, 256, 20, dup=True)
    deleted = deleted_mask(9600, 40_000, 0.05)
    srt, _ = H.assert_cuts(qs, rows, space, [63, 64, 65], deleted, "routes")
    H.assert_cuts(qs[:4], rows, space, [1023, 1024, 1025], deleted, "routes")
    assert_no_huge_tie_group(srt, 1025)
    return rows, qs, deleted


@pytest.mark.parametrize("space", SPACES)
def test_routes_by_topk(space):
    """k = 63 | 64 | 65 (filter | big-k) and 1023 | 1024 | 1025 (big-k | paged exact) on 40,000 x 256 under strategy="filter":
    strategy_used is 2 up to 1024 and 1 at 1025, scan_launches follows the route's own rule."""
    rows, qs, deleted = route_case(space)
    total, live = rows.shape[0], int((~deleted).sum())
    eng = open_engine(rows, space, "filter", deleted, pieces=2)
    try:
        for k in (63, 64, 65, 1023, 1024, 1025):
            q = qs if k <= 65 else qs[:4]
            route = H.knn_route(k, live)
            assert route == ("filter" if k <= 64 else "bigk" if k <= 1024 else "paged")
            launches = {"filter": len(H.filter_rounds(total, 5, 85, 2048)), "bigk": len(H.bigk_rounds(total, len(q), k, 400_000)),
                        "paged": -(-k // PAGE)}[route]
            want = H.oracle_knn(q, rows, k, space, deleted)
            got, st = search(eng, q, k)
            tag = f"routes/{space}/k{k}"
            assert st["strategy_used"] == H.ROUTE_STRATEGY[route] and st["scan_launches"] == launches, (tag, st, launches)
            if route != "paged":
                assert st["fallback_queries"] == 0, (tag, st)
            assert_knn_matches(got, want, tag)
    finally:
        eng.close()


@pytest.mark.parametrize("space", SPACES)
def test_bigk_needs_more_live_rows_than_k(space):
    """kRouteBigK requires live > k: 200 live rows of 300 with k = 199 (big-k pass), 200 and 201 (paged exact scan; 201 is padded,
    counts = 200)."""
    rows, qs = make_case(9700, 300, 256, 5)
    deleted = np.zeros(300, dtype=bool)
    deleted[np.random.default_rng(9700).choice(300, 100, replace=False)] = True
    H.assert_cuts(qs, rows, space, [64, 128, 192, 199], deleted, "live > k")
    eng = open_engine(rows, space, "filter", deleted)
    try:
        for k in (199, 200, 201):
            route = H.knn_route(k, 200)
            assert route == ("bigk" if k == 199 else "paged")
            want = H.oracle_knn(qs, rows, k, space, deleted)
            assert (want[2] == min(k, 200)).all()
            got, st = search(eng, qs, k)
            assert st["strategy_used"] == H.ROUTE_STRATEGY[route], (k, st)
            assert_knn_matches(got, want, f"live-k/{space}/k{k}")
    finally:
        eng.close()


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("k", [65, 300])
def test_bigk_rounds_under_bigk_budget(k, space):
    """BIGK_BUDGET=1: growth 1.5, a chain of short rounds, each with select -> mid -> prune; BIGK_BUDGET=100000000: growth capped
    at min(24, 1 + 4096 / k).  Query 0's nearest row lies in the first scan round, query 1's in the last, under either setting;
    scan_launches = the rounds of the loop in run_bigk_pass."""
    total, d, nq = 30_000, 256, 20
    rng = np.random.default_rng(9800 + k)
    rows = rng.standard_normal((total, d), dtype=np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    deleted = deleted_mask(9800, total, 0.05)
    chains = {budget: H.bigk_rounds(total, nq, k, budget) for budget in (1, 100_000_000)}
    assert H.bigk_growth(nq, k, 1) == 1.5 and H.bigk_growth(nq, k, 100_000_000) == min(24.0, 1.0 + 4096.0 / k)
    assert len(chains[1]) >= 5 and len(chains[1]) > len(chains[100_000_000]) >= 1, chains
    seed = H.bigk_seed_rows(total, nq, k)
    placements = [(0, seed + 5), (1, total - 1)]
    for rounds in chains.values():
        assert rounds[0][0] == seed and rounds[0][0] <= seed + 5 < rounds[0][1] and rounds[-1][0] <= total - 1 < rounds[-1][1]
    deleted[[r for _, r in placements]] = False
    H.plant(rows, qs, space, placements, rng)
    H.assert_rank0(qs, rows, space, placements, deleted)
    srt, _ = H.assert_cuts(qs, rows, space, [k], deleted, f"bigk budget k{k}")
    assert_no_huge_tie_group(srt, k)
    want = H.oracle_knn(qs, rows, k, space, deleted)
    eng = open_engine(rows, space, "filter", deleted, pieces=2)
    try:
        for budget, rounds in chains.items():
            eng.set_tuning(BIGK_BUDGET=budget)
            got, st = search(eng, qs, k)
            tag = f"bigk-budget/{space}/k{k}/budget{budget}"
            assert st["strategy_used"] == 2 and st["scan_launches"] == len(rounds) and st["fallback_queries"] == 0, (tag, st, rounds)
            assert_knn_matches(got, want, tag)
    finally:
        eng.close()
