"""Host-side helpers of tests/test_gpu_knn_limits.py: mirrors of the launch plans the cases sit on, the planted-row
builders and the gap assertion.  Nothing here touches a device; tests/test_knn_limits_host.py checks every helper against
the oracle (oracle.exact_scan) and against figures worked out by hand."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import exact_scan

PANEL_ROWS = 16        # layout.h: kPanelRows
FILTER_TILE = 768      # internal.h: kFilterTile
SEED_ROWS = 3840       # internal.h: kSeedRows
BIG_SEED_ROWS = 65280  # internal.h: kBigSeedRows
FILTER_QUERIES = 256   # internal.h: kFilterQueries
SMALL_NQ = 2           # internal.h: the SMALL_NQ tuning default
MAX_TOPK = 64          # include/mlvdb_hip.h: MLVDB_MAX_TOPK
BIGK_MAX = 1024        # internal.h: kBigKMax
MIN_GAP = 1e-9         # relative distance between two fp64 distances a case's cut depends on

ExactPlan = namedtuple("ExactPlan", "qt nw pw nqtiles nblk lds_bytes")


def layout_ld(d: int) -> int:
    return (d + 15) & ~15


def plan_exact(nrows: int, ld: int, nq: int) -> ExactPlan:
    """kernels_exact.hip: plan_exact over internal.h's kExactTiles (with_exact_tile instantiates them) -- the query tile (halved while its fp64 image is above 64 KiB), the waves
    per block and panels per wave of that tile, the blocks per query tile and the dynamic LDS of the launch."""
    qt = 8 if nq >= 8 else 4 if nq >= 4 else 2 if nq >= 2 else 1
    while qt > 1 and qt * ld * 8 > 64 * 1024:
        qt >>= 1
    nw = 16 if qt <= 2 else 8
    pw = 4 if qt == 4 else 2
    nqtiles = -(-nq // qt)
    ntasks = -(-(-(-nrows // PANEL_ROWS)) // pw)
    cap = max(8, min(256, 1024 // nqtiles))
    nblk = max(1, min(cap, -(-ntasks // nw)))
    return ExactPlan(qt, nw, pw, nqtiles, nblk, max(qt * ld * 8, nw * qt * 64 * 12))


def exact_owner(row: int, plan: ExactPlan):
    """(block, wave) of the exact scan that scores `row`: task = panel // PW, tasks are dealt wave by wave, block by block."""
    task = row // PANEL_ROWS // plan.pw
    slot = task % (plan.nblk * plan.nw)
    return slot // plan.nw, slot % plan.nw


def filter_rounds(total: int, seed_units: int, round1: int, round2: int, prefix_seed: bool = False):
    """api.hip: run_filter_pass -- the non-empty scan rounds [b, e) of a k <= 64 pass over `total` rows under SEED_ROWS /
    ROUND1 / ROUND2 (units of 768 rows).  prefix_seed: the pass seeds from the exact k-th best of the prefix (1-2 queries
    on the int8 shadow) and its first round starts at row 0.  One scan launch per round; the dense seed is not counted."""
    seed_rows = min(SEED_ROWS, max(1, seed_units) * FILTER_TILE)
    r1 = max(6, round1)
    r2 = max(r1, round2)
    bounds = [0 if prefix_seed else seed_rows, FILTER_TILE * r1, FILTER_TILE * r2, total]
    rounds = []
    for r in range(3):
        b, e = min(bounds[r], total), min(bounds[r + 1], total)
        if e > b:
            rounds.append((b, e))
    return rounds


def filter_call_rounds(total: int, nq: int, seed_units: int, round1: int, round2: int, int8: bool):
    """The rounds of every 256-query pass of a k <= 64 call.  A pass of at most SMALL_NQ = 2 queries on the int8 shadow (no row
    mask) takes the exact prefix seed, so its first round starts at row 0 -- the one-query last pass of a 257-query call too."""
    sizes = [min(FILTER_QUERIES, nq - q0) for q0 in range(0, nq, FILTER_QUERIES)]
    return [filter_rounds(total, seed_units, round1, round2, prefix_seed=int8 and n <= SMALL_NQ) for n in sizes]


def bigk_seed_rows(total: int, nq: int, k: int) -> int:
    want = min(BIG_SEED_ROWS, max(SEED_ROWS, -(-(66 * k * max(nq, 16) // 256) // FILTER_TILE) * FILTER_TILE))
    return want if total > want else (total + 127) // 128 * 128


def bigk_growth(nq: int, k: int, budget: int) -> float:
    return min(min(24.0, 1.0 + 4096.0 / k), max(1.5, 1.0 + max(1, budget) / (float(max(nq, 16)) * k)))


def bigk_rounds(total: int, nq: int, k: int, budget: int):
    """api.hip: run_bigk_pass -- the scan rounds [b, e) after the dense seed of one pass of nq <= 256 queries."""
    growth = bigk_growth(nq, k, budget)
    b = min(bigk_seed_rows(total, nq, k), total)
    rounds = []
    while b < total:
        e = int(b * growth) // FILTER_TILE * FILTER_TILE
        if e <= b:
            e = b + FILTER_TILE
        if e > total or e * 1.25 > total:
            e = total
        rounds.append((b, e))
        b = e
    return rounds


def knn_route(k: int, live: int, filter_path: bool = True) -> str:
    """api.hip: search_device_impl -- the route of a call by top_k (filter_path: the filter serves this index)."""
    if k > MAX_TOPK:
        return "bigk" if k <= BIGK_MAX and filter_path and live > k else "paged"
    return "filter" if filter_path else "exact"


ROUTE_STRATEGY = {"bigk": 2, "filter": 2, "paged": 1, "exact": 1}  # mlvdb_stats.strategy_used of each route


# ------------------------------------------------------------------------------------------------ the oracle, in query slabs
def live_mask(n: int, deleted) -> np.ndarray:
    live = np.ones(n, dtype=bool)
    if deleted is not None:
        live &= ~np.asarray(deleted, dtype=bool)
    return live


def oracle_knn(qs, rows, k, space, deleted=None, slab: int = 64):
    """oracle.exact_scan.knn in slabs of `slab` queries, so that the fp64 temporaries of wide rows stay small."""
    parts = [exact_scan.knn(qs[s:s + slab], rows, k, space, deleted=deleted) for s in range(0, len(qs), slab)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def oracle_topk_dense(qs, rows, k, space, slab: int = 65536):
    """The oracle's answer for MANY queries on a few live rows: exact_distances per slab and a stable sort along the rows --
    equal distances keep their label order, which is the ranking of exact_scan.knn.  -> (labels, dist32, sorted fp64)."""
    labs, d32, d64 = [], [], []
    for s in range(0, len(qs), slab):
        d = exact_scan.exact_distances(qs[s:s + slab], rows, space)
        order = np.argsort(d, axis=1, kind="stable")
        srt = np.take_along_axis(d, order, axis=1)
        labs.append(order[:, :k].astype(np.int64))
        d32.append(srt[:, :k].astype(np.float32))
        d64.append(srt[:, :k + 1])
    return np.concatenate(labs), np.concatenate(d32), np.concatenate(d64)


# ------------------------------------------------------------------------------------------------ the gap assertion
def gap_ok(a, b) -> np.ndarray:
    """Two fp64 distances a case's cut depends on: bit-equal (an intended tie, the label decides) or more than MIN_GAP relative
    apart (no arithmetic order can swap them)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.abs(a - b) > MIN_GAP * np.maximum(np.abs(a), np.abs(b)))


def sorted_live_distances(qs, rows, space, deleted=None):
    """(fp64 distances of every query to the live rows, ranked by (distance, label); the labels in that order)."""
    labels = np.nonzero(live_mask(len(rows), deleted))[0]
    d = exact_scan.exact_distances(qs, rows[labels], space)
    order = np.argsort(d, axis=1, kind="stable")  # (labels ascend, the sort is stable: ties by label)
    return np.take_along_axis(d, order, axis=1), labels[order]


def assert_cuts(qs, rows, space, cuts, deleted=None, tag: str = ""):
    """At every cut c (the rank c - 1 | c boundary: top_k = c, or a page edge) of every query the two fp64 distances are
    bit-equal or more than MIN_GAP apart.  -> the ranked distances and labels, for further preconditions."""
    srt, lab = sorted_live_distances(qs, rows, space, deleted)
    for c in cuts:
        if 0 < c < srt.shape[1]:
            ok = gap_ok(srt[:, c - 1], srt[:, c])
            assert ok.all(), (f"precondition {tag}: accidental near-tie across rank {c} for queries {np.nonzero(~ok)[0][:5]}: "
                              f"{srt[~ok][:, c - 1:c + 1][:3]} -- choose another seed")
    return srt, lab


# ------------------------------------------------------------------------------------------------ planted rows
def near_copy(q, space: str, rng, eps: float = 0.01):
    """A row that is the nearest of query q by a wide margin: q plus a little noise.  ip (d = 1 - <q, x>): <q, q> ~ d beats a
    random row's inner product (~ 4 sqrt(d) at most) from d = 64 on; narrower rows are made three times as long.  (Not the
    wide ones: ip rows share an int8 scale per group of 8, a row three times as long as its neighbours triples their
    quantisation error, and an index whose worst error passes 0.03 is taken off the filter -- i8_bounds_usable.)"""
    q = np.asarray(q, dtype=np.float32)
    scale = np.float32(np.sqrt((q.astype(np.float64) ** 2).mean()))
    row = q + np.float32(eps) * scale * rng.standard_normal(q.shape[0]).astype(np.float32)
    return (np.float32(3.0) * row if space == "ip" and q.shape[0] < 64 else row).astype(np.float32)


def plant(rows, qs, space, placements, rng, eps: float = 0.01):
    """placements: (query, row) pairs -- rows[row] becomes a near copy of qs[query].  In place."""
    for q, r in placements:
        rows[r] = near_copy(qs[q], space, rng, eps)


def plant_pair(rows, qs, space, q, r_a, r_b, rng, eps: float = 0.02):
    """Two bit-identical near copies of qs[q] at rows r_a < r_b: an exact tie that the label decides."""
    rows[r_a] = near_copy(qs[q], space, rng, eps)
    rows[r_b] = rows[r_a]


def plant_tie_group(rows, qs, space, q, first_rank, size, deleted=None):
    """Make the live rows at ranks first_rank .. first_rank + size - 1 of query q (0-based) bit-identical: the rows ranked
    first_rank + 1 .. are overwritten with the row at first_rank.  Their old distances were no smaller, so the group sits at
    exactly those ranks.  In place; -> the labels of the group, ascending."""
    _, lab = sorted_live_distances(qs[q:q + 1], rows, space, deleted)
    group = lab[0, first_rank:first_rank + size]
    assert group.size == size, "precondition: not enough live rows for the tie group"
    rows[group[1:]] = rows[group[0]]
    return np.sort(group)


def assert_rank0(qs, rows, space, placements, deleted=None):
    """The oracle confirms every planted row as its query's nearest live row, by more than MIN_GAP or by an exact tie."""
    want = exact_scan.knn(qs, rows, 1, space, deleted=deleted)[0][:, 0]
    for q, r in placements:
        assert want[q] == r, f"precondition: the oracle's nearest row of query {q} is {want[q]}, not the planted {r}"
