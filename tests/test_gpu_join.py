"""Similarity join on the MI355X (include/mlvdb_join.h) through the C ABI and ``HipScanEngine.join_within``.

The reference is the NumPy model of tests/join_helpers.py (oracle.exact_scan.range_query over the left rows, stripped by the
rule); every case asserts its preconditions on the oracle alone before the first GPU call.  One corpus of 12,000 rows per
width -- the size at which the range limits run both strategies -- holds everything planted:

* groups of identical rows (2, 3, 5, 300 and 364 of them) whose 64 non-zero components are +-1: their squared norm is 64 and
  every product is +-1, so each distance among them is exact in fp64 in any summation order (l2 0, ip -63, cosine 0) and the
  kernels and the oracle agree on them to the last bit;
* rows perturbed by one part in 1e3, component by component;
* pairs at the edges of a wave of 256 left rows and of the scan tiles (128, 192 and 256 rows) a LATER wave starts in.
"""
import functools

import numpy as np
import pytest

from mlvectordb_amd import _native, where as W
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.helpers import deleted_mask
from tests.join_helpers import (LATER, OTHERS, assert_clear_of_radius, assert_join_matches, assert_ties, cut, join_model,
                                native_join, offsets_of, strip)

pytestmark = pytest.mark.gpu

N = 12_000
ERR_INVALID, ERR_UNSUPPORTED = 1, 6  # include/mlvdb_hip.h: MLVDB_ERR_INVALID_ARG, MLVDB_ERR_UNSUPPORTED
STRATEGY_CODE = {"exact": 1, "filter": 2}
RADIUS = {"l2": 0.01, "cosine": 1e-4, "ip": -40.0}  # far from every unplanted distance (asserted per case)
MODES = [OTHERS, LATER]
GROUPS = [[2000, 7000], [2100, 2101, 9000], [1100, 1101, 3000, 5000, 11000],
          [1254, 1255],   # a the last row of the first wave of left(257) / left(513), b the first of the next
          [1010, 1020],   # both in one wave
          [1200, 1300],   # b = 1200 below the second wave's first label 1255, inside its 128-, 192- and 256-row scan tiles
          [0, N - 1],     # a row 0, b the last row of the index
          list(range(6000, 6300)), list(range(8000, 8364))]
PERTURBED = [(1400 + j, 4000 + 37 * j) for j in range(12)]
SPACES = ["l2", "cosine", "ip"]
ALL = pytest.mark.parametrize("strategy", ["exact", "filter"])


def left_set(m: int) -> np.ndarray:
    """m left rows: row 0, then 1000, 1001, ... -- waves {0, 1000..1254}, {1255..1510}, {1511}."""
    return np.concatenate([[0], np.arange(1000, 1000 + m - 1)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def corpus(d: int):
    rng = np.random.default_rng(4242 + d)
    rows = rng.standard_normal((N, d), dtype=np.float32)
    for g in GROUPS:
        p = np.zeros(d, np.float32)
        p[rng.permutation(d)[:64]] = rng.choice(np.array([-1.0, 1.0], np.float32), 64)
        rows[g] = p
    for a, b in PERTURBED:
        rows[a] *= np.float32(np.sqrt(d) / np.linalg.norm(rows[a].astype(np.float64)))  # (|x|^2 = d: inside the ip radius)
        rows[b] = rows[a] * (1 + np.float32(1e-3) * rng.standard_normal(d, dtype=np.float32))
    rows.setflags(write=False)
    deleted = deleted_mask(4242, N, 0.1)
    deleted[[x for g in GROUPS for x in g] + [x for p in PERTURBED for x in p]] = False
    deleted[[9000, 1101]] = True  # a tombstoned partner; a tombstoned left row of left_set(m >= 103)
    deleted.setflags(write=False)
    return rows, deleted


@functools.lru_cache(maxsize=None)
def checked(d: int, space: str):
    """The corpus with its preconditions asserted once per (width, space)."""
    rows, deleted = corpus(d)
    assert_ties(rows, GROUPS, space)
    assert_clear_of_radius(rows, left_set(513), RADIUS[space], space)
    return rows, deleted


@functools.lru_cache(maxsize=None)
def model(d: int, space: str, m: int, mode: int, dead: bool, radius=None):
    rows, deleted = checked(d, space)
    return join_model(rows, left_set(m), RADIUS[space] if radius is None else radius, space, mode,
                      deleted=deleted if dead else None)


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


# ---------------------------------------------------------------- 1. wave and tile edges against the NumPy model
@ALL
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("d", [64, 100])
def test_wave_and_tile_edges_against_the_numpy_model(d, space, strategy):
    """Left sets of 1, 255, 256, 257 and 513 rows in both modes: labels, counts, offsets, and float32 distances equal to the
    oracle's float64 rounded once."""
    rows, _ = checked(d, space)
    want513, _ = model(d, space, 513, LATER, False)
    at = {int(a): i for i, a in enumerate(left_set(513))}
    assert 1255 in want513[at[1254]][0] and 1020 in want513[at[1010]][0] and N - 1 in want513[at[0]][0], "precondition"
    assert 1300 in want513[at[1200]][0] and 1200 not in want513[at[1300]][0], "precondition: the pair below the wave's first label"
    assert 1200 in model(d, space, 513, OTHERS, False)[0][at[1300]][0], "precondition"
    eng = open_engine(rows, space, strategy)
    try:
        for m in (1, 255, 256, 257, 513):
            for mode in MODES:
                want, counts = model(d, space, m, mode, False)
                got, got_counts = eng.join_within(left_set(m), mode, RADIUS[space], 64)
                assert_join_matches(got, got_counts, want, counts, f"edges/{space}/{strategy}/d{d}/m{m}/mode{mode}")
        assert eng.last_stats()["strategy_used"] == STRATEGY_CODE[strategy]
    finally:
        eng.close()


# ---------------------------------------------------------------- 2. the definition itself, bit for bit
@ALL
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("d", [64, 100])
def test_the_join_is_the_range_search_of_the_stored_rows_stripped(d, space, strategy):
    """For both modes, with and without a program: ``join_within(labels)`` equals ``range(get_rows_at(labels), radius,
    where=program)`` stripped on the host -- labels, the bits of the distances, counts and offsets."""
    rows, deleted = checked(d, space)
    program = W.compile_where({"g": {"$ne": 0}}, {"g": "int"}, {})
    left = left_set(513)
    eng = open_engine(rows, space, strategy, deleted)
    try:
        eng.define_attr(0, "int64")
        eng.set_attr(0, 0, (np.arange(N) % 3).astype(np.int64))
        for where in (None, program):
            ref = eng.range(eng.get_rows_at(left), RADIUS[space], _native.MAX_TOPK_PAGED, where=where)
            for mode in MODES:
                want = [strip(l, dd, int(a), mode) for (l, dd), a in zip(ref, left)]
                counts = np.array([len(l) for l, _ in want], np.int64)
                got, got_counts = eng.join_within(left, mode, RADIUS[space], 1024, where=where)
                tag = f"definition/{space}/{strategy}/d{d}/mode{mode}/{'where' if where else 'plain'}"
                assert_join_matches(got, got_counts, want, counts, tag)
                for (gl, gd), (wl, wd) in zip(got, want):
                    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), f"{tag}: the bits of a distance differ"
    finally:
        eng.close()


# ---------------------------------------------------------------- 3. radius edges
@ALL
@pytest.mark.parametrize("space", SPACES)
def test_radius_edges(space, strategy):
    """The identical rows' distance is exact (l2 0, cosine 0, ip -63): at that radius they are in and nothing else is; a row
    that differs from them in one component by 1 sits exactly on an l2 / ip radius and is in, one float32 step below it is
    out.  Cosine: the radius is what the oracle computes for the identical rows."""
    d = 64
    rows = corpus(d)[0].copy()
    near = rows[2000].copy()
    k = int(np.flatnonzero(near)[0])
    near[k] += np.float32(1.0) if near[k] > 0 else np.float32(-1.0)  # |component| 1 -> 2: l2 distance 1, ip 1 - 65
    rows[2500] = near
    left = np.array([2000, 2100, 2500, 7000], np.int64)
    same = float(exact_scan.exact_distances(rows[2000:2001], rows[[7000]], space)[0, 0])
    assert same == {"l2": 0.0, "cosine": 0.0, "ip": -63.0}[space] and float(np.float32(same)) == same, "precondition"
    cases = [(same, True)]
    if space != "cosine":
        on = float(exact_scan.exact_distances(rows[2000:2001], rows[[2500]], space)[0, 0])
        assert on == {"l2": 1.0, "ip": -64.0}[space], "precondition: the planted row sits exactly on the radius"
        cases += [(on, True), (float(np.nextafter(np.float32(on), np.float32(-np.inf))), False)]
    eng = open_engine(rows, space, strategy)
    try:
        for radius, on_radius in cases:
            assert_clear_of_radius(rows, left, radius, space, on_radius=on_radius)
            for mode in MODES:
                want, counts = join_model(rows, left, radius, space, mode)
                got, got_counts = eng.join_within(left, mode, radius, 64)
                assert_join_matches(got, got_counts, want, counts, f"radius/{space}/{strategy}/{radius!r}/mode{mode}")
            # (mode LATER, the last of the loop) at the identical rows' own distance: they and nothing else
            if radius == same and space != "ip":
                assert got[0][0].tolist() == [7000] and got[1][0].tolist() == [2101, 9000] and counts.tolist() == [1, 2, 0, 0]
            if space == "l2" and radius != same:  # the row on the radius: in, and out one step below
                assert got[0][0].tolist() == ([7000, 2500] if on_radius else [7000]) and counts[0] == (2 if on_radius else 1)
    finally:
        eng.close()


# ---------------------------------------------------------------- 4. liveness and filters
@ALL
@pytest.mark.parametrize("space", SPACES)
def test_tombstones_and_filters(space, strategy):
    """10 % tombstones with a tombstoned partner (9000) and a tombstoned left row (1101: a valid query, never a partner) in
    both modes; a program the left rows do not all match; a program matching nothing; no left row; an empty index."""
    d = 100
    rows, deleted = checked(d, space)
    left = left_set(513)
    at = {int(a): i for i, a in enumerate(left)}
    g = (np.arange(N) % 3).astype(np.int64)
    some = W.compile_where({"g": 1}, {"g": "int"}, {})
    none = W.compile_where({"g": 7}, {"g": "int"}, {})
    eng = open_engine(rows, space, strategy, deleted)
    try:
        eng.define_attr(0, "int64")
        eng.set_attr(0, 0, g)
        for mode in MODES:
            want, counts = model(d, space, 513, mode, True)
            assert 1100 not in want[at[1101]][0] or mode == OTHERS, "precondition"
            assert want[at[1101]][0].size > 0, "precondition: the tombstoned left row has partners"
            assert all(1101 not in l and 9000 not in l for l, _ in want), "precondition: a tombstoned row is no partner"
            got, got_counts = eng.join_within(left, mode, RADIUS[space], 64)
            assert_join_matches(got, got_counts, want, counts, f"tombstones/{space}/{strategy}/mode{mode}")
        want, counts = join_model(rows, left, RADIUS[space], space, OTHERS, deleted=deleted, matching=g == 1)
        assert counts.sum() > 0 and (g[left] != 1).any() and counts[g[left] != 1].sum() > 0, "precondition"
        got, got_counts = eng.join_within(left, OTHERS, RADIUS[space], 64, where=some)
        assert_join_matches(got, got_counts, want, counts, f"where/{space}/{strategy}")
        got, got_counts = eng.join_within(left, LATER, RADIUS[space], 64, where=none)
        assert got_counts.tolist() == [0] * 513 and got.offsets.tolist() == [0] * 514
        rc, hits, cnt, off, _, _ = native_join(eng, np.zeros(0, np.int64), LATER, RADIUS[space], 8, 16)
        assert rc == _native.OK and off.tolist() == [0]
        got, got_counts = eng.join_within(np.zeros(0, np.int64), OTHERS, RADIUS[space], 8)
        assert len(got) == 0 and got_counts.size == 0
    finally:
        eng.close()
    empty = HipScanEngine(d, space, device=0, strategy=strategy)
    try:
        rc, _, _, off, _, _ = native_join(empty, np.zeros(0, np.int64), LATER, RADIUS[space], 8, 16)
        assert rc == _native.OK and off.tolist() == [0]
        rc, _, cnt, off, lab, _ = native_join(empty, np.array([0], np.int64), LATER, RADIUS[space], 8, 16)
        assert rc == ERR_INVALID and off.tolist() == [-1, -1] and cnt.tolist() == [-1] and lab[0] == -9  # no row 0 to name
    finally:
        empty.close()


# ---------------------------------------------------------------- 5. capacity, the statuses, the truncated inner list
@ALL
@pytest.mark.parametrize("space", SPACES)
def test_capacity_and_statuses(space, strategy):
    """The 300 identical rows 6000..6299: capacities 1, 255, 256, 257 and 299 return the nearest partners in (distance,
    label) order with exact counts and MLVDB_ERR_OVERFLOW; a counting call; a short total_capacity; a capacity above
    MLVDB_JOIN_MAX_CAPACITY.  The 364 identical rows 8000..8363 at capacity 64: the inner list (capacity + 256 entries) is
    truncated for every left row, the counts must be exact all the same."""
    d = 64
    rows, _ = checked(d, space)
    left = np.arange(5990, 6310, dtype=np.int64)  # 320 left rows: the group spans the two waves
    big = np.arange(8000, 8100, dtype=np.int64)   # one wave inside the group of 364
    eng = open_engine(rows, space, strategy)
    try:
        for mode in MODES:
            want, counts = join_model(rows, left, RADIUS[space], space, mode)
            assert counts.max() == 299 and (counts[10:310] == (299 if mode == OTHERS else np.arange(299, -1, -1))).all(), "precondition"
            for capacity in (1, 255, 256, 257, 299):
                tag = f"capacity/{space}/{strategy}/mode{mode}/cap{capacity}"
                total = int(np.minimum(counts, capacity).sum())
                rc, hits, cnt, off, _, _ = native_join(eng, left, mode, RADIUS[space], capacity, total)
                assert rc == (_native.ERR_OVERFLOW if capacity < 299 else _native.OK), tag
                assert np.array_equal(off, offsets_of(cut(want, capacity))), f"{tag}: offsets"
                assert_join_matches(hits, cnt, cut(want, capacity), counts, tag)
                got, got_counts = eng.join_within(left, mode, RADIUS[space], capacity, truncate=True)
                assert_join_matches(got, got_counts, cut(want, capacity), counts, tag + "/engine")
            got, got_counts = eng.join_within(left, mode, RADIUS[space], 8)  # the resizing wrapper: every partner
            assert_join_matches(got, got_counts, want, counts, f"capacity/{space}/{strategy}/mode{mode}/grown")
            # a counting call: counts and layout, NULL hit arrays
            rc, _, cnt, off, _, _ = native_join(eng, left, mode, RADIUS[space], 256, 0)
            assert rc == _native.ERR_OVERFLOW and np.array_equal(cnt, counts) and np.array_equal(off, offsets_of(cut(want, 256)))
            # a short total_capacity: offsets and counts written, the hit arrays untouched
            short = int(np.minimum(counts, 256).sum()) - 1
            rc, _, cnt, off, lab, dist = native_join(eng, left, mode, RADIUS[space], 256, short)
            assert rc == _native.ERR_OVERFLOW and np.array_equal(cnt, counts) and np.array_equal(off, offsets_of(cut(want, 256)))
            assert (lab == -9).all() and (dist == -9.0).all(), "a call that does not fit writes no hit"
            # one above the largest capacity: refused, nothing written
            rc, _, cnt, off, lab, _ = native_join(eng, left, mode, RADIUS[space], _native.JOIN_MAX_CAPACITY + 1, 64)
            assert rc == ERR_UNSUPPORTED and (cnt == -1).all() and (off == -1).all() and (lab == -9).all()
            # the truncated inner list
            want, counts = join_model(rows, big, RADIUS[space], space, mode)
            assert (counts == (363 if mode == OTHERS else 363 - np.arange(100))).all(), "precondition"
            got, got_counts = eng.join_within(big, mode, RADIUS[space], 64, truncate=True)
            assert_join_matches(got, got_counts, cut(want, 64), counts, f"truncated/{space}/{strategy}/mode{mode}")
        for bad_left in ([5, 5], [6, 5], [-1], [N]):
            rc, _, cnt, off, _, _ = native_join(eng, np.array(bad_left, np.int64), OTHERS, RADIUS[space], 8, 16)
            assert rc == ERR_INVALID and (off == -1).all(), bad_left
        assert native_join(eng, left, 2, RADIUS[space], 8, 16)[0] == ERR_INVALID       # an unknown mode
        assert native_join(eng, left, OTHERS, RADIUS[space], 0, 16)[0] == ERR_INVALID  # capacity < 1
        assert eng._lib.mlvdb_join_within(eng.handle, left.ctypes.data, left.size, OTHERS, 0.5, 8, -1, None, None, None,
                                          left.ctypes.data, left.ctypes.data) == ERR_INVALID
    finally:
        eng.close()


# ---------------------------------------------------------------- 6. mutations on one handle
@ALL
@pytest.mark.parametrize("space", SPACES)
def test_the_join_follows_appends_tombstones_compact_and_reset(space, strategy):
    """One handle through an append, a tombstone, ``compact`` and ``reset``: the lazily built shadows (int8, fp16 mid) and
    the masked copies are re-made, every answer is the model's for the rows as they stand."""
    d = 64
    rows, deleted = checked(d, space)
    rows = np.array(rows)
    eng = HipScanEngine(d, space, device=0, strategy=strategy)
    try:
        def check(stage, have, dead, left):
            for mode in MODES:
                want, counts = join_model(have, left, RADIUS[space], space, mode, deleted=dead)
                got, got_counts = eng.join_within(left, mode, RADIUS[space], 64)
                assert_join_matches(got, got_counts, want, counts, f"mutations/{space}/{strategy}/{stage}/mode{mode}")
            return counts

        eng.append(rows[:8000])
        left = np.concatenate([[0], np.arange(5900, 6200)]).astype(np.int64)
        before = check("first rows", rows[:8000], None, left)
        eng.append(rows[8000:])
        after = check("appended", rows, None, left)
        assert after[0] == before[0] + 1, "precondition: the append brought row 0 its partner, the last row"
        assert eng.tombstone(np.nonzero(deleted)[0]) == int(deleted.sum()) and eng.tombstone(np.array([6001])) == 1
        dead = deleted.copy()
        dead[6001] = True
        check("tombstoned", rows, dead, left)
        old = eng.compact()
        assert np.array_equal(old, np.nonzero(~dead)[0])
        packed = rows[old]
        first = int(np.searchsorted(old, 5900))
        check("compacted", packed, None, np.concatenate([[0], np.arange(first, first + 300)]).astype(np.int64))
        eng.reset()
        eng.append(rows[5000:9000])
        check("reset", rows[5000:9000], None, np.arange(900, 1300, dtype=np.int64))
        assert eng.last_stats()["strategy_used"] in (STRATEGY_CODE[strategy], STRATEGY_CODE["exact"])
    finally:
        eng.close()
