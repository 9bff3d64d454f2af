"""Geo attributes on the MI355X (include/mlvdb_geo.h) against the NumPy oracle of tests/geo_helpers.py: the two predicate ops
through every consumer of a program, nearest by distance, the life cycle of the stored points.  Box results, labels, point
bits, matched and absent are compared exactly; radius membership and rank order are exact too, because the helper asserts on
the CPU -- before any device call -- that no input lies within G = 1e-10 of a decision (its guards); distances are compared
with the long double oracle under 16 x the deviation of a plain NumPy fp64 evaluation over the test's own inputs, and a
distance of zero must be exactly 0.0.  Rows are 4 floats wide and every call is made twice and must agree.

Largest relative deviation of the device's distances from the long double oracle seen in this file: see DESIGN.md 11.15."""
import functools
import json
import math

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests import geo_helpers as GH
from tests.facet_helpers import GRID_ROWS

pytestmark = pytest.mark.gpu

WINDOWS = ((0, 1), (0, 20), (4076, 20), (0, 4096))
VIENNA = (48.2082, 16.3738)
SEEN = {"device_deviation": 0.0}  # the largest relative deviation of a returned distance from the oracle, printed per test


def _pt(lat, lon):
    return int(GH.quantise([lat], [lon])[0])


def _engine(col, tomb=None, extra=None):
    """An index of len(col) rows of 4 floats with the geo column 0 (and the int64 / float64 columns of `extra`)."""
    n = col.size
    eng = HipScanEngine(4, "l2", device=0)
    if n:
        eng.append(np.ones((n, 4), dtype=np.float32))
    eng.define_attr(0, "geo")
    for a, c in (extra or {}).items():
        eng.define_attr(a, c.dtype.name)
    if n:
        eng.set_attr(0, 0, col)
        for a, c in (extra or {}).items():
            eng.set_attr(a, 0, c)
    if tomb is not None and tomb.any():
        eng.tombstone(np.flatnonzero(tomb))
    return eng


def _check_filter(eng, program, want_mask, tag):
    """where_count and where_labels, twice each, against the oracle's mask (live rows only)."""
    want = np.flatnonzero(want_mask)
    for _ in range(2):
        assert eng.where_count(program) == want.size, f"{tag}: where_count"
        got = eng.where_labels(program)
        assert np.array_equal(got, want), f"{tag}: where_labels differ ({got.size} rows, oracle {want.size})"


def _check_nearest(eng, col, mask, centre, tol, program=None, windows=WINDOWS, tag="nearest", h=None):
    """geo_nearest twice per window against the oracle's ranking of the rows of `mask` (live and matching)."""
    top, d, matched, absent = GH.nearest_oracle(col, mask, centre, h)
    out = {}
    for offset, limit in windows:
        want, want_d = top[offset:offset + limit], d[offset:offset + limit]
        name = f"{tag}_{offset}_{limit}"
        got = eng.geo_nearest(0, centre, limit, where=program, offset=offset)
        again = eng.geo_nearest(0, centre, limit, where=program, offset=offset)
        assert got[3:] == (matched, absent), f"{name}: (matched, absent) {got[3:]}, oracle {(matched, absent)}"
        assert got[0].size == want.size == max(0, min(matched - absent - offset, limit)), f"{name}: n_out {got[0].size}"
        assert np.array_equal(got[0], want), f"{name}: labels differ at ranks {np.flatnonzero(got[0] != want)[:8]}"
        assert np.array_equal(got[1], col[want]), f"{name}: point bits differ"
        assert got[2].dtype == np.float64 and np.array_equal(got[2] == 0.0, want_d == 0), f"{name}: zero distances"
        nz = want_d > 0
        if nz.any():
            dev = float(np.max(np.abs(got[2][nz].astype(GH.LD) - want_d[nz]) / want_d[nz]))
            SEEN["device_deviation"] = max(SEEN["device_deviation"], dev)
            print(f"{name}: device deviation {dev:.3e}, tolerance {tol:.3e}")
            assert dev <= tol, f"{name}: distance deviates by {dev:.3e} relative, tolerance {tol:.3e}"
        assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(got[:3], again[:3])) and \
            got[3:] == again[3:], f"{name}: two calls disagree"
        out[(offset, limit)] = got
    return out


def _tolerance(points, centres):
    dev = GH.fp64_deviation(points, centres)
    print(f"NumPy fp64 deviation from long double over {np.count_nonzero(points != GH.ABSENT)} points x {len(centres)} "
          f"centres: {dev:.3e} (tolerance 16 x: {16 * dev:.3e}); largest device deviation so far {SEEN['device_deviation']:.3e}")
    return 16 * dev


# ---------------------------------------------------------------- row counts
@functools.lru_cache(maxsize=None)
def _pool():
    """The points, tombstones, tolerance and long double hav of test_row_counts: every case takes a prefix (computed once)."""
    rng = np.random.default_rng(20261020)
    n = GRID_ROWS + 300
    col = GH.random_points(rng, n, VIENNA)
    tomb = rng.random(n) < 0.1
    return col, tomb, _tolerance(col, [_pt(*VIENNA)]), GH.hav(col, _pt(*VIENNA))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 40_000, GRID_ROWS + 300])
def test_row_counts(n):
    col, tomb, tol, h = _pool()
    col, tomb, h = col[:n].copy(), tomb[:n], h[:n]
    centre = _pt(*VIENNA)
    sw, ne = _pt(VIENNA[0] - 0.15, VIENNA[1] - 0.3), _pt(VIENNA[0] + 0.2, VIENNA[1] + 0.25)
    inside = GH.radius_mask(col, centre, 25_000.0, h)
    cases = {"radius": (GH.radius_program(0, centre, 25_000.0), inside),
             "box": (GH.box_program(0, sw, ne), GH.box_mask(col, sw, ne)),
             "not_radius": (GH.negate(GH.radius_program(0, centre, 25_000.0)), ~inside)}
    eng = _engine(col, tomb)
    try:
        got = _check_nearest(eng, col, ~tomb, centre, tol, tag=f"rows_{n}_all", h=h)
        if n == 0:
            assert all(g[0].size == 0 and g[3:] == (0, 0) for g in got.values())
        for name, (program, mask) in cases.items():
            _check_filter(eng, program, mask & ~tomb, f"rows_{n}_{name}")
            _check_nearest(eng, col, mask & ~tomb, centre, tol, program=program, tag=f"rows_{n}_{name}", h=h)
    finally:
        eng.close()


# ---------------------------------------------------------------- geometry at the edges
def test_a_centre_next_to_the_antimeridian():
    rng = np.random.default_rng(5)
    n = 3000
    lat = rng.uniform(-0.01, 0.01, n)
    lon = (179.9999 + rng.uniform(-0.02, 0.02, n) + 180) % 360 - 180  # on both sides of +-180
    col = GH.quantise(lat, lon)
    col[rng.random(n) < 0.1] = GH.ABSENT
    _, lons = GH.unpack(col[col != GH.ABSENT])
    assert (lons > 0).sum() > 500 and (lons < 0).sum() > 500
    centre = _pt(0.0, 179.9999)
    tol = _tolerance(col, [centre])
    eng = _engine(col)
    try:
        for r in (50.0, 500.0, 1500.0):
            mask = GH.radius_mask(col, centre, r)
            _check_filter(eng, GH.radius_program(0, centre, r), mask, f"antimeridian_{r}")
            _check_nearest(eng, col, mask, centre, tol, GH.radius_program(0, centre, r), ((0, 20), (0, 4096)), f"antimeridian_{r}")
        _, lons = GH.unpack(col[GH.radius_mask(col, centre, 500.0)])
        assert (lons > 0).any() and (lons < 0).any()  # the circle holds points of both sides
        _check_nearest(eng, col, np.ones(n, bool), centre, tol, tag="antimeridian_all")
    finally:
        eng.close()


@pytest.mark.parametrize("pole", [90.0, -90.0])
def test_a_centre_at_a_pole(pole):
    rng = np.random.default_rng(17 if pole > 0 else 18)
    n = 600
    col = GH.random_points(rng, n, (pole * 0.99, 40.0))  # (4.5 sigma off the pole: two rows AT the pole with different
    # longitudes are one place, whose distance is cos(90 degrees) in each precision -- 6e-17 in fp64 -- and no test of rounding)
    col[:3] = GH.quantise([pole, pole * 0.9999999, -pole], [0.0, -77.0, 12.0])  # the pole itself, 1.1 cm off, the other pole
    centre = _pt(pole, 0.0)
    tol = _tolerance(col, [centre])
    eng = _engine(col)
    try:
        for r in (0.0, 1000.0, 2_000_000.0):
            mask = GH.radius_mask(col, centre, r)
            _check_filter(eng, GH.radius_program(0, centre, r), mask, f"pole_{pole}_{r}")
        assert GH.radius_mask(col, centre, 0.0).sum() == 1
        got = _check_nearest(eng, col, np.ones(n, bool), centre, tol, windows=((0, 20), (0, 4096)), tag=f"pole_{pole}")
        assert got[(0, 20)][0][:2].tolist() == [0, 1] and got[(0, 20)][2][0] == 0.0
    finally:
        eng.close()


def test_seams_zero_radius_whole_sphere_and_boxes():
    rng = np.random.default_rng(23)
    n = 2500
    col = GH.random_points(rng, n, (10.0, 179.5), sigma=0.5)
    # lon -180 and +180 at one latitude are one place; three rows at one spot and its neighbours 1e-7 degree away
    spot = (10.0, -179.2)
    col[:9] = GH.quantise([10.0, 10.0, spot[0], spot[0], spot[0], spot[0] + 1e-7, spot[0], 90.0, -90.0],
                          [-180.0, 180.0, spot[1], spot[1], spot[1], spot[1], spot[1] - 1e-7, 5.0, -5.0])
    eng = _engine(col)
    try:
        for lon in (-180.0, 180.0):
            mask = GH.radius_mask(col, _pt(10.0, lon), 1.0)
            assert mask[:2].all() and mask.sum() == 2
            _check_filter(eng, GH.radius_program(0, _pt(10.0, lon), 1.0), mask, f"seam_{lon}")
        zero = GH.radius_mask(col, _pt(*spot), 0.0)
        assert np.flatnonzero(zero).tolist() == [2, 3, 4]
        _check_filter(eng, GH.radius_program(0, _pt(*spot), 0.0), zero, "zero_radius")
        _check_filter(eng, GH.radius_program(0, _pt(*spot), 0.02), GH.radius_mask(col, _pt(*spot), 0.02), "two_centimetres")
        assert GH.radius_mask(col, _pt(*spot), 0.02).sum() == 5
        have = col != GH.ABSENT
        for r in (math.pi * GH.R, 2.5e7, 1e12):
            assert np.array_equal(GH.radius_mask(col, _pt(-33.0, 151.0), r), have)
            _check_filter(eng, GH.radius_program(0, _pt(-33.0, 151.0), r), have, f"whole_sphere_{r}")
        boxes = {"wraps": (_pt(9.0, 179.0), _pt(11.0, -179.0)), "plain": (_pt(9.0, -179.0), _pt(11.0, 179.0)),
                 "degenerate": (_pt(*spot), _pt(*spot)), "both_poles": (_pt(-90.0, 100.0), _pt(90.0, -100.0)),
                 "everything": (_pt(-90.0, -180.0), _pt(90.0, 180.0)), "seam_line": (_pt(-90.0, 180.0), _pt(90.0, -180.0))}
        for name, (sw, ne) in boxes.items():
            mask = GH.box_mask(col, sw, ne)
            _check_filter(eng, GH.box_program(0, sw, ne), mask, f"box_{name}")
            _check_filter(eng, GH.negate(GH.box_program(0, sw, ne)), ~mask, f"not_box_{name}")
        assert GH.box_mask(col, *boxes["wraps"]).sum() > 100 and GH.box_mask(col, *boxes["degenerate"]).sum() == 3
        assert GH.box_mask(col, *boxes["both_poles"])[7:9].tolist() == [False, False]
        assert GH.box_mask(col, *boxes["seam_line"])[:2].all() and np.array_equal(GH.box_mask(col, *boxes["everything"]), have)
        exists = W.Program(np.array([(W.EXISTS, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
        _check_filter(eng, exists, have, "exists")
    finally:
        eng.close()


# ---------------------------------------------------------------- ties
def test_rows_on_fifty_points_are_ranked_by_label_inside_a_tie():
    rng = np.random.default_rng(31)
    spots = GH.random_points(rng, 50, VIENNA, absent=0.0)
    assert np.unique(spots).size == 50
    # ... and 3,000 rows with points of their own between them (they also make the fp64 deviation a measurement over
    # thousands of distances, not fifty)
    col = np.concatenate([spots[rng.integers(0, 50, 5000)], GH.random_points(rng, 3000, VIENNA, absent=0.0)])
    col = col[rng.permutation(col.size)]
    col[rng.random(col.size) < 0.1] = GH.ABSENT
    tomb = rng.random(col.size) < 0.1
    centre = _pt(48.0, 16.0)
    tol = _tolerance(col, [centre])
    eng = _engine(col, tomb)
    try:
        windows = WINDOWS + ((37, 100), (99, 2), (150, 1), (4000, 96))  # groups hold about 80 rows: these begin and end inside one
        got = _check_nearest(eng, col, ~tomb, centre, tol, windows=windows, tag="fifty_points")
        labels, points = got[(0, 4096)][:2]
        same = points[1:] == points[:-1]
        assert same.sum() > 2000 and (labels[1:][same] > labels[:-1][same]).all()
        inside = GH.radius_mask(col, centre, 40_000.0)
        _check_nearest(eng, col, inside & ~tomb, centre, tol, GH.radius_program(0, centre, 40_000.0), windows, "fifty_points_where")
    finally:
        eng.close()


def test_more_rows_at_one_point_than_one_block_ranks():
    rng = np.random.default_rng(37)
    n, sydney, tokyo = 6000, _pt(-33.8688, 151.2093), _pt(35.0, 139.0)
    # 6,000 rows at one point, then 2,000 rows elsewhere (some of them nearer to the second centre than the point is; they
    # also make the fp64 deviation a measurement over thousands of distances, not one)
    col = np.concatenate([np.full(n, sydney, dtype=np.int64), GH.random_points(rng, 2000, (35.0, 139.0), absent=0.0)])
    col[[7, 4095, 4096, 5000]] = GH.ABSENT
    tomb = np.zeros(col.size, bool)
    tomb[[0, 5, 4097]] = True
    group = np.flatnonzero(~tomb[:n] & (col[:n] != GH.ABSENT))
    eng = _engine(col, tomb)
    try:
        for centre, least in ((sydney, 4096), (tokyo, 2500)):  # hav == 0 for the whole group; one hav > 0 for the whole group
            tol = _tolerance(col, [centre])
            got = _check_nearest(eng, col, ~tomb, centre, tol, tag="one_point")
            labels, points, dist = got[(0, 4096)][:3]
            at = points == sydney
            assert at.sum() >= least and labels[at].tolist() == group[:at.sum()].tolist()
            assert np.unique(dist[at]).size == 1
    finally:
        eng.close()


# ---------------------------------------------------------------- every consumer of a program
CONSUMER_SCHEMA = {"loc": "geo", "near": "int", "far": "int", "boxed": "int", "cat": "int", "price": "float"}


@functools.lru_cache(maxsize=None)
def _consumer_data():
    rng = np.random.default_rng(41)
    n = 20_000
    col = GH.random_points(rng, n, VIENNA)
    k = 60  # a handful of rows around 50 m from the centre, so that the small circle is neither empty nor everything near it
    col[:k] = GH.quantise(VIENNA[0] + rng.uniform(-6e-4, 6e-4, k), VIENNA[1] + rng.uniform(-9e-4, 9e-4, k))
    centre = _pt(*VIENNA)
    sw, ne = _pt(VIENNA[0] - 0.1, VIENNA[1] - 0.2), _pt(VIENNA[0] + 0.15, VIENNA[1] + 0.1)
    masks = {"near": GH.radius_mask(col, centre, 50.0), "far": GH.radius_mask(col, centre, 2_000_000.0),
             "boxed": GH.box_mask(col, sw, ne)}
    assert 3 <= masks["near"].sum() < k and masks["far"].sum() > n // 3 and masks["boxed"].sum() > 1000
    geo = {"near": {"loc": {"$geo_radius": {"center": VIENNA, "radius": 50}}},
           "far": {"loc": {"$geo_radius": {"center": {"lat": VIENNA[0], "lon": VIENNA[1]}, "radius": 2_000_000.0}}},
           "boxed": {"loc": {"$geo_box": {"sw": W.geo_degrees(sw), "ne": W.geo_degrees(ne)}}}}
    rows = rng.standard_normal((n, 4)).astype(np.float32)
    cat = rng.integers(0, 12, n)
    price = np.round(rng.uniform(1, 500, n), 2)
    return col, masks, geo, rows, cat, price


def _consumer_index():
    col, masks, geo, rows, cat, price = _consumer_data()
    index = Index(space="l2", attributes=CONSUMER_SCHEMA)
    lat, lon = GH.unpack(col)
    points = [None if v == GH.ABSENT else (a / 1e7, o / 1e7) for v, a, o in zip(col.tolist(), lat.tolist(), lon.tolist())]
    attrs = {"loc": points, "cat": cat, "price": price}
    attrs.update({name: m.astype(np.int64) for name, m in masks.items()})  # the oracle's masks, as columns of their own
    ids = index.add_arrays(rows, "ns", attributes=attrs)
    stored = index._ns["ns"].engine.get_attr(0, 0, col.size)
    assert np.array_equal(stored, col)  # degrees -> e7 is the identity on what the oracle saw
    return index, ids


def _same_hits(a, b, tag):
    assert np.array_equal(a.counts, b.counts), f"{tag}: counts"
    assert np.array_equal(a.labels, b.labels), f"{tag}: labels"
    assert np.array_equal(a.scores.view(np.int32), b.scores.view(np.int32)), f"{tag}: scores"


def test_every_search_consumer_agrees_with_the_host_built_mask():
    col, masks, geo, rows, cat, price = _consumer_data()
    index, _ = _consumer_index()
    try:
        q = np.random.default_rng(43).standard_normal((3, 4)).astype(np.float32)
        for name in ("near", "far", "boxed"):
            for _ in range(2):
                got = index.search_many(q, 10, "ns", "l2", where=geo[name])
                _same_hits(got, index.search_many(q, 10, "ns", "l2", where={name: 1}), f"search_many_{name}")
                assert int(got.counts[0]) == min(10, int(masks[name].sum()))
        each = [geo["near"], geo["far"], None]
        plain = [{"near": 1}, {"far": 1}, None]
        programs, of = index._compile_each("ns", each)  # the small circle is gathered, the large one scanned under its mask
        routes = index._ns["ns"].engine.search_each(q, 10, programs, of, return_routes=True)[-1]
        assert routes.tolist() == [_native.ROUTE_GATHER, _native.ROUTE_SCAN]
        for _ in range(2):
            got = index.search_many(q, 10, "ns", "l2", where=each)
            _same_hits(got, index.search_many(q, 10, "ns", "l2", where=plain), "search_many_each")
            _same_hits(got, index.search_many(q, 10, "ns", "l2", where=[{"$and": [w]} if w else None for w in each]), "each_again")
            assert got.counts.tolist() == [min(10, int(masks["near"].sum())), 10, 10]
            want = index.range_search_many(q, 1.5, "ns", "l2", where=plain)
            assert index.range_search_many(q, 1.5, "ns", "l2", where=each) == want and len(want[1]) > 10
        wheres = [geo["near"], geo["far"], geo["boxed"], {"$not": geo["far"]}, {"$and": [geo["boxed"], {"cat": {"$lt": 3}}]}]
        want = [masks["near"].sum(), masks["far"].sum(), masks["boxed"].sum(), (~masks["far"]).sum(),
                (masks["boxed"] & (cat < 3)).sum()]
        for _ in range(2):
            assert index.count_many("ns", wheres) == [int(w) for w in want]
            assert [index.count("ns", w) for w in wheres] == [int(w) for w in want]
    finally:
        index.close()


def test_facets_top_by_and_histogram_take_a_geo_filter():
    col, masks, geo, rows, cat, price = _consumer_data()
    index, _ = _consumer_index()
    try:
        for name in ("near", "far", "boxed"):
            for _ in range(2):
                got = index.facets("ns", "cat", geo[name], order="value")
                assert got == index.facets("ns", "cat", {name: 1}, order="value")
                assert got["matched"] == int(masks[name].sum()) and dict(got["values"]) == \
                    {int(v): int(c) for v, c in zip(*np.unique(cat[masks[name]], return_counts=True))}
                top = index.top_by("ns", "price", 20, geo[name], descending=True)
                assert top == index.top_by("ns", "price", 20, {name: 1}, descending=True)
                assert top["values"] == np.sort(price[masks[name]])[::-1][:20].tolist()
                hist = index.histogram("ns", "price", [100, 200.5, 400], geo[name])
                assert hist["counts"].tolist() == index.histogram("ns", "price", [100, 200.5, 400], {name: 1})["counts"].tolist()
    finally:
        index.close()


def test_update_where_then_remove_where_by_a_geo_filter():
    col, masks, geo, rows, cat, price = _consumer_data()
    index, ids = _consumer_index()
    try:
        model_cat, live = cat.copy(), np.ones(col.size, bool)
        assert index.update_where("ns", geo["boxed"], {"cat": 99}) == int(masks["boxed"].sum())
        model_cat[masks["boxed"]] = 99
        assert index.count("ns", {"cat": 99}) == int((model_cat == 99).sum())
        there = (12.5, -45.25)  # a geo value assigned by a geo filter that reads the same column
        assert index.update_where("ns", geo["near"], {"loc": there}) == int(masks["near"].sum())
        model = col.copy()
        model[masks["near"]] = _pt(*there)
        assert index.count("ns", geo["near"]) == 0
        assert index.count("ns", {"loc": {"$geo_radius": {"center": there, "radius": 0}}}) == int(masks["near"].sum())
        assert index.update_where("ns", {"near": 1}, {"loc": None}) == int(masks["near"].sum())
        model[masks["near"]] = GH.ABSENT
        assert np.array_equal(index._ns["ns"].engine.get_attr(0, 0, col.size), model)
        gone = GH.radius_mask(model, _pt(*VIENNA), 30_000.0)
        removed = index.remove_where("ns", {"loc": {"$geo_radius": {"center": VIENNA, "radius": 30_000}}}, return_ids=True)
        live &= ~gone
        assert len(removed) == int(gone.sum()) > 1000
        assert [u.bytes for u in removed] == [bytes(b) for b in ids[gone]]
        assert index.count("ns", {}) == int(live.sum())
        survivors = index.query_by_metadata("ns", {"loc": {"$exists": True}})
        assert [u.bytes for u in survivors] == [bytes(b) for b in ids[live & (model != GH.ABSENT)]]
        assert index.count("ns", geo["far"]) == int((GH.radius_mask(model, _pt(*VIENNA), 2_000_000.0) & live).sum())
        got = index.nearest("ns", "loc", VIENNA, 5)
        top, d, matched, absent = GH.nearest_oracle(model, live, _pt(*VIENNA))
        assert [u.bytes for u in got["ids"]] == [bytes(b) for b in ids[top[:5]]] and (got["matched"], got["absent"]) == (matched, absent)
        assert min(got["distances"]) > 30_000
    finally:
        index.close()


# ---------------------------------------------------------------- the native refusals (host checks: nothing is launched)
def test_native_refusals_name_the_geo_column():
    col = GH.quantise([1.0, 2.0, 3.0], [4.0, 5.0, 6.0])
    eng = _engine(col, extra={1: np.array([1, 2, 3], np.int64)})
    P = lambda *ops: W.Program(np.array(list(ops), W.OP_DTYPE), np.zeros(4, np.int64))  # noqa: E731
    bad_lat, bad_lon = (900_000_001 << 32), 1_800_000_001
    try:
        refused = [
            (lambda: eng.set_attr(0, 0, np.array([bad_lat], np.int64)), "geo value outside"),
            (lambda: eng.set_attr(0, 0, np.array([bad_lon], np.int64)), "geo value outside"),
            (lambda: eng.set_attr_at(0, np.array([1]), np.array([-bad_lat], np.int64)), "geo value outside"),
            (lambda: eng.update_where(P((W.TRUE, 0, 0, 0)), [(0, 0, bad_lon)]), "geo value outside"),
            (lambda: eng.update_where(P((W.TRUE, 0, 0, 0)), [(0, 1, 5)]), "ADD on a geo column"),
            (lambda: eng.where_count(P((W.EQ, 0, int(col[0]), 0))), "a geo column takes GEO_RADIUS, GEO_BOX and EXISTS only"),
            (lambda: eng.where_count(P((W.IN, 0, 0, 2))), "a geo column takes"),
            (lambda: eng.where_count(P((W.LEN, 0, 0, 2))), "need a list column"),
            (lambda: eng.where_count(P((W.GEO_RADIUS, 1, 0, 0))), "need a geo column"),
            (lambda: eng.where_count(P((W.GEO_BOX, 1, 0, 0))), "need a geo column"),
            (lambda: eng.where_count(P((W.GEO_BOX, 0, _pt(2.0, 0.0), _pt(1.0, 0.0)))), "south-west corner lies north"),
            (lambda: eng.where_count(P((W.GEO_BOX, 0, 0, bad_lon))), "b is not a point"),
            (lambda: eng.where_count(P((W.GEO_RADIUS, 0, bad_lat, 0))), "a is not a point"),
            (lambda: eng.where_count(P((W.GEO_RADIUS, 0, 0, W.float_bits(1.5)))), r"must be in \[0, 1\]"),
            (lambda: eng.where_count(P((W.GEO_RADIUS, 0, 0, W.float_bits(-0.5)))), r"must be in \[0, 1\]"),
            (lambda: eng.where_count(P((W.GEO_RADIUS, 0, 0, W.float_bits(float("nan"))))), r"must be in \[0, 1\]"),
            (lambda: eng.where_count(P((18, 0, 0, 0))), "unknown where op"),
            (lambda: eng.where_ordered(0, 5), "a geo column"),
            (lambda: eng.facet_values(0, 10), "a geo column"),
            (lambda: eng.facet_bins(0, np.array([1, 2], np.int64)), "geo column"),
            (lambda: eng.search_distinct(np.ones((1, 4), np.float32), 1, 0), "a geo column"),
            (lambda: eng.search_grouped(np.ones((1, 4), np.float32), 1, 2, 0), "a geo column"),
            (lambda: eng.search_maxsim(np.ones((1, 4), np.float32), np.array([0, 1], np.int64), 1, 0), "a geo column"),
            (lambda: eng.geo_nearest(1, 0, 5), "needs a geo column"),
            (lambda: eng.geo_nearest(0, bad_lon, 5), "center is not a point"),
            (lambda: eng.geo_nearest(0, 0, 0), "offset >= 0, limit >= 1"),
            (lambda: eng.geo_nearest(0, 0, 4096, offset=1), "offset >= 0, limit >= 1"),
        ]
        for call, needle in refused:
            with pytest.raises(RuntimeError, match=needle):
                call()
        assert np.array_equal(eng.get_attr(0, 0, 3), col)  # nothing was written
        assert eng.update_where(P((W.TRUE, 0, 0, 0)), [(0, 0, GH.ABSENT)]) == (3, 0)  # ASSIGN of absent clears
        assert eng.where_count(P((W.EXISTS, 0, 0, 0))) == 0
    finally:
        eng.close()


# ---------------------------------------------------------------- life cycle
def test_points_survive_regrowth_and_compaction():
    rng = np.random.default_rng(53)
    col = GH.random_points(rng, 9000, VIENNA)
    centre = _pt(*VIENNA)
    tol = _tolerance(col, [centre])
    eng = HipScanEngine(4, "l2", device=0, capacity_hint=64)
    try:
        eng.define_attr(0, "geo")
        for first, last in ((0, 50), (50, 700), (700, 9000)):  # each append outgrows the capacity before it
            assert eng.append(np.ones((last - first, 4), np.float32)) == first
            eng.set_attr(0, first, col[first:last])
            assert np.array_equal(eng.get_attr(0, 0, last), col[:last])
        _check_nearest(eng, col, np.ones(9000, bool), centre, tol, tag="regrown")
        tomb = rng.random(9000) < 0.3
        eng.tombstone(np.flatnonzero(tomb))
        old = eng.compact()
        assert np.array_equal(old, np.flatnonzero(~tomb))
        kept = col[old]
        assert np.array_equal(eng.get_attr(0, 0, kept.size), kept)
        mask = GH.radius_mask(kept, centre, 25_000.0)
        _check_filter(eng, GH.radius_program(0, centre, 25_000.0), mask, "compacted")
        _check_nearest(eng, kept, np.ones(kept.size, bool), centre, tol, tag="compacted")
        eng.reset()
        assert eng.append(np.ones((10, 4), np.float32)) == 0
        assert (eng.get_attr(0, 0, 10) == GH.ABSENT).all()  # reset drops the values and keeps the definition
    finally:
        eng.close()


def _city_vectors(rng, n):
    lat = np.round(VIENNA[0] + rng.uniform(-2, 2, n), 6)
    lon = np.round(VIENNA[1] + rng.uniform(-3, 3, n), 6)
    return [Vector(values=rng.standard_normal(4).tolist(),
                   metadata={"loc": None if i % 9 == 4 else ((lat[i], lon[i]) if i % 2 else {"lat": lat[i], "lon": lon[i]}),
                             "stock": int(i % 5), "name": f"shop{i}"}) for i in range(n)]


def test_update_attributes_by_id_and_a_snapshot_round_trip(tmp_path):
    rng = np.random.default_rng(61)
    vs = _city_vectors(rng, 400)
    index = Index(space="l2", attributes={"loc": "geo", "stock": "int"})
    loaded = Index(space="l2")
    try:
        index.add(vs, "ns")
        col = W.encode_column("loc", "geo", [v.metadata["loc"] for v in vs], {})
        assert index.update_attributes([vs[0].id, vs[1].id, vs[4].id], [{"loc": (1.25, 2.5)}, {"loc": None}, {"loc": VIENNA}], "ns") == 3
        col[[0, 1, 4]] = [_pt(1.25, 2.5), GH.ABSENT, _pt(*VIENNA)]
        assert np.array_equal(index._ns["ns"].engine.get_attr(0, 0, 400), col)
        index.remove([vs[7].id, vs[8].id], "ns")
        live = np.ones(400, bool)
        live[[7, 8]] = False
        top, d, matched, absent = GH.nearest_oracle(col, live, _pt(*VIENNA))
        tol = _tolerance(col, [_pt(*VIENNA)])
        got = index.nearest("ns", "loc", VIENNA, 50, offset=0)
        assert got["ids"] == [vs[i].id for i in top[:50]] and got["ids"][0] == vs[4].id and got["distances"][0] == 0.0
        assert (got["matched"], got["absent"]) == (matched, absent) == (398, int((col[live] == GH.ABSENT).sum()))
        assert got["points"] == [W.geo_degrees(int(col[i])) for i in top[:50]]
        want = np.array(d[:50], dtype=GH.LD)
        assert (np.abs(np.array(got["distances"][1:], dtype=GH.LD) - want[1:]) <= tol * want[1:]).all()
        index.save_index(str(tmp_path))
        manifest = json.loads((tmp_path / "index.json").read_text())
        assert manifest["format"] == "mlvdb-index-v5" and manifest["attributes"] == {"loc": "geo", "stock": "int"}
        assert np.array_equal(np.fromfile(tmp_path / "ns0.attr0.i64", dtype=np.int64), col)
        assert loaded.load_index(str(tmp_path)) and loaded.attributes == index.attributes
        assert loaded.nearest("ns", "loc", VIENNA, 50) == got
        where = {"loc": {"$geo_radius": {"center": VIENNA, "radius": 120_000}}, "stock": {"$gte": 2}}
        assert loaded.count("ns", where) == index.count("ns", where) == \
            int((GH.radius_mask(col, _pt(*VIENNA), 120_000.0) & live & (np.arange(400) % 5 >= 2)).sum()) > 0
    finally:
        index.close()
        loaded.close()


@pytest.mark.parametrize("schema, fmt", [({}, "mlvdb-index-v1"), ({"stock": "int"}, "mlvdb-index-v2"),
                                         ({"tags": "str[]"}, "mlvdb-index-v3"), ({"terms": "sparse"}, "mlvdb-index-v4")])
def test_an_index_without_a_geo_attribute_writes_the_format_it_wrote_before(tmp_path, schema, fmt):
    index = Index(space="l2", attributes=schema)
    try:
        index.add([Vector(values=[1.0, 2.0, 3.0, 4.0], metadata={"stock": 1, "tags": ["a"], "terms": {3: 1.0}})], "ns")
        index.save_index(str(tmp_path))
        assert json.loads((tmp_path / "index.json").read_text())["format"] == fmt
    finally:
        index.close()


# ---------------------------------------------------------------- QueryProcessor
def test_query_processor_find_nearby_end_to_end():
    rng = np.random.default_rng(71)
    vs = _city_vectors(rng, 300)
    qp = QueryProcessor(InMemoryStorage(), Index(space="l2", attributes={"loc": "geo", "stock": "int"}))
    try:
        qp.upsert_many(vs, "ns")
        stored = qp.get_namespace_vectors("ns")
        assert [v["metadata"]["name"] for v in stored] == [v.metadata["name"] for v in vs]
        col = W.encode_column("loc", "geo", [v.metadata["loc"] for v in vs], {})
        stock = np.arange(300) % 5
        centre = (48.0, 16.0)
        tol = _tolerance(col, [_pt(*centre)])
        where = {"stock": {"$gte": 1}, "loc": {"$geo_radius": {"center": centre, "radius": 150_000}}}
        mask = (stock >= 1) & GH.radius_mask(col, _pt(*centre), 150_000.0)
        top, d, _, _ = GH.nearest_oracle(col, mask, _pt(*centre))
        assert 20 < top.size < 300
        for _ in range(2):
            hits = qp.find_nearby(centre, 20, "ns", "loc", where=where, offset=3)
            assert [h["metadata"]["name"] for h in hits] == [f"shop{i}" for i in top[3:23]]
            assert [h["id"] for h in hits] == [stored[i]["id"] for i in top[3:23]]
            assert all(h["metadata"] == vs[i].metadata and np.allclose(h["values"], vs[i].values) for h, i in zip(hits, top[3:23]))
            got = np.array([h["distance"] for h in hits], dtype=GH.LD)
            assert (np.abs(got - d[3:23]) <= tol * d[3:23]).all() and all(h["distance"] <= 150_000 for h in hits)
            assert [h["point"] for h in hits] == [W.geo_degrees(int(col[i])) for i in top[3:23]]
        moved = stored[int(top[3])]["id"]
        qp.update_metadata([moved], {"loc": centre}, "ns")
        first = qp.find_nearby(centre, 1, "ns", "loc")[0]
        assert first["id"] == moved and first["distance"] == 0.0 and first["metadata"]["loc"] == centre
        assert qp.update_where({"loc": {"$geo_radius": {"center": centre, "radius": 0}}}, {"loc": None}, "ns") == 1
        assert qp.find_nearby(centre, 1, "ns", "loc")[0]["id"] != moved
        assert [v for v in qp.get_namespace_vectors("ns") if v["id"] == moved][0]["metadata"].get("loc") is None
    finally:
        qp._index.close()
