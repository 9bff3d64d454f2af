"""Geo attributes (include/mlvdb_geo.h) without a device: packing, the compiled programs and every refusal of where.py and
``Index``, the NumPy oracle against hand-computed distances, the header's constants and symbol, ``Index`` / ``QueryProcessor``
over the NumPy model engine, and the snapshot format chosen per schema."""
import ctypes as C
import json
import math
import re
from pathlib import Path
from uuid import UUID

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, _native
from mlvectordb_amd import where as W
from tests import geo_helpers as GH

ROOT = Path(__file__).resolve().parents[1]
SCHEMA = {"loc": "geo", "stock": "int", "genre": "str"}


# ---------------------------------------------------------------- packing
@pytest.mark.parametrize("lat, lon", [(90, 180), (-90, -180), (90, -180), (-90, 180), (0, 0), (12.3456789, -179.9999999)])
def test_pack_and_unpack_round_trip(lat, lon):
    v = W.geo_pack((lat, lon))
    assert -(2 ** 63) < v < 2 ** 63 and v != W.INT64_ABSENT
    assert W.geo_unpack(v) == (round(lat * 1e7), round(lon * 1e7))
    assert W.geo_pack({"lat": lat, "lon": lon}) == v == int(GH.quantise([lat], [lon])[0])
    assert W.geo_degrees(v) == (round(lat * 1e7) / 1e7, round(lon * 1e7) / 1e7)
    la, lo = GH.unpack(np.array([v]))
    assert (int(la[0]), int(lo[0])) == W.geo_unpack(v)


def test_the_packed_layout_is_lat_high_lon_low():
    assert W.geo_pack((1e-7, 2e-7)) == (1 << 32) | 2
    assert W.geo_pack((-1e-7, -1e-7)) == -1  # lat -1 << 32 | 0xFFFFFFFF
    assert W.geo_unpack(W.INT64_ABSENT)[0] == -(2 ** 31)  # absent decodes to no latitude


def test_none_maps_to_absent_and_a_batch_is_packed():
    col = W.encode_column("loc", "geo", [None, (1, 2), {"lat": -3.5, "lon": 4}], {})
    assert col.dtype == np.int64 and col[0] == W.INT64_ABSENT
    assert col[1:].tolist() == [W.geo_pack((1, 2)), W.geo_pack((-3.5, 4))]
    assert W.column_kind("geo") == "geo" and W.is_geo("geo") and not W.is_pooled("geo") and W.GEO_TYPES == ("geo",)


@pytest.mark.parametrize("bad", [(91, 0), (0, 180.1), (-90.0000001, 0), (float("nan"), 0), (0, float("inf")), (1,), (1, 2, 3),
                                 "1,2", 5, {"lat": 1}, {"lat": 1, "lon": 2, "alt": 3}, (True, 1), ("1", 2)])
def test_a_bad_point_is_refused_naming_the_attribute(bad):
    with pytest.raises(ValueError, match="'loc'"):
        W.encode_column("loc", "geo", [bad], {})
    with pytest.raises(ValueError, match="'loc'"):
        W.compile_where({"loc": {"$geo_radius": {"center": bad, "radius": 1}}}, SCHEMA)


# ---------------------------------------------------------------- compiled programs
def test_compiled_radius_program():
    p = W.compile_where({"loc": {"$geo_radius": {"center": (48.2, 16.37), "radius": 2000}}}, SCHEMA)
    thr = math.sin(2000 / (2 * 6371008.8)) ** 2
    assert p.ops.tolist() == [(W.GEO_RADIUS, 0, W.geo_pack((48.2, 16.37)), W.float_bits(thr))] and p.set.size == 0
    zero = W.compile_where({"loc": {"$geo_radius": {"center": {"lat": 0, "lon": 0}, "radius": 0}}}, SCHEMA)
    assert zero.ops.tolist() == [(W.GEO_RADIUS, 0, 0, 0)]  # sin^2(0): the bits of 0.0
    for r in (math.pi * 6371008.8, 3e7, 1e300):
        full = W.compile_where({"loc": {"$geo_radius": {"center": (0, 0), "radius": r}}}, SCHEMA)
        assert full.ops["b"][0] == W.float_bits(1.0)
    assert (W.GEO_BOX, W.GEO_RADIUS) == (16, 17)


def test_compiled_box_program_and_composition():
    p = W.compile_where({"loc": {"$geo_box": {"sw": (-10, 170), "ne": (10, -170)}}, "stock": {"$gt": 0}}, SCHEMA)
    assert p.ops.tolist() == [(W.GEO_BOX, 0, W.geo_pack((-10, 170)), W.geo_pack((10, -170))), (W.GT, 1, 0, 0), (W.AND, 0, 0, 0)]
    q = W.compile_where({"$or": [{"loc": {"$exists": False}}, {"$not": {"loc": {"$geo_box": {"sw": (1, 1), "ne": (1, 1)}}}}]},
                        SCHEMA)
    assert q.ops["op"].tolist() == [W.EXISTS, W.NOT, W.GEO_BOX, W.NOT, W.OR]
    progs, of = W.compile_each([{"loc": {"$geo_radius": {"center": (1, 2), "radius": 50}}}, None,
                                {"loc": {"$geo_radius": {"center": (1, 2), "radius": 50.0}}}], SCHEMA)
    assert len(progs) == 1 and of.tolist() == [0, -1, 0]
    assert len(W.chunk_programs(progs, of)) == 1


@pytest.mark.parametrize("where, needle", [
    ({"loc": (1, 2)}, "geo attribute"),
    ({"loc": {"$eq": (1, 2)}}, "geo attribute"),
    ({"loc": {"$gt": 1}}, r"\$geo_radius, \$geo_box and \$exists"),
    ({"loc": {"$in": [(1, 2)]}}, "geo attribute"),
    ({"loc": {"$size": 1}}, "geo attribute"),
    ({"loc": {"$all": [1]}}, "geo attribute"),
    ({"stock": {"$geo_radius": {"center": (1, 2), "radius": 5}}}, "geo attributes only"),
    ({"genre": {"$geo_box": {"sw": (1, 2), "ne": (3, 4)}}}, "geo attributes only"),
    ({"loc": {"$geo_radius": {"center": (1, 2)}}}, "'center' and 'radius'"),
    ({"loc": {"$geo_radius": {"center": (1, 2), "radius": 5, "unit": "km"}}}, "'center' and 'radius'"),
    ({"loc": {"$geo_radius": (1, 2, 5)}}, "'center' and 'radius'"),
    ({"loc": {"$geo_radius": {"center": (1, 2), "radius": -1}}}, "finite and >= 0"),
    ({"loc": {"$geo_radius": {"center": (1, 2), "radius": float("inf")}}}, "finite and >= 0"),
    ({"loc": {"$geo_radius": {"center": (1, 2), "radius": float("nan")}}}, "finite and >= 0"),
    ({"loc": {"$geo_radius": {"center": (1, 2), "radius": "5"}}}, "not a number"),
    ({"loc": {"$geo_box": {"sw": (1, 2)}}}, "'sw' and 'ne'"),
    ({"loc": {"$geo_box": {"sw": (3, 2), "ne": (1, 4)}}}, "north of ne"),
    ({"loc": {"$geo_box": {"sw": (1, 2), "ne": (95, 4)}}}, "outside lat"),
])
def test_refused_filters_name_the_attribute(where, needle):
    with pytest.raises(ValueError, match=needle) as e:
        W.compile_where(where, SCHEMA)
    assert "'loc'" in str(e.value) or "'stock'" in str(e.value) or "'genre'" in str(e.value)


# ---------------------------------------------------------------- the oracle against hand-computed cases
def test_oracle_same_point_is_exactly_zero():
    for p in GH.quantise([0, 89.9, -90, 12.3456789], [0, 179.9999, 0, -45.5]):
        for dtype in (GH.LD, np.float64):
            assert GH.dist(np.array([p]), p, dtype)[0] == 0


def test_oracle_one_degree_of_latitude():
    want = GH.LD(GH.R) * GH.PI_LD / 180
    for lon in (0.0, 77.0, -180.0):
        d = GH.dist(GH.quantise([11.0], [lon]), GH.quantise([10.0], [lon])[0])[0]
        assert abs(d - want) <= 1e-17 * want
    assert abs(float(want) - 111195.08023353292) < 1e-6


def test_oracle_across_the_antimeridian():
    # 0.0002 degrees of longitude apart on the equator, on the two sides of +-180
    d = GH.dist(GH.quantise([0.0], [-179.9999]), GH.quantise([0.0], [179.9999])[0])[0]
    want = GH.LD(GH.R) * GH.PI_LD / 180 * GH.LD("0.0002")
    assert abs(d - want) <= 1e-15 * want and 22.2 < float(d) < 22.3
    # lon -180 and +180 are the same meridian
    assert GH.dist(GH.quantise([5.0], [-180.0]), GH.quantise([5.0], [180.0])[0])[0] == 0


def test_oracle_pole_to_pole():
    d = GH.dist(GH.quantise([-90.0], [33.0]), GH.quantise([90.0], [-120.0])[0])[0]
    want = GH.PI_LD * GH.LD(GH.R)
    assert abs(d - want) <= 1e-9 * want  # (asin is steep at 1: sqrt(eps) of long double)
    assert float(GH.hav(GH.quantise([-90.0], [33.0]), GH.quantise([90.0], [-120.0])[0])[0]) == pytest.approx(1.0, abs=1e-18)


def test_oracle_box_is_inclusive_and_wraps():
    col = GH.quantise([0, 0, 0, 0, 5, -5.0000001], [170, -170, 180, 0, 175, 175])
    col = np.append(col, GH.ABSENT)
    wrap = GH.box_mask(col, W.geo_pack((-5, 170)), W.geo_pack((5, -170)))
    assert wrap.tolist() == [True, True, True, False, True, False, False]
    plain = GH.box_mask(col, W.geo_pack((-5, -170)), W.geo_pack((5, 170)))
    assert plain.tolist() == [True, True, False, True, False, False, False]


def test_the_guards_trip_where_they_must():
    col = GH.quantise([0.0, 0.0], [1.0, -1.0])  # mirror images: the same distance from (0, 0)
    with pytest.raises(AssertionError, match="rank guard"):
        GH.nearest_oracle(col, np.ones(2, bool), 0)
    d = float(GH.dist(col[:1], 0)[0])
    with pytest.raises(AssertionError, match="radius guard"):
        GH.radius_mask(col, 0, d)
    assert GH.radius_mask(np.array([0, col[0]]), 0, 0.0).tolist() == [True, False]  # d == 0 under r == 0 is exempt


# ---------------------------------------------------------------- the header and the library
def test_geo_header_constants_symbol_and_binding():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_geo.h").read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))
    assert names == ["mlvdb_geo_nearest"] == sorted(_native.GEO_SIGNATURES)
    params = re.search(r"mlvdb_geo_nearest\s*\(([^)]*)\)", text).group(1).split(",")
    assert len(params) == len(_native.GEO_SIGNATURES["mlvdb_geo_nearest"][1]) == 12
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?[\d.]+)", text))
    assert int(consts["MLVDB_ATTR_GEO"]) == _native.ATTR_GEO == _native.ATTR_CODES["geo"] == 5
    assert int(consts["MLVDB_WHERE_GEO_BOX"]) == W.GEO_BOX == _native.WHERE_GEO_BOX == 16
    assert int(consts["MLVDB_WHERE_GEO_RADIUS"]) == W.GEO_RADIUS == _native.WHERE_GEO_RADIUS == 17
    assert int(consts["MLVDB_GEO_LAT_MAX_E7"]) == W.GEO_LAT_MAX_E7 == 900_000_000
    assert int(consts["MLVDB_GEO_LON_MAX_E7"]) == W.GEO_LON_MAX_E7 == 1_800_000_000
    assert float(consts["MLVDB_GEO_EARTH_RADIUS_M"]) == W.GEO_EARTH_RADIUS_M == GH.R == 6371008.8
    others = [t for n, t in vars(_native).items() if n.endswith("SIGNATURES") and n != "GEO_SIGNATURES"]
    assert all("mlvdb_geo_nearest" not in t for t in others)
    lib = _native.load()
    assert hasattr(lib, "mlvdb_geo_nearest")
    assert lib.mlvdb_abi_version() == _native.ABI_VERSION == 7


def test_geo_nearest_refuses_a_null_handle_inside_the_guard():
    lib = _native.load()
    buf = (C.c_int64 * 4)()
    z = C.c_int64(0)
    assert lib.mlvdb_geo_nearest(C.c_void_p(), 0, 0, None, 0, 1, buf, buf, buf, C.byref(z), C.byref(z), C.byref(z)) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    body = re.search(r"^int mlvdb_geo_nearest\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
    assert body.lstrip().startswith("return guarded(")


def test_the_geo_headers_are_in_the_build_and_hav_is_one_function():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    hdrs = make[make.index("HDRS ="):make.index("# the filter scan")]
    assert "../../include/mlvdb_geo.h" in hdrs and "geo_common.h" in hdrs
    csrc = ROOT / "mlvectordb_amd" / "csrc"
    defs = {p.name: len(re.findall(r"\bdouble geo_hav\s*\(", p.read_text())) for p in list(csrc.glob("*.hip")) + list(csrc.glob("*.h"))}
    assert {n for n, c in defs.items() if c} == {"geo_common.h"} and defs["geo_common.h"] == 1
    text = (csrc / "geo_common.h").read_text()
    assert "__device__ __forceinline__ double geo_hav" in text and "#pragma clang fp contract(off)" in text
    users = {p.name for p in csrc.glob("*") if p.suffix in (".hip", ".h") and re.search(r"\bgeo_hav\(", p.read_text())}
    assert users == {"geo_common.h", "where_common.h", "kernels_order.hip"}


# ---------------------------------------------------------------- Index and QueryProcessor on the NumPy model engine
CITIES = {"vienna": (48.2082, 16.3738), "bratislava": (48.1486, 17.1077), "graz": (47.0707, 15.4395),
          "suva": (-18.1416, 178.4419), "apia": (-13.8333, -171.7667), "nowhere": None}


def gidx(**kw):
    return Index(space="l2", engine_factory=GH.oracle_engine_class(), attributes=SCHEMA, **kw)


def cities():
    return [Vector(values=[float(i), 0.0, 0.0, 1.0], metadata={"loc": p, "stock": i, "genre": name, "name": name})
            for i, (name, p) in enumerate(CITIES.items())]


def test_index_nearest_and_filters_on_the_model_engine():
    index, vs = gidx(), cities()
    index.add(vs, "ns")
    ids = {v.metadata["name"]: v.id for v in vs}
    got = index.nearest("ns", "loc", CITIES["vienna"], 10)
    assert got["ids"] == [ids[n] for n in ("vienna", "bratislava", "graz", "apia", "suva")]
    assert (got["matched"], got["absent"]) == (6, 1)
    assert got["points"][0] == CITIES["vienna"] and got["distances"][0] == 0.0
    assert 54_000 < got["distances"][1] < 56_000 and 144_000 < got["distances"][2] < 146_000
    near = {"loc": {"$geo_radius": {"center": CITIES["vienna"], "radius": 100_000}}}
    assert index.count("ns", near) == 2
    assert index.nearest("ns", "loc", {"lat": 47, "lon": 15}, 1, where=near, offset=1)["ids"] == [ids["bratislava"]]
    pacific = {"loc": {"$geo_box": {"sw": (-20, 170), "ne": (-10, -170)}}}
    assert index.query_by_metadata("ns", pacific) == [ids["suva"], ids["apia"]]
    assert index.count("ns", {"loc": {"$exists": False}}) == 1
    assert index.nearest("other", "loc", (0, 0), 5) == {"ids": [], "points": [], "distances": [], "matched": 0, "absent": 0}


def test_index_updates_of_geo_values():
    index, vs = gidx(), cities()
    index.add(vs, "ns")
    assert index.update_attributes([vs[5].id, vs[0].id], [{"loc": (1.5, 2.5)}, {"loc": None}], "ns") == 2
    got = index.nearest("ns", "loc", (1.5, 2.5), 1)
    assert got["ids"] == [vs[5].id] and got["points"] == [(1.5, 2.5)] and (got["matched"], got["absent"]) == (6, 1)
    europe = {"loc": {"$geo_box": {"sw": (40, 10), "ne": (50, 20)}}}
    assert index.update_where("ns", europe, {"loc": {"lat": -1, "lon": -2}}) == 2
    assert index.count("ns", {"loc": {"$geo_radius": {"center": (-1, -2), "radius": 0}}}) == 2
    assert index.update_where("ns", {"stock": {"$gte": 0}}, {"loc": None}) == 6
    assert index.count("ns", {"loc": {"$exists": True}}) == 0


@pytest.mark.parametrize("call, needle", [
    (lambda i: i.update_where("ns", {"stock": 1}, {"loc": {"$inc": 1}}), r"geo attribute.*\$inc"),
    (lambda i: i.update_where("ns", {"stock": 1}, {"loc": (91, 0)}), "outside lat"),
    (lambda i: i.update_attributes([UUID(int=1)], {"loc": 5}, "ns"), "not a point"),
    (lambda i: i.top_by("ns", "loc", 5), "top_by.*geo column"),
    (lambda i: i.facets("ns", "loc"), "facets.*geo column"),
    (lambda i: i.histogram("ns", "loc", [1, 2]), "histogram.*geo column"),
    (lambda i: i.search_many(np.zeros((1, 4), np.float32), 1, "ns", "l2", distinct="loc"), "distinct.*geo column"),
    (lambda i: i.search_late([np.zeros((1, 4), np.float32)], 1, "ns", "l2", by="loc"), "geo column"),
    (lambda i: i.nearest("ns", "stock", (0, 0), 5), "nearest.*needs a geo attribute"),
    (lambda i: i.nearest("ns", "nope", (0, 0), 5), "not a declared attribute"),
    (lambda i: i.nearest("ns", "loc", (0, 200), 5), "nearest: point"),
    (lambda i: i.nearest("ns", "loc", (0, 0), 0), "limit"),
    (lambda i: i.nearest("ns", "loc", (0, 0), 4000, offset=97), "offset \\+ limit"),
    (lambda i: i.nearest("ns", "loc", (0, 0), 5, where=[{}]), "one dict filter"),
])
def test_index_refusals(call, needle):
    index = gidx()
    index.add(cities(), "ns")
    with pytest.raises(ValueError, match=needle):
        call(index)


def test_the_schema_takes_geo_and_names_it_among_the_types():
    assert Index(space="l2", attributes={"loc": "geo"}).attributes == {"loc": "geo"}
    with pytest.raises(ValueError, match="geo"):
        Index(space="l2", attributes={"loc": "point"})


def test_query_processor_find_nearby_and_metadata_in_step():
    qp = QueryProcessor(InMemoryStorage(), gidx())
    vs = cities()
    qp.upsert_many(vs, "ns")
    ids = {v["metadata"]["name"]: v["id"] for v in qp.get_namespace_vectors("ns")}
    hits = qp.find_nearby(CITIES["graz"], 2, "ns", "loc", where={"stock": {"$lte": 2}})
    assert [h["metadata"]["name"] for h in hits] == ["graz", "vienna"]
    assert hits[0]["distance"] == 0.0 and hits[0]["point"] == CITIES["graz"] and 140_000 < hits[1]["distance"] < 150_000
    assert hits[0]["id"] == ids["graz"] and list(hits[0]["values"]) == [2.0, 0.0, 0.0, 1.0]
    qp.update_metadata([ids["graz"]], {"loc": (10, 10)}, "ns")
    qp.update_where({"genre": "vienna"}, {"loc": {"lat": 10.5, "lon": 10}}, "ns")
    hits = qp.find_nearby((10, 10), 2, "ns", "loc")
    assert [(h["metadata"]["name"], h["metadata"]["loc"]) for h in hits] == [("graz", (10, 10)), ("vienna", {"lat": 10.5, "lon": 10})]
    with pytest.raises(ValueError, match="dict filter or None"):
        qp.find_nearby((0, 0), 1, "ns", "loc", where=lambda m: True)


# ---------------------------------------------------------------- snapshots
def test_an_index_with_a_geo_attribute_writes_v5_and_loads_back(tmp_path):
    index, vs = gidx(), cities()
    index.add(vs, "ns")
    index.remove([vs[1].id], "ns")
    index.save_index(str(tmp_path))
    manifest = json.loads((tmp_path / "index.json").read_text())
    assert manifest["format"] == "mlvdb-index-v5" and manifest["attributes"] == SCHEMA
    col = np.fromfile(tmp_path / "ns0.attr0.i64", dtype=np.int64)
    assert col.tolist() == [W.INT64_ABSENT if p is None else W.geo_pack(p) for p in CITIES.values()]
    loaded = Index(space="l2", engine_factory=GH.oracle_engine_class())
    assert loaded.load_index(str(tmp_path)) and loaded.attributes == SCHEMA
    want = index.nearest("ns", "loc", (0, 0), 10)
    assert loaded.nearest("ns", "loc", (0, 0), 10) == want and len(want["ids"]) == 4
    manifest["format"] = "mlvdb-index-v4"  # an older format cannot hold a geo attribute
    (tmp_path / "index.json").write_text(json.dumps(manifest))
    with pytest.raises(RuntimeError, match="geo attribute"):
        Index(space="l2", engine_factory=GH.oracle_engine_class()).load_index(str(tmp_path))


@pytest.mark.parametrize("schema, fmt", [({}, "v1"), ({"stock": "int"}, "v2"), ({"tags": "str[]"}, "v3"),
                                         ({"stock": "int", "loc": "geo"}, "v5")])
def test_the_snapshot_format_is_chosen_per_schema(tmp_path, schema, fmt):
    index = Index(space="l2", engine_factory=GH.oracle_engine_class(), attributes=schema)
    if fmt != "v3":  # (the model engine holds no list columns; an empty index writes the manifest all the same)
        index.add([Vector(values=[1.0, 2.0], metadata={"stock": 3, "loc": (1, 2)})], "ns")
    index.save_index(str(tmp_path))
    assert json.loads((tmp_path / "index.json").read_text())["format"] == f"mlvdb-index-{fmt}"
