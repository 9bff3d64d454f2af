"""Facet counts and histograms (include/mlvdb_facet.h) without a GPU: the C ABI's shape, the refusals of ``Index.facets`` /
``Index.histogram`` / ``QueryProcessor``, ordering and decoding over an oracle engine, and the host path of a predicate
``where`` against the dict path."""
import ctypes as C
import re
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, _native
from tests import facet_helpers as F
from tests.where_helpers import SCHEMA, py_match, random_filter, random_metadata

ROOT = Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------- C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_facet.h").read_text(), flags=re.S)


def test_facet_header_declares_what_the_binding_binds():
    lib = _native.load()
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", _header())))
    assert names == ["mlvdb_facet_bins", "mlvdb_facet_values"] == sorted(_native.FACET_SIGNATURES)
    for name in names:
        assert hasattr(lib, name)
        params = re.search(name + r"\((.*?)\);", _header(), flags=re.S).group(1).split(",")
        assert len(params) == len(_native.FACET_SIGNATURES[name][1])
    known = set(_native.SIGNATURES) | set(_native.WHERE_SIGNATURES) | set(_native.WHERE_EACH_SIGNATURES) | \
        set(_native.WHERE_EACH_RANGE_SIGNATURES) | set(_native.DISTINCT_SIGNATURES)
    assert not set(names) & known
    assert lib.mlvdb_abi_version() == 7 == _native.ABI_VERSION
    assert re.search(r"#define MLVDB_FACET_MAX_VALUES \(1 << 20\)", _header()) and _native.FACET_MAX_VALUES == F.MAX_VALUES
    assert re.search(r"#define MLVDB_FACET_MAX_EDGES 4096\b", _header()) and _native.FACET_MAX_EDGES == F.MAX_EDGES


def test_facet_entries_refuse_a_null_handle_inside_the_exception_guard():
    lib = _native.load()
    buf = (C.c_int64 * 8)()
    n = C.c_int64(0)
    assert lib.mlvdb_facet_values(C.c_void_p(), 0, None, 4, buf, buf, C.byref(n), C.byref(n), C.byref(n)) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    assert lib.mlvdb_facet_bins(C.c_void_p(), 0, None, buf, 1, buf, C.byref(n), C.byref(n)) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    for name in ("mlvdb_facet_values", "mlvdb_facet_bins"):
        body = re.search(r"^int " + name + r"\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
        assert body.lstrip().startswith("return guarded(")


def test_the_facet_kernels_are_in_the_build_and_the_helper_mirrors_their_constants():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_facet\.hip\b", make, flags=re.M) and "mlvdb_facet.h" in make
    internal = (ROOT / "mlvectordb_amd" / "csrc" / "internal.h").read_text()
    assert re.search(rf"kFacetLdsSlots = {F.LDS_SLOTS};", internal) and re.search(rf"kFacetLdsProbes = {F.LDS_PROBES};", internal)
    assert "0x9E3779B97F4A7C15ull" in internal and "x ^ (x >> 32)" in internal
    # the mirrored hash against plain Python integers
    for v in (0, 1, -1, 12345, F.INT64_MAX, F.ABSENT + 1):
        x = (v * 0x9E3779B97F4A7C15) % 2 ** 64
        assert int(F.facet_hash(v)) == x ^ (x >> 32)
    keys = F.colliding_keys(F.LDS_SLOTS, F.LDS_PROBES + 4)
    assert np.unique(keys).size == keys.size and set((F.facet_hash(keys) & np.uint64(F.LDS_SLOTS - 1)).tolist()) == {5}
    assert [F.global_slots(m) for m in (1, 32, 33, 64, 1 << 20)] == [64, 64, 128, 128, 1 << 21]


# ---------------------------------------------------------------- Index / QueryProcessor over the oracle engine
class UntouchableEngine(F.FacetOracleEngine):
    """Fails the test if a facet call reaches the engine."""

    def facet_values(self, *a, **kw):
        raise AssertionError("the engine was touched")

    facet_bins = facet_values


def _filled(factory=F.FacetOracleEngine, n=600, seed=2):
    rng = np.random.default_rng(seed)
    index = Index(space="l2", engine_factory=factory, attributes=SCHEMA)
    vecs = [Vector(values=rng.standard_normal(4).astype(np.float32), metadata=m) for m in random_metadata(rng, n)]
    index.add(vecs[:400], "ns")
    index.add(vecs[400:], "ns")
    gone = {v.id for v in vecs[::7]}
    index.remove(list(gone), "ns")
    return rng, index, [v for v in vecs if v.id not in gone]


def test_facets_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, _ = _filled(UntouchableEngine)
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.facets("ns", "author")
    with pytest.raises(ValueError, match="float column"):
        index.facets("ns", "price")
    with pytest.raises(ValueError, match="float column"):
        index.facets("ns", ["genre", "price"])
    with pytest.raises(ValueError, match="order must be"):
        index.facets("ns", "genre", order="alpha")
    for limit in (0, -3):
        with pytest.raises(ValueError, match="limit must be"):
            index.facets("ns", "genre", limit=limit)
    for mv in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="max_values must be"):
            index.facets("ns", "year", max_values=mv)
    with pytest.raises(ValueError, match="one dict filter"):
        index.facets("ns", "genre", [{"year": 2000}])
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.facets("ns", "genre", {"nope": 1})
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="dict filter, a predicate or None"):
        qp.facets("genre", where=[{"year": 2000}], namespace="ns")
    with pytest.raises(ValueError, match="float column"):
        qp.facets("price", where=lambda m: True, namespace="ns")


def test_histogram_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, _ = _filled(UntouchableEngine)
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.histogram("ns", "author", [1])
    for by in ("genre", "in_stock"):
        with pytest.raises(ValueError, match="int or float attribute"):
            index.histogram("ns", by, [1])
    with pytest.raises(ValueError, match="is not an int"):
        index.histogram("ns", "year", [1990, 2000.0])
    with pytest.raises(ValueError, match="is not an int or float"):
        index.histogram("ns", "price", [1.0, "2"])
    with pytest.raises(ValueError, match="is not an int or float"):
        index.histogram("ns", "price", [True])
    with pytest.raises(ValueError, match="outside int64"):
        index.histogram("ns", "year", [-2 ** 63, 0])
    for edges in ([2000, 1990], [1990, 1990], [1.0, 0.5]):
        with pytest.raises(ValueError, match="strictly ascending"):
            index.histogram("ns", "year" if isinstance(edges[0], int) else "price", edges)
    with pytest.raises(ValueError, match="NaN"):
        index.histogram("ns", "price", [0.0, float("nan")])
    for edges in ([], list(range(4097))):
        with pytest.raises(ValueError, match="1..4096 edges"):
            index.histogram("ns", "year", edges)
    with pytest.raises(ValueError, match="one dict filter"):
        index.histogram("ns", "year", [2000], [{"year": 1}])
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="strictly ascending"):
        qp.histogram("year", [3, 2], where=lambda m: True, namespace="ns")


def _want_facets(live, by, where):
    rows = [v.metadata for v in live if where is None or py_match(where, v.metadata)]
    vals = [m.get(by) for m in rows]
    present = [x for x in vals if x is not None]
    return Counter(present), len(rows), len(rows) - len(present)


def test_facets_order_ties_limit_and_decoding():
    rng, index, live = _filled()
    for where in (None, {"in_stock": True}, {"year": {"$gte": 1990}, "genre": {"$ne": "rock"}}, {"genre": "zydeco"}):
        for by in ("genre", "year", "in_stock"):
            want, matched, absent = _want_facets(live, by, where)
            got = index.facets("ns", by, where)
            assert got["matched"] == matched and got["absent"] == absent
            assert got["values"] == sorted(want.items(), key=lambda p: (-p[1], p[0]))
            assert all(type(v) is {"genre": str, "year": int, "in_stock": bool}[by] for v, _ in got["values"])
            assert sum(c for _, c in got["values"]) + absent == matched
            by_value = index.facets("ns", by, where, order="value")
            assert by_value["values"] == sorted(want.items())
            assert index.facets("ns", by, where, limit=2)["values"] == got["values"][:2]
            assert index.facets("ns", by, where, limit=2, order="value")["values"] == by_value["values"][:2]
    years = index.facets("ns", "year")["values"]
    assert any(a[1] == b[1] and a[0] < b[0] for a, b in zip(years, years[1:]))  # ties by value ascending are exercised
    # the list form: one answer per attribute
    both = index.facets("ns", ["genre", "in_stock"], {"year": {"$lt": 2000}})
    assert both == {by: index.facets("ns", by, {"year": {"$lt": 2000}}) for by in ("genre", "in_stock")}
    # an int attribute with more distinct values than max_values: a ValueError naming it; exactly as many: fine
    distinct = len(years)
    assert len(index.facets("ns", "year", max_values=distinct)["values"]) == distinct
    with pytest.raises(ValueError, match=f"max_values={distinct - 1}"):
        index.facets("ns", "year", max_values=distinct - 1)
    assert index.facets("other", "genre") == {"values": [], "matched": 0, "absent": 0}
    assert index.facets("other", ["genre", "year"]) == {by: {"values": [], "matched": 0, "absent": 0} for by in ("genre", "year")}


def test_a_string_whose_rows_are_all_tombstoned_does_not_appear():
    rng = np.random.default_rng(0)
    index = Index(space="l2", engine_factory=F.FacetOracleEngine, attributes=SCHEMA)
    vecs = [Vector(values=rng.standard_normal(4).astype(np.float32), metadata={"genre": g})
            for g in ["jazz", "dub", "jazz", "dub", "folk"]]
    index.add(vecs, "ns")
    index.remove([v.id for v in vecs if v.metadata["genre"] == "dub"], "ns")
    assert index.facets("ns", "genre") == {"values": [("jazz", 2), ("folk", 1)], "matched": 3, "absent": 0}
    assert index.facets("ns", "year") == {"values": [], "matched": 3, "absent": 3}


def test_histogram_equals_searchsorted_over_the_matching_rows():
    rng, index, live = _filled()
    for where in (None, {"in_stock": False}, {"genre": {"$in": ["jazz", "pop"]}}):
        rows = [v.metadata for v in live if where is None or py_match(where, v.metadata)]
        for by, edges in (("year", [1960, 1980, 2000, 2024]), ("year", [1950]), ("price", [0, 10.0, 50, 99.9]),
                          ("price", np.array([-np.inf, 25.5, np.inf]))):
            vals = [m.get(by) for m in rows]
            present = [x for x in vals if x is not None and x == x]
            got = index.histogram("ns", by, edges, where)
            e = np.asarray(edges, dtype=np.int64 if by == "year" else np.float64)
            want = np.bincount(np.searchsorted(e, np.asarray(present, dtype=e.dtype), side="right"), minlength=e.size + 1)
            assert got["counts"].dtype == np.int64 and got["counts"].tolist() == want.tolist()
            assert got["matched"] == len(rows) and got["absent"] == len(rows) - len(present)
    empty = index.histogram("other", "year", [1, 2])
    assert empty["counts"].tolist() == [0, 0, 0] and empty["matched"] == 0 and empty["absent"] == 0


def test_query_processor_predicate_path_agrees_with_the_dict_path():
    rng = np.random.default_rng(5)
    qp = QueryProcessor(InMemoryStorage(), Index(space="l2", engine_factory=F.FacetOracleEngine, attributes=SCHEMA))
    metas = random_metadata(rng, 500)
    vecs = [Vector(values=rng.standard_normal(4).astype(np.float32), metadata=m) for m in metas]
    qp.upsert_many(vecs, "ns")
    stored = list(qp._storage.namespace_map["ns"])  # the stored vectors carry the ids minted at upsert
    assert len(qp.delete([v.id for v in stored[::11]], "ns")) == len(stored[::11])
    assert qp.facets("genre", namespace="ns")["matched"] == len(stored) - len(stored[::11])
    for f in [None] + [random_filter(rng) for _ in range(25)]:
        pred = (lambda m: True) if f is None else (lambda m, f=f: py_match(f, m))
        for by in ("genre", "year", "in_stock"):
            for order in ("count", "value"):
                assert qp.facets(by, where=pred, namespace="ns", order=order, limit=5) == \
                    qp.facets(by, where=f, namespace="ns", order=order, limit=5), (f, by)
        assert qp.facets(["genre", "year"], where=pred, namespace="ns") == qp.facets(["genre", "year"], where=f, namespace="ns")
        for by, edges in (("year", [1970, 1990, 2010]), ("price", [10, 33.3, 80.0])):
            a, b = qp.histogram(by, edges, where=pred, namespace="ns"), qp.histogram(by, edges, where=f, namespace="ns")
            assert a["counts"].tolist() == b["counts"].tolist() and (a["matched"], a["absent"]) == (b["matched"], b["absent"])
    assert qp.facets("genre", namespace="nowhere") == {"values": [], "matched": 0, "absent": 0}
    assert qp.facets("genre", where=lambda m: True, namespace="nowhere") == {"values": [], "matched": 0, "absent": 0}
