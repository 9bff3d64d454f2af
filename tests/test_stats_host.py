"""Attribute statistics (include/mlvdb_stats.h) without a GPU: the C ABI's shape, the refusals of ``Index.stats`` /
``QueryProcessor.stats``, the answers over an oracle engine against plain Python over the metadata, the host path of a
predicate ``where`` against the dict path, and the fixed-point rule of float sums itself against ``math.fsum``."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, _native
from mlvectordb_amd import stats as host_stats
from tests import stats_helpers as S
from tests.where_helpers import SCHEMA, py_match, random_filter, random_metadata

ROOT = Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------- C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_stats.h").read_text(), flags=re.S)


def test_stats_header_declares_what_the_binding_binds():
    lib = _native.load()
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", _header())))
    assert names == ["mlvdb_attr_stats"] == sorted(_native.STATS_SIGNATURES)
    for name in names:
        assert hasattr(lib, name)
        params = re.search(name + r"\((.*?)\);", _header(), flags=re.S).group(1).split(",")
        assert len(params) == len(_native.STATS_SIGNATURES[name][1]) == 15
    others = [getattr(_native, t) for t in dir(_native) if t.endswith("SIGNATURES") and t != "STATS_SIGNATURES"]
    assert len(others) >= 16 and not any(set(names) & set(table) for table in others)
    assert lib.mlvdb_abi_version() == 7 == _native.ABI_VERSION


def test_stats_entry_refuses_a_null_handle_inside_the_exception_guard():
    lib = _native.load()
    buf = (C.c_int64 * 8)()
    n = C.c_int64(0)
    assert lib.mlvdb_attr_stats(C.c_void_p(), 0, -1, None, 1, buf, buf, buf, buf, buf, buf, buf, C.byref(n), C.byref(n),
                                C.byref(n)) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    body = re.search(r"^int mlvdb_attr_stats\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
    assert body.lstrip().startswith("return guarded(") and body.rstrip().endswith("});")


def test_the_stats_kernels_are_in_the_build_and_the_helper_mirrors_their_constants():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_stats\.hip\b", make, flags=re.M) and "mlvdb_stats.h" in make
    internal = (ROOT / "mlvectordb_amd" / "csrc" / "internal.h").read_text()
    assert re.search(rf"kStatsLdsSlots = {S.LDS_SLOTS};", internal) and re.search(rf"kStatsLdsSlotsOne = {S.LDS_SLOTS_ONE};", internal)
    assert re.search(rf"kFacetLdsProbes = {S.LDS_PROBES};", internal) and re.search(rf"kFacetPeelRounds = {S.PEEL_ROUNDS};", internal)
    kernels = (ROOT / "mlvectordb_amd" / "csrc" / "kernels_stats.hip").read_text()
    assert f"{S.SCALE} - E" in kernels and "asm" not in kernels.replace("kernels_stats", "")


# ---------------------------------------------------------------- Index / QueryProcessor over the oracle engine
class UntouchableEngine(S.StatsOracleEngine):
    """Fails the test if a statistics call reaches the engine."""

    def attr_stats(self, *a, **kw):
        raise AssertionError("the engine was touched")


WIDE = dict(SCHEMA, tags="str[]", loc="geo", terms="sparse")


def _filled(factory=S.StatsOracleEngine, n=600, seed=2, schema=SCHEMA):
    rng = np.random.default_rng(seed)
    index = Index(space="l2", engine_factory=factory, attributes=schema)
    vecs = [Vector(values=rng.standard_normal(4).astype(np.float32), metadata=m) for m in random_metadata(rng, n)]
    index.add(vecs[:400], "ns")
    index.add(vecs[400:], "ns")
    gone = {v.id for v in vecs[::7]}
    index.remove(list(gone), "ns")
    return rng, index, [v for v in vecs if v.id not in gone]


def test_stats_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, _ = _filled(UntouchableEngine)
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.stats("ns", "author")
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.stats("ns", ["price", "author"])
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.stats("ns", "price", by="author")
    with pytest.raises(ValueError, match="is a str column"):
        index.stats("ns", "genre")
    with pytest.raises(ValueError, match="by='price' is a float column"):
        index.stats("ns", "year", by="price")
    with pytest.raises(ValueError, match="not a declared attribute"):  # a list of names is no group column
        index.stats("ns", "year", by=["genre", "in_stock"])
    for mg in (0, -1, (1 << 20) + 1, True, 2.0):
        with pytest.raises(ValueError, match="max_groups must be"):
            index.stats("ns", "price", by="year", max_groups=mg)
    with pytest.raises(ValueError, match="one dict filter"):
        index.stats("ns", "price", [{"year": 2000}])
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.stats("ns", "price", {"nope": 1})
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="dict filter, a predicate or None"):
        qp.stats("price", where=[{"year": 2000}], namespace="ns")
    with pytest.raises(ValueError, match="is a str column"):
        qp.stats("genre", where=lambda m: True, namespace="ns")
    with pytest.raises(ValueError, match="float column"):
        qp.stats("year", where=lambda m: True, namespace="ns", by="price")
    # list, sparse and geo columns are neither summarised nor grouped by
    wide = Index(space="l2", engine_factory=UntouchableEngine, attributes=WIDE)
    for name, what in (("tags", "scalar attribute"), ("terms", "sparse column"), ("loc", "geo column")):
        with pytest.raises(ValueError, match=what):
            wide.stats("ns", name)
        with pytest.raises(ValueError, match=what):
            wide.stats("ns", "price", by=name)
    sharded = Index(space="l2", engine_factory=UntouchableEngine, devices=[0, 1])
    with pytest.raises(ValueError, match="row-sharded"):
        sharded.stats("ns", "price")


def _want(live, attr, where, by=None):
    return S.metadata_stats([v.metadata for v in live], attr, where, by)


def test_stats_answers_equal_plain_python_over_the_metadata():
    rng, index, live = _filled()
    for where in (None, {"in_stock": True}, {"year": {"$gte": 1990}, "genre": {"$ne": "rock"}}, {"genre": "zydeco"}):
        for attr in ("price", "year", "in_stock"):
            got = index.stats("ns", attr, where)
            assert got == _want(live, attr, where), (attr, where)
            assert set(got) == {"matched", "count", "absent", "min", "max", "sum", "mean"}
            for by in ("genre", "year", "in_stock"):
                got = index.stats("ns", attr, where, by=by)
                want = _want(live, attr, where, by)
                assert got == want, (attr, by, where)
                assert sum(g["rows"] for _, g in got["groups"]) + got["by_absent"] == got["matched"]
                assert all(type(v) is {"genre": str, "year": int, "in_stock": bool}[by] for v, _ in got["groups"])
    total = index.stats("ns", "year")
    assert type(total["sum"]) is int and type(total["min"]) is int and total["mean"] == total["sum"] / total["count"]
    share = index.stats("ns", "in_stock")
    assert share["min"] is False and share["max"] is True and 0 < share["mean"] < 1 and type(share["sum"]) is int
    assert type(index.stats("ns", "price")["sum"]) is float
    # the list form: one answer per attribute
    both = index.stats("ns", ["price", "year"], {"year": {"$lt": 2000}}, by="genre")
    assert both == {a: index.stats("ns", a, {"year": {"$lt": 2000}}, by="genre") for a in ("price", "year")}
    # more groups than max_groups: a ValueError naming it; exactly as many: fine
    distinct = len(index.stats("ns", "price", by="year")["groups"])
    assert len(index.stats("ns", "price", by="year", max_groups=distinct)["groups"]) == distinct
    with pytest.raises(ValueError, match=f"max_groups={distinct - 1}"):
        index.stats("ns", "price", by="year", max_groups=distinct - 1)
    empty = {"matched": 0, "absent": 0, "count": 0, "min": None, "max": None, "sum": 0, "mean": None}
    assert index.stats("other", "price") == empty == index.stats("ns", "price", {"genre": "zydeco"})
    assert index.stats("other", "price", by="genre") == {"groups": [], "matched": 0, "by_absent": 0}
    assert index.stats("other", ["price", "year"]) == {"price": empty, "year": empty}


def test_query_processor_predicate_path_agrees_with_the_dict_path():
    rng = np.random.default_rng(5)
    qp = QueryProcessor(InMemoryStorage(), Index(space="l2", engine_factory=S.StatsOracleEngine, attributes=SCHEMA))
    vecs = [Vector(values=rng.standard_normal(4).astype(np.float32), metadata=m) for m in random_metadata(rng, 500)]
    qp.upsert_many(vecs, "ns")
    stored = list(qp._storage.namespace_map["ns"])  # the stored vectors carry the ids minted at upsert
    assert len(qp.delete([v.id for v in stored[::11]], "ns")) == len(stored[::11])
    assert qp.stats("price", namespace="ns")["matched"] == len(stored) - len(stored[::11])
    for f in [None] + [random_filter(rng) for _ in range(25)]:
        pred = (lambda m: True) if f is None else (lambda m, f=f: py_match(f, m))
        for attr in ("price", "year", "in_stock"):
            assert qp.stats(attr, where=pred, namespace="ns") == qp.stats(attr, where=f, namespace="ns"), (f, attr)
            for by in ("genre", "year", "in_stock"):
                assert qp.stats(attr, where=pred, namespace="ns", by=by) == qp.stats(attr, where=f, namespace="ns", by=by), \
                    (f, attr, by)
        assert qp.stats(["price", "year"], where=pred, namespace="ns", by="genre") == \
            qp.stats(["price", "year"], where=f, namespace="ns", by="genre")
    with pytest.raises(ValueError, match="max_groups=3"):
        qp.stats("price", where=lambda m: True, namespace="ns", by="year", max_groups=3)
    assert qp.stats("price", namespace="nowhere") == qp.stats("price", where=lambda m: True, namespace="nowhere")
    assert qp.stats("price", namespace="nowhere", by="genre") == \
        qp.stats("price", where=lambda m: True, namespace="nowhere", by="genre") == {"groups": [], "matched": 0, "by_absent": 0}


# ---------------------------------------------------------------- the fixed-point rule itself
def _rule_inputs():
    rng = np.random.default_rng(11)
    return {
        "normal": rng.standard_normal(5000),
        "cents": np.round(rng.uniform(0, 1000, 5000), 2),
        "decades": rng.standard_normal(3000) * 10.0 ** rng.integers(-30, 30, 3000),
        "subnormal": rng.integers(-2 ** 40, 2 ** 40, 2000) * 5e-324,
    }


@pytest.mark.parametrize("name", ["normal", "cents", "decades", "subnormal"])
def test_the_model_meets_fsum_within_the_bound_of_the_header(name):
    v = _rule_inputs()[name]
    got, true = S.float_sum_model(v), math.fsum(v.tolist())
    S_fixed, E = S.fixed_sum(v)
    assert E == math.floor(math.log2(np.abs(v).max())) if name != "subnormal" else E < -1022
    bound = v.size * math.ldexp(1.0, E - 62) + math.ulp(true)  # count * 2^(E - 62) plus the final rounding
    print(f"{name}: model {got!r}, fsum {true!r}, |diff| {abs(got - true)!r}, bound {bound!r}")
    assert abs(got - true) <= bound
    # the package's host path is the same function of the values, bit for bit, in any order
    count, lo, hi, fixed = host_stats.float_group(v[::-1].tolist())
    assert (count, fixed) == (v.size, S_fixed) and host_stats.float_sum(fixed, lo, hi).hex() == got.hex()


def test_a_sum_beyond_the_largest_double_is_an_infinity_with_finite_min_and_max():
    v = np.full(1000, 1.7e308)
    assert S.float_sum_model(v) == math.inf and S.float_sum_model(-v) == -math.inf
    count, lo, hi, fixed = host_stats.float_group(v.tolist())
    assert (lo, hi) == (1.7e308, 1.7e308) and host_stats.float_sum(fixed, lo, hi) == math.inf
    assert host_stats.float_sum(-fixed, -hi, -lo) == -math.inf
    assert S.float_sum_model([1.7e308, -1.7e308, 1.0]) == 0.0  # (1.0 is far below half a unit of the scale)


def test_the_sum_is_correctly_rounded_within_a_factor_two_to_the_nine_of_the_largest_value():
    rng = np.random.default_rng(12)
    for trial in range(50):
        m = float(rng.uniform(1, 2) * 2.0 ** rng.integers(-1000, 1000))
        v = rng.uniform(-1, 1, 2000) * m
        v = np.where(np.abs(v) < m / 512, m / 512 * np.sign(v + (v == 0)), v)
        v[0] = m
        assert np.abs(v).min() * 512 >= np.abs(v).max()
        assert S.float_sum_model(v).hex() == math.fsum(v.tolist()).hex()
        count, lo, hi, fixed = host_stats.float_group(v.tolist())
        assert host_stats.float_sum(fixed, lo, hi).hex() == math.fsum(v.tolist()).hex()


def test_half_way_terms_round_to_even_and_powers_of_two_pick_their_own_exponent():
    m = 2.0 ** 61  # E = 61: a term is rint(v) itself
    for v, term in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (0.75, 1), (3.0, 3)):
        fixed, E = S.fixed_sum(np.array([m, v]))
        assert E == 61 and fixed - 2 ** 61 == term == host_stats.fixed_term(v, 61)
    for m in (1.0, 2.0 ** -1022, 2.0 ** 1023, 5e-324, 2.0 ** -1060):  # m = 2^E exactly: the term of m is 2^61
        E = round(math.log2(m)) if m > 5e-324 else -1074
        assert S.fixed_sum(np.array([m])) == (2 ** 61, E) and host_stats.fixed_exponent(-m, m) == E
        below = math.nextafter(m, 0.0)  # one ulp below: the exponent drops by one, the term nearly doubles
        if below > 0:
            fixed, Eb = S.fixed_sum(np.array([below]))
            assert Eb == E - 1 and 2 ** 61 < fixed < 2 ** 62 and host_stats.fixed_exponent(below, below) == Eb
            assert host_stats.float_sum(fixed, below, below) == below == S.float_sum_model([below])
        assert S.float_sum_model([m, m]) == 2 * m if m < 2.0 ** 1023 else S.float_sum_model([m, m]) == math.inf
    # infinities, signed zeros and NaN
    assert math.isnan(S.float_sum_model([math.inf, -math.inf, 1.0])) and S.float_sum_model([1.0, math.inf]) == math.inf
    assert S.float_sum_model([-math.inf, 5.0]) == -math.inf and S.fixed_sum(np.array([math.inf, 3.0])) == (0, None)
    assert host_stats.float_group([0.0, -0.0, math.nan])[:3] == (2, -0.0, 0.0)
    assert math.copysign(1, host_stats.float_group([0.0, -0.0])[1]) == -1 and S.float_sum_model([0.0, -0.0]) == 0.0
    assert math.isnan(host_stats.float_sum(0, -math.inf, math.inf)) and host_stats.float_sum(0, 1.0, math.inf) == math.inf
    assert host_stats.int128(*host_stats.split128(-(2 ** 100) - 7)) == -(2 ** 100) - 7
