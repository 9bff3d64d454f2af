"""Distinct-by-attribute kNN (include/mlvdb_distinct.h) without a GPU: the NumPy oracle against the definition, the refusals
of ``Index.search_many(distinct=...)`` / ``QueryProcessor.find_similar_many(distinct=...)``, the Index surface over an
oracle engine, and the C ABI's shape."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from oracle import exact_scan
from tests.distinct_helpers import (ABSENT, DistinctOracleEngine, distinct_knn, distinct_knn_brute,
                                    group_spans_blocks_and_waves, oracle_index, scan_geometry)
from tests.where_helpers import WhereOracleEngine

ROOT = Path(__file__).resolve().parents[1]
SCHEMA = {"doc": "int", "genre": "str", "flag": "bool", "price": "float"}


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_oracle_equals_the_per_group_definition(space):
    rng = np.random.default_rng(3)
    n, d, nq = 400, 6, 7
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows[200:220] = rows[10:30]  # exact duplicates: within a group and across groups
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    groups = rng.integers(0, 25, n).astype(np.int64)
    groups[200:210] = groups[10:20]
    groups[rng.random(n) < 0.15] = ABSENT
    groups[5] = ABSENT + 1
    groups[6] = np.iinfo(np.int64).max
    allowed = rng.random(n) > 0.1
    dist = exact_scan.exact_distances(qs, rows, space)
    for k in (1, 3, 24, 64):
        lab, d64, cnt, grp = distinct_knn(dist, groups, allowed, k)
        want = distinct_knn_brute(dist, groups, allowed, k)
        for i in range(nq):
            assert cnt[i] == len(want[i]) == min(k, np.unique(groups[allowed & (groups != ABSENT)]).size)
            assert lab[i, :cnt[i]].tolist() == [row for _, row, _ in want[i]]
            assert grp[i, :cnt[i]].tolist() == [g for _, _, g in want[i]]
            assert d64[i, :cnt[i]].tolist() == [dd for dd, _, _ in want[i]]
            assert (lab[i, cnt[i]:] == -1).all() and np.isinf(d64[i, cnt[i]:]).all() and (grp[i, cnt[i]:] == ABSENT).all()
            assert np.unique(grp[i, :cnt[i]]).size == cnt[i]


def test_scan_geometry_helper_states_where_a_groups_rows_are_scanned():
    assert scan_geometry(40_000, 64, 70) == (8, 2, 8, 113)
    assert scan_geometry(40_000, 64, 1) == (1, 2, 16, 79)
    assert scan_geometry(17, 3, 9) == (8, 2, 8, 1)
    groups = np.random.default_rng(0).integers(0, 200, 40_000)
    assert group_spans_blocks_and_waves(groups, np.ones(40_000, bool), scan_geometry(40_000, 64, 70))
    assert not group_spans_blocks_and_waves(np.arange(64, dtype=np.int64), np.ones(64, bool), scan_geometry(64, 64, 9))


# ---------------------------------------------------------------- refusals, before the engine is touched
class UntouchableEngine(WhereOracleEngine):
    """Fails the test if a search of any kind reaches the engine."""

    def search(self, *a, **kw):
        raise AssertionError("the engine was touched")

    search64 = search_distinct = search_each = search


def _filled(factory=DistinctOracleEngine, n=300, d=8, seed=1, **kw):
    rng = np.random.default_rng(seed)
    index = Index(space="l2", engine_factory=factory, attributes=SCHEMA, **kw)
    metas = []
    for i in range(n):
        m = {"doc": int(rng.integers(0, 40)), "genre": ["jazz", "rock", "folk"][i % 3], "flag": bool(i % 2),
             "price": float(i)}
        if rng.random() < 0.15:
            del m["doc"]
        metas.append(m)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs, "ns")
    return rng, index, vecs, rows, metas


def test_distinct_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, _, _, _ = _filled(UntouchableEngine)
    qs = np.zeros((3, 8), np.float32)
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.search_many(qs, 5, "ns", "l2", distinct="author")
    with pytest.raises(ValueError, match="float column"):
        index.search_many(qs, 5, "ns", "l2", distinct="price")
    with pytest.raises(ValueError, match="top_k must be <= 64"):
        index.search_many(qs, 65, "ns", "l2", distinct="doc")
    with pytest.raises(ValueError, match="per-query where list"):
        index.search_many(qs, 5, "ns", "l2", distinct="doc", where=[None, {"doc": 1}, None])
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.search_many(qs, 5, "ns", "l2", distinct="doc", where={"nope": 1})
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="one dict filter"):
        qp.find_similar_many(qs, 5, "ns", distinct="doc", where=lambda m: True)
    with pytest.raises(ValueError, match="top_k must be <= 64"):
        qp.find_similar_many(qs, 100, "ns", distinct="doc")


def test_distinct_on_a_row_sharded_index_is_refused():
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    with pytest.raises(ValueError, match="row-sharded"):
        sharded.search_many(np.zeros((1, 4), np.float32), 3, "ns", "l2", distinct="doc")


# ---------------------------------------------------------------- Index / QueryProcessor over the oracle engine
def test_index_distinct_returns_one_hit_per_value_and_follows_where():
    rng, index, vecs, rows, metas = _filled()
    qs = rng.standard_normal((5, 8)).astype(np.float32)
    dist = exact_scan.exact_distances(qs, rows, "l2")
    doc = np.array([m.get("doc", ABSENT) for m in metas], dtype=np.int64)
    for where, allowed in ((None, np.ones(len(metas), bool)),
                           ({"flag": True}, np.array([m["flag"] for m in metas]))):
        got = index.search_many(qs, 10, "ns", "l2", distinct="doc", where=where)
        lab, _, cnt, _ = distinct_knn(dist, doc, allowed, 10)
        assert np.array_equal(got.labels, lab) and np.array_equal(got.counts, cnt)
        for i, hits in enumerate(got):
            assert [h.vector_id for h in hits] == [vecs[j].id for j in lab[i, :cnt[i]]]
    # a str column: the dictionary bounds the groups; a bool column: two
    got = index.search_many(qs, 10, "ns", "l2", distinct="genre")
    assert got.counts.tolist() == [3] * 5
    got = index.search_many(qs, 10, "ns", "l2", distinct="flag")
    assert got.counts.tolist() == [2] * 5
    # without distinct= nothing changed
    plain = index.search_many(qs, 10, "ns", "l2")
    assert plain.counts.tolist() == [10] * 5
    assert len(index.search_many(qs, 10, "other", "l2", distinct="doc")) == 5


def test_query_processor_distinct_returns_pairwise_different_values():
    rng = np.random.default_rng(4)
    qp = QueryProcessor(InMemoryStorage(), oracle_index({"doc": "int"}, space="cosine"))
    qp.upsert_many([VectorDTO(values=rng.standard_normal(6).tolist(), metadata={"doc": int(i % 9)}) for i in range(120)], "ns")
    out = qp.find_similar_many(rng.standard_normal((4, 6)), 5, "ns", distinct="doc")
    for hits in out:
        docs = [h["metadata"]["doc"] for h in hits]
        assert len(docs) == 5 == len(set(docs))
        assert [h["score"] for h in hits] == sorted((h["score"] for h in hits), reverse=True)


# ---------------------------------------------------------------- C ABI
def _header_functions():
    text = (ROOT / "include" / "mlvdb_distinct.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))


def test_distinct_header_declares_what_the_binding_binds():
    lib = _native.load()
    names = _header_functions()
    assert names == ["mlvdb_search_batch_distinct"] == sorted(_native.DISTINCT_SIGNATURES)
    assert hasattr(lib, names[0])
    known = set(_native.SIGNATURES) | set(_native.WHERE_SIGNATURES) | set(_native.WHERE_EACH_SIGNATURES)
    assert not set(names) & known
    text = (ROOT / "include" / "mlvdb_distinct.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    params = re.search(r"mlvdb_search_batch_distinct\((.*?)\);", text, flags=re.S).group(1).split(",")
    assert len(params) == len(_native.DISTINCT_SIGNATURES[names[0]][1]) == 12
    assert lib.mlvdb_abi_version() == 7


def test_distinct_entry_refuses_a_null_handle_inside_the_exception_guard():
    lib = _native.load()
    buf = (C.c_float * 4)()
    assert lib.mlvdb_search_batch_distinct(C.c_void_p(), buf, 1, 1, 0, 0, None, buf, buf, buf, buf, buf) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    body = re.search(r"^int mlvdb_search_batch_distinct\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
    assert body.lstrip().startswith("return guarded(")


def test_the_distinct_kernels_header_and_tuning_key_are_in_the_build():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_distinct\.hip\b", make, flags=re.M)
    assert "mlvdb_distinct.h" in make and "wave_topk_distinct.h" in make
    internal = (ROOT / "mlvectordb_amd" / "csrc" / "internal.h").read_text()
    assert re.search(r'X\(distinct_oversample, "DISTINCT_OVERSAMPLE", 4\)', internal)
