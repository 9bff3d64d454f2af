"""Grouped kNN (include/mlvdb_grouped.h) without a GPU: the NumPy oracle against the definition, the Index surface of
``search_many(distinct=..., group_size=...)`` over an oracle engine, its refusals, ``QueryProcessor.find_similar_many`` on
top, the mirrored host rules of the member stage and the C ABI's shape."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import GroupedBatchHits, Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from oracle import exact_scan
from tests.distinct_helpers import ABSENT
from tests.grouped_helpers import (GroupedOracleEngine, chunk_rows, grouped_knn, grouped_knn_brute, oracle_index, table_slots,
                                   tile_plan)
from tests.where_helpers import WhereOracleEngine

ROOT = Path(__file__).resolve().parents[1]
SCHEMA = {"doc": "int", "genre": "str", "flag": "bool", "price": "float"}
GENRES = ["jazz", "rock", "folk"]


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_oracle_equals_the_per_group_definition(space):
    rng = np.random.default_rng(3)
    n, d, nq = 300, 6, 5
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
    for k, g in ((1, 1), (3, 2), (24, 5), (64, 64)):
        lab, d64, cnt, gcnt, grp = grouped_knn(dist, groups, allowed, k, g)
        want = grouped_knn_brute(dist, groups, allowed, k, g)
        for i in range(nq):
            assert cnt[i] == len(want[i])
            for j, (code, rows_) in enumerate(want[i]):
                c = gcnt[i, j]
                assert grp[i, j] == code and c == len(rows_) == min(g, int((allowed & (groups == code)).sum()))
                assert lab[i, j, :c].tolist() == [r for _, r in rows_] and d64[i, j, :c].tolist() == [dd for dd, _ in rows_]
                assert (lab[i, j, c:] == -1).all() and np.isinf(d64[i, j, c:]).all()
            assert (lab[i, cnt[i]:] == -1).all() and (gcnt[i, cnt[i]:] == 0).all() and (grp[i, cnt[i]:] == ABSENT).all()


def test_the_mirrored_host_rules():
    assert [table_slots(u) for u in (0, 1, 2, 3, 4, 5, 1000)] == [2, 2, 4, 8, 8, 16, 2048]
    assert chunk_rows(0) == 256 and chunk_rows(2048 * 256) == 256 and chunk_rows(2048 * 256 + 1) == 320
    assert chunk_rows(10_000_000) == 4928
    grp = np.array([[7, 3], [7, 3], [7, ABSENT], [7, ABSENT], [7, ABSENT]], np.int64)
    rows, tiles = tile_plan(grp, np.array([2, 2, 1, 1, 1]), {7: 1000, 3: 10})
    assert rows == 256 and tiles == [(3, 2, 1), (7, 4, 4), (7, 1, 4)]


# ---------------------------------------------------------------- Index over the oracle engine
class UntouchableEngine(WhereOracleEngine):
    """Fails the test if a search of any kind reaches the engine."""

    def search(self, *a, **kw):
        raise AssertionError("the engine was touched")

    search64 = search_distinct = search_grouped = search_each = search_mmr = search


def _filled(factory=GroupedOracleEngine, n=300, d=8, seed=1, **kw):
    rng = np.random.default_rng(seed)
    index = Index(space="l2", engine_factory=factory, attributes=SCHEMA, **kw)
    metas = []
    for i in range(n):
        m = {"doc": int(rng.integers(0, 40)), "genre": GENRES[i % 3], "flag": bool(i % 2), "price": float(i)}
        if rng.random() < 0.15:
            del m["doc"]
        metas.append(m)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs, "ns")
    return rng, index, vecs, rows, metas


def _flat(lab, gcnt, i):
    return [int(x) for j in range(lab.shape[1]) for x in lab[i, j, :gcnt[i, j]]]


def test_index_grouped_flat_order_counts_sizes_and_values():
    rng, index, vecs, rows, metas = _filled()
    qs = rng.standard_normal((5, 8)).astype(np.float32)
    dist = exact_scan.exact_distances(qs, rows, "l2")
    doc = np.array([m.get("doc", ABSENT) for m in metas], dtype=np.int64)
    for where, allowed in ((None, np.ones(len(metas), bool)), ({"flag": True}, np.array([m["flag"] for m in metas]))):
        got = index.search_many(qs, 10, "ns", "l2", distinct="doc", where=where, group_size=3)
        assert isinstance(got, GroupedBatchHits) and got.labels.shape == (5, 30)
        lab, d64, cnt, gcnt, grp = grouped_knn(dist, doc, allowed, 10, 3)
        assert np.array_equal(got.group_sizes, gcnt) and got.group_sizes.dtype == np.int32
        assert np.array_equal(got.counts, gcnt.sum(axis=1)) and got.counts.dtype == np.int32
        for i, hits in enumerate(got):
            flat = _flat(lab, gcnt, i)
            assert got.labels[i, :len(flat)].tolist() == flat and (got.labels[i, len(flat):] == -1).all()
            assert [h.vector_id for h in hits] == [vecs[j].id for j in flat]
            assert [h.score for h in hits] == [float(np.float32(dist[i, j])) for j in flat]
            assert got.group_values[i, :cnt[i]].tolist() == grp[i, :cnt[i]].tolist()
            assert all(type(v) is int for v in got.group_values[i, :cnt[i]]) and (got.group_values[i, cnt[i]:] == None).all()  # noqa: E711
    # str through the dictionary, bool as bool
    got = index.search_many(qs, 10, "ns", "l2", distinct="genre", group_size=2)
    assert got.counts.tolist() == [6] * 5 and got.group_sizes[:, :3].tolist() == [[2, 2, 2]] * 5
    for i in range(5):
        assert sorted(got.group_values[i, :3].tolist()) == sorted(GENRES) and got.group_values[i, 3:].tolist() == [None] * 7
        split = np.split(got.labels[i, :6], np.cumsum(got.group_sizes[i, :3])[:-1])
        for value, members in zip(got.group_values[i, :3], split):
            assert all(metas[j]["genre"] == value for j in members)
    got = index.search_many(qs, 10, "ns", "l2", distinct="flag", group_size=64)
    assert got.counts.tolist() == [128] * 5
    assert all(sorted(got.group_values[i, :2].tolist()) == [False, True] and type(got.group_values[i, 0]) is bool for i in range(5))


def test_group_size_one_is_the_distinct_result_and_none_is_untouched():
    rng, index, _, _, _ = _filled()
    qs = rng.standard_normal((4, 8)).astype(np.float32)
    one = index.search_many(qs, 7, "ns", "l2", distinct="doc", group_size=1)
    plain = index.search_many(qs, 7, "ns", "l2", distinct="doc")
    assert type(plain).__name__ == "BatchHits" and not hasattr(plain, "group_sizes")
    assert np.array_equal(one.labels, plain.labels) and np.array_equal(one.scores, plain.scores)
    assert np.array_equal(one.counts, plain.counts) and one == plain
    same = index.search_many(qs, 7, "ns", "l2", distinct="doc", group_size=None)
    assert type(same).__name__ == "BatchHits" and np.array_equal(same.labels, plain.labels)


def test_grouped_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, _, _, _ = _filled(UntouchableEngine)
    qs = np.zeros((3, 8), np.float32)
    with pytest.raises(ValueError, match="group_size is the member count of distinct"):
        index.search_many(qs, 5, "ns", "l2", group_size=3)
    for bad in (0, 65, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match=r"group_size must be an int in \[1, 64\]"):
            index.search_many(qs, 5, "ns", "l2", distinct="doc", group_size=bad)
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.search_many(qs, 5, "ns", "l2", distinct="author", group_size=3)
    with pytest.raises(ValueError, match="float column"):
        index.search_many(qs, 5, "ns", "l2", distinct="price", group_size=3)
    with pytest.raises(ValueError, match="top_k must be <= 64"):
        index.search_many(qs, 65, "ns", "l2", distinct="doc", group_size=3)
    with pytest.raises(ValueError, match="per-query where list"):
        index.search_many(qs, 5, "ns", "l2", distinct="doc", group_size=3, where=[None, {"doc": 1}, None])
    with pytest.raises(ValueError, match="allowed_ids is not supported"):
        index.search_many(qs, 5, "ns", "l2", distinct="doc", group_size=3, allowed_ids=[])
    with pytest.raises(ValueError, match="distinct= cannot be combined"):
        index.search_many(qs, 5, "ns", "l2", distinct="doc", group_size=3, mmr_lambda=0.5)
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="group_size is the member count of distinct"):
        qp.find_similar_many(qs, 5, "ns", group_size=3)
    with pytest.raises(ValueError, match="one dict filter"):
        qp.find_similar_many(qs, 5, "ns", distinct="doc", group_size=3, where=lambda m: True)
    with pytest.raises(ValueError, match=r"group_size must be an int in \[1, 64\]"):
        qp.find_similar_many(qs, 5, "ns", distinct="doc", group_size=100)
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    with pytest.raises(ValueError, match="row-sharded"):
        sharded.search_many(np.zeros((1, 4), np.float32), 3, "ns", "l2", distinct="doc", group_size=3)


def test_empty_namespace_and_a_str_attribute_never_stored():
    _, index, _, _, _ = _filled()
    qs = np.zeros((3, 8), np.float32)
    got = index.search_many(qs, 5, "other", "l2", distinct="doc", group_size=3)
    assert isinstance(got, GroupedBatchHits) and len(got) == 3 and got.counts.tolist() == [0, 0, 0]
    assert got.group_sizes.shape == (3, 0) and got.group_values.shape == (3, 0) and [list(h) for h in got] == [[], [], []]
    index2 = Index(space="l2", engine_factory=GroupedOracleEngine, attributes={"tag": "str", "doc": "int"})
    index2.add([Vector(values=np.ones(4, np.float32) * i, metadata={"doc": i}) for i in range(6)], "ns")
    got = index2.search_many(np.zeros((2, 4), np.float32), 4, "ns", "l2", distinct="tag", group_size=3)
    assert got.counts.tolist() == [0, 0] and got.labels.shape == (2, 12) and (got.labels == -1).all()
    assert got.group_sizes.tolist() == [[0] * 4] * 2 and (got.group_values == None).all() and got[0] == []  # noqa: E711


def test_query_processor_grouped_order_and_dict_shape():
    rng = np.random.default_rng(4)
    index = oracle_index({"doc": "int", "even": "bool"}, space="cosine")
    qp = QueryProcessor(InMemoryStorage(), index)
    qp.upsert_many([VectorDTO(values=rng.standard_normal(6).tolist(), metadata={"doc": int(i % 9), "even": i % 2 == 0, "chunk": i})
                    for i in range(120)], "ns")
    qs = rng.standard_normal((4, 6)).astype(np.float32)
    for where in (None, {"even": True}):
        out = qp.find_similar_many(qs, 5, "ns", distinct="doc", group_size=3, where=where)
        bh = index.search_many(qs, 5, "ns", "cosine", distinct="doc", group_size=3, where=where)
        assert len(out) == 4
        for i, hits in enumerate(out):
            assert len(hits) == 15 == int(bh.counts[i]) and bh.group_sizes[i].tolist() == [3] * 5
            assert [h["id"] for h in hits] == [r.vector_id for r in bh[i]]
            assert all(set(h) == {"id", "values", "metadata", "score"} for h in hits)
            docs = [h["metadata"]["doc"] for h in hits]
            assert docs == [v for v in bh.group_values[i].tolist() for _ in range(3)] and len(set(docs)) == 5
            for j in range(5):  # members in order inside a group, groups by their first member
                s = [h["score"] for h in hits[3 * j:3 * j + 3]]
                assert s == sorted(s, reverse=True)
            firsts = [hits[3 * j]["score"] for j in range(5)]
            assert firsts == sorted(firsts, reverse=True)
            if where:
                assert all(h["metadata"]["even"] for h in hits)


# ---------------------------------------------------------------- C ABI
def test_grouped_header_declares_what_the_binding_binds():
    lib = _native.load()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_grouped.h").read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))
    assert names == ["mlvdb_search_batch_grouped"] == sorted(_native.GROUPED_SIGNATURES)
    assert hasattr(lib, names[0]) and names[0] not in _native.SIGNATURES
    params = re.search(r"mlvdb_search_batch_grouped\((.*?)\);", text, flags=re.S).group(1).split(",")
    assert len(params) == len(_native.GROUPED_SIGNATURES[names[0]][1]) == 14
    assert int(re.search(r"#define\s+MLVDB_GROUPED_MAX_SIZE\s+(\d+)", text).group(1)) == _native.GROUPED_MAX_SIZE == 64
    assert lib.mlvdb_abi_version() == 7


def test_grouped_entry_refuses_a_null_handle_inside_the_exception_guard():
    lib = _native.load()
    buf = (C.c_float * 4)()
    assert lib.mlvdb_search_batch_grouped(C.c_void_p(), buf, 1, 1, 1, 0, 0, None, buf, buf, buf, buf, buf, buf) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    body = re.search(r"^int mlvdb_search_batch_grouped\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
    assert body.lstrip().startswith("return guarded(")
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_grouped\.hip\b", make, flags=re.M) and "mlvdb_grouped.h" in make
