"""Per-query metadata filters (include/mlvdb_where_each.h) without a GPU: the C ABI's shape, the dedupe / chunking helpers
of where.py, and Index / QueryProcessor on an oracle engine that answers every query under its own program."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from mlvectordb_amd import where as W
from tests.where_helpers import SCHEMA, EachOracleEngine, py_match, random_filter, random_metadata

ROOT = Path(__file__).resolve().parents[1]


def each_header_functions():
    text = (ROOT / "include" / "mlvdb_where_each.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))


def eidx(space="l2", **kw):
    return Index(space=space, engine_factory=EachOracleEngine, attributes=SCHEMA, **kw)


def hits(bh):
    return [[(h.vector_id, h.score) for h in row] for row in bh]


# ---------------------------------------------------------------- C ABI
def test_each_header_symbols_are_exported_and_bound():
    lib = _native.load()
    names = each_header_functions()
    assert names == ["mlvdb_search_batch_where_each", "mlvdb_where_count_each"]
    assert sorted(_native.WHERE_EACH_SIGNATURES) == names
    for name in names:
        assert hasattr(lib, name), name
    assert not set(names) & (set(_native.SIGNATURES) | set(_native.WHERE_SIGNATURES))
    text = (ROOT / "include" / "mlvdb_where_each.h").read_text()
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert int(consts["MLVDB_WHERE_EACH_MAX_PROGRAMS"]) == _native.WHERE_EACH_MAX_PROGRAMS == W.EACH_MAX_PROGRAMS == 64
    assert int(consts["MLVDB_WHERE_EACH_MAX_OPS"]) == _native.WHERE_EACH_MAX_OPS == W.EACH_MAX_OPS == 1024
    assert [int(consts[f"MLVDB_WHERE_ROUTE_{r}"]) for r in ("NONE", "SCAN", "GATHER")] == \
        [_native.ROUTE_NONE, _native.ROUTE_SCAN, _native.ROUTE_GATHER]


def test_every_each_entry_refuses_a_null_handle_with_a_status_code():
    lib = _native.load()
    null = C.c_void_p()
    buf = (C.c_float * 4)()
    w = (_native.Where * 1)()
    calls = {
        "mlvdb_search_batch_where_each": (null, buf, 1, 1, w, 1, buf, buf, buf, buf, buf, buf),
        "mlvdb_where_count_each": (null, w, 1, buf),
    }
    assert sorted(calls) == sorted(_native.WHERE_EACH_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 1, name  # MLVDB_ERR_INVALID_ARG
        assert b"null index handle" in lib.mlvdb_last_global_error(), name


def test_every_each_entry_runs_inside_the_exception_guard():
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    region = text[text.index('extern "C" {'):text.index('}  // extern "C"')]
    bodies = dict(re.findall(r"^int (mlvdb_\w+)\([^)]*\) \{\n(.*?)^\}", region, flags=re.S | re.M))
    for name in each_header_functions():
        assert name in bodies, name
        assert bodies[name].lstrip().startswith("return guarded("), f"{name} is not wrapped by guarded()"


def test_the_each_kernels_and_header_are_in_the_build():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_where_each\.hip\b", make, flags=re.M)
    assert "mlvdb_where_each.h" in make
    internal = (ROOT / "mlvectordb_amd" / "csrc" / "internal.h").read_text()
    assert re.search(r'X\(where_gather, "WHERE_GATHER", \d+\)', internal)


# ---------------------------------------------------------------- dedupe and chunking
def test_compile_each_dedupes_identical_programs():
    strings = {"genre": {"jazz": 0, "blues": 1}}
    wheres = [{"year": 1990}, None, {"genre": "jazz"}, {"year": 1990}, {"genre": {"$in": ["jazz"]}}, None,
              {"genre": "jazz"}, {}]
    programs, of = W.compile_each(wheres, SCHEMA, strings)
    assert of.dtype == np.int32 and of.tolist() == [0, -1, 1, 0, 2, -1, 1, 3]
    assert len(programs) == 4
    for w, j in zip(wheres, of.tolist()):
        if w is not None:
            want = W.compile_where(w, SCHEMA, strings)
            assert programs[j].ops.tobytes() == want.ops.tobytes() and np.array_equal(programs[j].set, want.set)
    # same ops, different set contents: two programs
    p2, of2 = W.compile_each([{"year": {"$in": [1, 2]}}, {"year": {"$in": [1, 3]}}], SCHEMA)
    assert len(p2) == 2 and of2.tolist() == [0, 1]
    assert W.compile_each([None, None], SCHEMA)[0] == []


def test_chunking_respects_both_limits_and_covers_every_query():
    wheres = [None if i % 7 == 0 else {"year": int(i % 150)} for i in range(400)]  # 130 distinct one-op programs
    programs, of = W.compile_each(wheres, SCHEMA)
    assert len(programs) > 64
    chunks = W.chunk_programs(programs, of)
    assert len(chunks) == 3
    seen = np.zeros(len(wheres), int)
    for c, (idx, progs, local) in enumerate(chunks):
        assert 1 <= len(progs) <= 64 and sum(p.ops.size for p in progs) <= 1024
        assert np.all(np.diff(idx) > 0) and local.shape == idx.shape
        seen[idx] += 1
        for i, j in zip(idx.tolist(), local.tolist()):
            if of[i] < 0:
                assert j == -1 and c == 0
            else:
                assert progs[j] is programs[of[i]]
    assert np.all(seen == 1)
    # op-limited: programs of 17 ops each -> 60 per call (1024 // 17)
    big = [{"$or": [{"year": int(y)} for y in range(8)] + [{"price": float(i)}]} for i in range(100)]
    programs, of = W.compile_each(big, SCHEMA)
    n_ops = programs[0].ops.size
    assert n_ops > 16
    chunks = W.chunk_programs(programs, of)
    assert all(sum(p.ops.size for p in progs) <= 1024 for _, progs, _ in chunks)
    assert max(len(progs) for _, progs, _ in chunks) == 1024 // n_ops
    assert sum(len(progs) for _, progs, _ in chunks) == 100
    # tight limits, and only unfiltered queries
    chunks = W.chunk_programs(programs[:5], np.array([4, 3, 2, 1, 0, -1], np.int32), max_programs=2)
    assert [len(p) for _, p, _ in chunks] == [2, 2, 1]
    assert chunks[0][0].tolist() == [3, 4, 5] and chunks[0][2].tolist() == [1, 0, -1]
    only = W.chunk_programs([], np.array([-1, -1], np.int32))
    assert len(only) == 1 and only[0][0].tolist() == [0, 1] and only[0][1] == []
    with pytest.raises(ValueError, match="at most 4"):
        W.chunk_programs(programs[:1], np.zeros(1, np.int32), max_ops=4)


# ---------------------------------------------------------------- Index over the oracle engine
def _filled(space="l2", seed=11, n=320, d=8):
    rng = np.random.default_rng(seed)
    index = eidx(space=space)
    metas = random_metadata(rng, n)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs[:200], "ns")
    index.add(vecs[200:], "ns")
    gone = [v.id for v in vecs[::9]]
    index.remove(gone, "ns")
    return rng, index, vecs, set(gone)


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_index_per_query_filters_equal_one_single_dict_call_per_query(space):
    rng, index, vecs, gone = _filled(space)
    live = [v for v in vecs if v.id not in gone]
    nq = 24
    qs = rng.standard_normal((nq, 8)).astype(np.float32)
    fs = [random_filter(rng) for _ in range(8)] + [{"genre": "jazz"}, {"genre": "zydeco"}, {}]
    wheres = [None if i % 5 == 0 else fs[int(rng.integers(len(fs)))] for i in range(nq)]
    for k in (1, 7, 400):
        got = index.search_many(qs, k, "ns", space, where=wheres)
        for i, w in enumerate(wheres):
            one = index.search_many(qs[i:i + 1], k, "ns", space, where=w)
            assert hits(got)[i] == hits(one)[0], (i, w)
            n_match = len(live) if w is None else sum(py_match(w, v.metadata) for v in live)
            assert len(hits(got)[i]) == min(k, n_match, len(live))
    assert hits(index.search_many(qs[:3], 5, "ns", space, where=(None, None, None))) == \
        hits(index.search_many(qs[:3], 5, "ns", space))


def test_index_per_query_filters_refusals():
    _, index, _, _ = _filled()
    qs = np.zeros((3, 8), np.float32)
    with pytest.raises(ValueError, match="3 queries"):
        index.search_many(qs, 2, "ns", "l2", where=[{"year": 1}, None])
    with pytest.raises(ValueError, match="not both"):
        index.search_many(qs, 2, "ns", "l2", where=[None, None, None], allowed_ids=[])
    with pytest.raises(ValueError, match="dict filters or None"):
        index.search_many(qs, 2, "ns", "l2", where=[None, lambda m: True, None])
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.search_many(qs, 2, "ns", "l2", where=[None, {"nope": 1}, None])
    assert hits(index.search_many(qs, 2, "other", "l2", where=[None, {"year": 1}, None])) == [[], [], []]


def test_count_many_equals_count():
    rng, index, _, _ = _filled()
    fs = [random_filter(rng) for _ in range(30)] + [{"genre": "jazz"}, {"genre": "jazz"}, {}]
    assert index.count_many("ns", fs) == [index.count("ns", f) for f in fs]
    assert index.count_many("other", fs[:2]) == [0, 0]
    with pytest.raises(ValueError):
        index.count_many("ns", [None])


def test_per_query_filters_follow_appends_tombstones_and_compaction():
    rng, index, vecs, gone = _filled(seed=5)
    qs = rng.standard_normal((6, 8)).astype(np.float32)
    wheres = [{"genre": "blues"}, None, {"year": {"$gte": 1990}}, {"genre": "blues"}, {"in_stock": True}, {}]

    def check():
        got = index.search_many(qs, 5, "ns", "l2", where=wheres)
        for i, w in enumerate(wheres):
            assert hits(got)[i] == hits(index.search_many(qs[i:i + 1], 5, "ns", "l2", where=w))[0]

    check()
    index.remove([v.id for v in vecs[1::4]], "ns")
    check()
    index.compact("ns")
    check()


# ---------------------------------------------------------------- QueryProcessor
def test_query_processor_list_where_and_its_refusal_of_callables():
    rng = np.random.default_rng(9)
    qp = QueryProcessor(InMemoryStorage(), eidx(space="cosine"))
    qp.upsert_many([VectorDTO(values=rng.standard_normal(6).tolist(), metadata=m) for m in random_metadata(rng, 90)], "ns")
    q = rng.standard_normal((4, 6))
    wheres = [{"genre": "jazz"}, None, {"year": {"$lt": 1990}}, {"genre": "jazz"}]
    got = qp.find_similar_many(q, 5, "ns", where=wheres)
    for i, w in enumerate(wheres):
        assert got[i] == qp.find_similar_many(q[i:i + 1], 5, "ns", where=w)[0]
    assert qp.find_similar_many(q, 5, "ns", where=tuple(wheres)) == got
    with pytest.raises(ValueError, match="host path"):
        qp.find_similar_many(q, 5, "ns", where=[None, lambda m: True, None, None])
