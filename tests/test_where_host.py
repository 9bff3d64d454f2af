"""Metadata filters (include/mlvdb_where.h, mlvectordb_amd/where.py) without a GPU: the C ABI's shape, the dict compiler,
and Index / QueryProcessor on an oracle engine that evaluates the compiled programs with NumPy."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, _native
from mlvectordb_amd import where as W
from oracle.engine import OracleScanEngine
from tests.where_helpers import SCHEMA, WhereOracleEngine, py_match, random_filter, random_metadata

ROOT = Path(__file__).resolve().parents[1]


def where_header_functions():
    text = (ROOT / "include" / "mlvdb_where.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))


# ---------------------------------------------------------------- C ABI
def test_where_header_symbols_are_exported_and_bound():
    lib = _native.load()
    names = where_header_functions()
    assert len(names) == 7
    assert sorted(_native.WHERE_SIGNATURES) == names
    for name in names:
        assert hasattr(lib, name), name
    assert not set(names) & set(_native.SIGNATURES)
    text = (ROOT / "include" / "mlvdb_where.h").read_text()
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert int(consts["MLVDB_ATTR_INT64"]) == _native.ATTR_INT64 and int(consts["MLVDB_ATTR_FLOAT64"]) == _native.ATTR_FLOAT64
    ops = ["TRUE", "EQ", "NE", "LT", "LE", "GT", "GE", "IN", "EXISTS", "AND", "OR", "NOT"]
    assert [int(consts[f"MLVDB_WHERE_{o}"]) for o in ops] == [getattr(W, o) for o in ops]
    assert (int(consts["MLVDB_WHERE_MAX_OPS"]), int(consts["MLVDB_WHERE_MAX_DEPTH"]), int(consts["MLVDB_MAX_ATTRS"])) == \
        (W.MAX_OPS, W.MAX_DEPTH, W.MAX_ATTRS)
    assert W.OP_DTYPE.itemsize == 24 and C.sizeof(_native.Where) == 32
    hip = (ROOT / "include" / "mlvdb_hip.h").read_text()
    assert re.search(r"#define\s+MLVDB_ABI_VERSION\s+7\b", hip) and lib.mlvdb_abi_version() == _native.ABI_VERSION == 7


def test_every_where_entry_refuses_a_null_handle_with_a_status_code():
    lib = _native.load()
    null = C.c_void_p()
    z64 = C.c_int64(0)
    buf = (C.c_float * 4)()
    w = _native.Where()
    calls = {
        "mlvdb_attr_define": (null, 0, 1),
        "mlvdb_attr_set": (null, 0, 0, 1, buf),
        "mlvdb_attr_get": (null, 0, 0, 1, buf),
        "mlvdb_where_count": (null, C.byref(w), C.byref(z64)),
        "mlvdb_where_labels": (null, C.byref(w), buf, 1, C.byref(z64)),
        "mlvdb_search_batch_where": (null, buf, 1, 1, C.byref(w), buf, buf, buf, buf),
        "mlvdb_range_batch_packed_where": (null, buf, 1, 1.0, 1, 1, C.byref(w), buf, buf, buf, buf),
    }
    assert sorted(calls) == sorted(_native.WHERE_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 1, name  # MLVDB_ERR_INVALID_ARG
        assert b"null index handle" in lib.mlvdb_last_global_error(), name


def test_every_where_entry_runs_inside_the_exception_guard():
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    region = text[text.index('extern "C" {'):text.index('}  // extern "C"')]
    bodies = dict(re.findall(r"^int (mlvdb_\w+)\([^)]*\) \{\n(.*?)^\}", region, flags=re.S | re.M))
    for name in where_header_functions():
        assert name in bodies, name
        assert bodies[name].lstrip().startswith("return guarded("), f"{name} is not wrapped by guarded()"


def test_the_where_kernel_is_in_the_build():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_where\.hip\b", make, flags=re.M)


# ---------------------------------------------------------------- compiler
def ops_of(where, strings=None):
    return [tuple(r) for r in W.compile_where(where, SCHEMA, strings).ops.tolist()]


STRINGS = {"genre": {"jazz": 0, "blues": 1, "rock": 2}}


def test_compiler_each_operator():
    g, y, p, s = 0, 1, 2, 3
    assert ops_of({}) == [(W.TRUE, 0, 0, 0)]
    assert ops_of({"genre": "jazz"}, STRINGS) == [(W.EQ, g, 0, 0)]
    assert ops_of({"genre": {"$ne": "rock"}}, STRINGS) == [(W.NE, g, 2, 0)]
    assert ops_of({"year": {"$gte": 2000, "$lt": 2010}}) == [(W.GE, y, 2000, 0), (W.LT, y, 2010, 0), (W.AND, 0, 0, 0)]
    assert ops_of({"year": {"$lte": 5}}) == [(W.LE, y, 5, 0)]
    assert ops_of({"year": {"$gt": -5}}) == [(W.GT, y, -5, 0)]
    assert ops_of({"price": {"$lt": 2.5}}) == [(W.LT, p, W.float_bits(2.5), 0)]
    assert ops_of({"price": 3}) == [(W.EQ, p, W.float_bits(3.0), 0)]  # int literal on a float attribute
    assert ops_of({"in_stock": True}) == [(W.EQ, s, 1, 0)]
    assert ops_of({"year": {"$exists": True}}) == [(W.EXISTS, y, 0, 0)]
    assert ops_of({"year": {"$exists": False}}) == [(W.EXISTS, y, 0, 0), (W.NOT, 0, 0, 0)]
    prog = W.compile_where({"year": {"$in": [2001, 1999, 2001]}, "genre": {"$nin": ["rock", "jazz", "zydeco"]}}, SCHEMA,
                           STRINGS)
    assert [tuple(r) for r in prog.ops.tolist()] == [(W.IN, y, 0, 2), (W.IN, g, 2, 2), (W.NOT, 0, 0, 0), (W.AND, 0, 0, 0)]
    assert prog.set.tolist() == [1999, 2001, 0, 2]  # each range sorted, duplicates and unseen strings dropped
    assert ops_of({"price": {"$in": [1.5, 2]}}) == [(W.EQ, p, W.float_bits(1.5), 0), (W.EQ, p, W.float_bits(2.0), 0),
                                                    (W.OR, 0, 0, 0)]


def test_compiler_literals_that_match_nothing():
    false = [(W.TRUE, 0, 0, 0), (W.NOT, 0, 0, 0)]
    assert ops_of({"genre": "zydeco"}, STRINGS) == false  # a string never ingested
    assert ops_of({"genre": {"$ne": "zydeco"}}, STRINGS) == [(W.TRUE, 0, 0, 0)]
    assert ops_of({"genre": {"$in": ["zydeco"]}}, STRINGS) == false
    assert ops_of({"genre": {"$nin": []}}) == false + [(W.NOT, 0, 0, 0)]
    assert ops_of({"price": float("nan")}) == false
    assert ops_of({"year": {"$lt": 2 ** 70}}) == [(W.EXISTS, 1, 0, 0)]
    assert ops_of({"year": {"$gt": 2 ** 70}}) == false
    assert ops_of({"$or": []}) == false
    assert ops_of({"$and": []}) == [(W.TRUE, 0, 0, 0)]


def test_compiler_nesting():
    got = ops_of({"$or": [{"genre": "jazz"}, {"$not": {"year": {"$lt": 1960}}}], "in_stock": False}, STRINGS)
    assert got == [(W.EQ, 0, 0, 0), (W.LT, 1, 1960, 0), (W.NOT, 0, 0, 0), (W.OR, 0, 0, 0), (W.EQ, 3, 0, 0), (W.AND, 0, 0, 0)]


@pytest.mark.parametrize("bad", [
    {"year": 2000.0}, {"year": {"$in": [1, 2.5]}}, {"in_stock": 1.0}, {"price": "cheap"}, {"price": True},
    {"genre": 3}, {"genre": {"$lt": "m"}}, {"genre": {"$gte": "a"}}, {"year": {"$exists": 1}}, {"year": {"$in": 5}},
    {"year": {"$between": [1, 2]}}, {"year": {}}, {"$nor": []}, {"$and": {"year": 1}}, {"year": None},
])
def test_compiler_type_refusals(bad):
    with pytest.raises(ValueError):
        W.compile_where(bad, SCHEMA, STRINGS)


def test_compiler_refuses_undeclared_keys_by_name():
    with pytest.raises(ValueError, match="'colour'"):
        W.compile_where({"$or": [{"year": 1}, {"colour": "red"}]}, SCHEMA)


def test_compiler_size_limits():
    W.compile_where({"$and": [{"year": i} for i in range(32)]}, SCHEMA)  # 63 ops
    with pytest.raises(ValueError, match="ops"):
        W.compile_where({"$and": [{"year": i} for i in range(33)]}, SCHEMA)  # 65 ops
    deep = {"year": 0}
    for i in range(31):
        deep = {"$or": [{"year": i + 1}, deep]}  # right-nested: every level keeps one value on the stack
    W.compile_where(deep, SCHEMA)
    assert max(np.cumsum([1 if o <= W.EXISTS else -1 if o in (W.AND, W.OR) else 0
                          for o in W.compile_where(deep, SCHEMA).ops["op"]])) == 32
    deeper = {"$or": [{"year": 99}, deep]}  # depth 33 needs 33 pushes + 32 combines: over the op limit as well
    with pytest.raises(ValueError):
        W.compile_where(deeper, SCHEMA)


# ---------------------------------------------------------------- Index on the NumPy engine
def widx(space="l2", **kw):
    return Index(space=space, engine_factory=WhereOracleEngine, attributes=SCHEMA, **kw)


def hits(bh):
    return [[(h.vector_id, h.score) for h in row] for row in bh]


def test_fuzz_filters_agree_with_the_dict_semantics_and_the_allowed_ids_path():
    rng = np.random.default_rng(20251015)
    d, n = 8, 300
    index = widx()
    metas = random_metadata(rng, n)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs[:200], "ns")
    index.add(vecs[200:], "ns")
    gone = [v.id for v in vecs[::10]]
    index.remove(gone, "ns")
    live = [v for v in vecs if v.id not in set(gone)]
    qs = rng.standard_normal((5, d)).astype(np.float32)
    seen_sizes = set()
    for _ in range(200):
        f = random_filter(rng)
        want = [v.id for v in live if py_match(f, v.metadata)]
        seen_sizes.add(min(len(want), 1) + (len(want) == len(live)))
        assert index.query_by_metadata("ns", f) == want, f
        assert index.count("ns", f) == len(want), f
        k = int(rng.choice([1, 5, 17]))
        got = index.search_many(qs, k, "ns", "l2", where=f)
        if want:
            assert hits(got) == hits(index.search_many(qs, k, "ns", "l2", allowed_ids=want)), f
        else:
            assert all(len(h) == 0 for h in got), f
    assert seen_sizes == {0, 1, 2}  # filters matching nothing, some rows and every row


def test_range_search_where_equals_a_filtered_range():
    rng = np.random.default_rng(3)
    index = widx()
    metas = random_metadata(rng, 120)
    vecs = [Vector(values=rng.standard_normal(6), metadata=m) for m in metas]
    index.add(vecs, "ns")
    q = rng.standard_normal((3, 6)).astype(np.float32)
    f = {"$or": [{"genre": {"$in": ["jazz", "rock"]}}, {"price": {"$lt": 30}}]}
    keep = {v.id for v in vecs if py_match(f, v.metadata)}
    full = index.range_search_many(q, 8.0, "ns", "l2", max_results=None)
    got = index.range_search_many(q, 8.0, "ns", "l2", max_results=None, where=f)
    assert [[(h.vector_id, h.score) for h in row] for row in got] == \
        [[(h.vector_id, h.score) for h in row if h.vector_id in keep] for row in full]


def test_compact_and_rebuild_keep_attributes_with_their_rows():
    rng = np.random.default_rng(5)
    index = widx()
    metas = random_metadata(rng, 80)
    vecs = [Vector(values=rng.standard_normal(4), metadata=m) for m in metas]
    index.add(vecs, "ns")
    index.remove([v.id for v in vecs[::3]], "ns")
    live = [v for i, v in enumerate(vecs) if i % 3]
    f = {"year": {"$gte": 1990}, "genre": {"$ne": "pop"}}
    want = [v.id for v in live if py_match(f, v.metadata)]
    assert index.compact("ns")
    assert index.query_by_metadata("ns", f) == want
    index.rebuild({"ns": live, "other": vecs[:5]}, "l2")
    assert index.query_by_metadata("ns", f) == want
    assert index.query_by_metadata("other", f) == [v.id for v in vecs[:5] if py_match(f, v.metadata)]


def test_a_refused_batch_leaves_the_namespace_unchanged():
    rng = np.random.default_rng(1)
    index = widx()
    vecs = [Vector(values=rng.standard_normal(4), metadata={"genre": "jazz", "year": 2000}) for _ in range(5)]
    index.add(vecs, "ns")
    before = (index.namespace_counts("ns"), index.query_by_metadata("ns", {}), dict(index._ns["ns"].strings["genre"]))
    for bad in ({"genre": "blues", "year": 2001.5}, {"genre": 7}, {"in_stock": 1}, {"price": "x"},
                {"year": np.iinfo(np.int64).min}):
        batch = [Vector(values=rng.standard_normal(4), metadata={"genre": "blues"}),
                 Vector(values=rng.standard_normal(4), metadata=bad)]
        with pytest.raises(ValueError):
            index.add(batch, "ns")
        with pytest.raises(ValueError):
            index.add(batch, "fresh")
    with pytest.raises(ValueError):
        index.add_arrays(rng.standard_normal((2, 4)), "ns", attributes={"year": np.array([1.5, 2.0])})
    with pytest.raises(ValueError):
        index.add_arrays(rng.standard_normal((2, 4)), "ns", attributes={"colour": ["red", "blue"]})
    with pytest.raises(ValueError):
        index.add_arrays(rng.standard_normal((2, 4)), "ns", attributes={"genre": ["blues"]})
    assert (index.namespace_counts("ns"), index.query_by_metadata("ns", {}), index._ns["ns"].strings["genre"]) == before
    assert index.count("ns", {"genre": "blues"}) == 0 and "fresh" not in index._ns


def test_add_arrays_columnar_attributes():
    rng = np.random.default_rng(2)
    index = widx()
    ids = index.add_arrays(rng.standard_normal((4, 3)), "ns", attributes={
        "genre": ["jazz", None, "rock", "jazz"], "year": np.array([1990, 2000, 2010, 2020]),
        "price": np.array([1.0, np.nan, 3.0, 4.0]), "in_stock": np.array([True, False, True, False])})
    from uuid import UUID
    uu = [UUID(bytes=bytes(r)) for r in ids]
    assert index.query_by_metadata("ns", {"genre": "jazz"}) == [uu[0], uu[3]]
    assert index.query_by_metadata("ns", {"genre": {"$exists": False}}) == [uu[1]]
    assert index.query_by_metadata("ns", {"price": {"$ne": 3}}) == [uu[0], uu[1], uu[3]]
    assert index.query_by_metadata("ns", {"in_stock": True, "year": {"$gt": 1995}}) == [uu[2]]
    assert index.count("unknown", {}) == 0 and index.query_by_metadata("unknown", {"year": 1}) == []
    with pytest.raises(ValueError, match="'colour'"):
        index.count("ns", {"colour": "red"})


def test_schema_refusals():
    with pytest.raises(ValueError):
        Index(attributes={"a": "date"})
    with pytest.raises(ValueError):
        Index(attributes={f"a{i}": "int" for i in range(17)})
    with pytest.raises(ValueError, match="row-sharded"):
        Index(devices=[0, 0], attributes={"a": "int"})
    with pytest.raises(ValueError):
        Index(engine_factory=OracleScanEngine).add_arrays(np.zeros((1, 2)), "ns", attributes={"a": [1]})


# ---------------------------------------------------------------- persistence
def test_v1_snapshot_of_an_attribute_free_index_is_unchanged(tmp_path):
    rng = np.random.default_rng(4)
    index = Index(space="cosine", engine_factory=OracleScanEngine)
    rows = rng.standard_normal((6, 5)).astype(np.float32)
    raw = index.add_arrays(rows, "ns")
    index.remove([__import__("uuid").UUID(bytes=bytes(raw[2]))], "ns")
    index.save_index(str(tmp_path))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["index.json", "ns0.deleted.i64", "ns0.ids.u8", "ns0.rows.f32"]
    want = {"format": "mlvdb-index-v1", "space": "cosine", "rebuild_threshold": 0.2, "namespaces": [
        {"name": "ns", "dim": 5, "space": "cosine", "total": 6, "deleted": 1, "rebuild_required": False}]}
    assert (tmp_path / "index.json").read_text() == json.dumps(want, indent=1)
    assert (tmp_path / "ns0.rows.f32").read_bytes() == rows.tobytes()
    ids = raw.copy()
    ids[2] = 0
    assert (tmp_path / "ns0.ids.u8").read_bytes() == ids.tobytes()
    assert (tmp_path / "ns0.deleted.i64").read_bytes() == np.array([2], np.int64).tobytes()


def test_v2_snapshot_round_trips(tmp_path):
    rng = np.random.default_rng(6)
    index = widx()
    metas = random_metadata(rng, 50)
    vecs = [Vector(values=rng.standard_normal(4), metadata=m) for m in metas]
    index.add(vecs, "a")
    index.add(vecs[:7], "b")
    index.remove([vecs[3].id], "a")
    index.save_index(str(tmp_path))
    meta = json.loads((tmp_path / "index.json").read_text())
    assert meta["format"] == "mlvdb-index-v2" and meta["attributes"] == SCHEMA
    back = Index(engine_factory=WhereOracleEngine)
    assert back.load_index(str(tmp_path)) and back.attributes == SCHEMA
    for f in ({"genre": "jazz"}, {"price": {"$gte": 40}}, {"$not": {"year": {"$exists": True}}}, {"in_stock": False}):
        for ns in ("a", "b"):
            assert back.query_by_metadata(ns, f) == index.query_by_metadata(ns, f), (ns, f)
    q = rng.standard_normal((2, 4))
    assert hits(back.search_many(q, 5, "a", "l2", where={"genre": {"$in": ["jazz", "rock"]}})) == \
        hits(index.search_many(q, 5, "a", "l2", where={"genre": {"$in": ["jazz", "rock"]}}))
    # v1 snapshots still load into an index with attributes: every value absent
    plain = Index(engine_factory=OracleScanEngine)
    plain.add(vecs[:4], "p")
    plain.save_index(str(tmp_path / "v1"))
    v1 = widx()
    assert v1.load_index(str(tmp_path / "v1"))
    assert v1.count("p", {}) == 4 and v1.count("p", {"genre": {"$exists": True}}) == 0


# ---------------------------------------------------------------- QueryProcessor
def test_query_processor_dict_where_matches_the_callable_path():
    rng = np.random.default_rng(8)
    qp = QueryProcessor(InMemoryStorage(), widx(space="cosine"))
    metas = random_metadata(rng, 90)
    from mlvectordb_amd import VectorDTO
    qp.upsert_many([VectorDTO(values=rng.standard_normal(6).tolist(), metadata=m) for m in metas], "ns")
    f = {"year": {"$gte": 1980}, "genre": {"$in": ["jazz", "blues"]}}
    pred = lambda m: py_match(f, m)  # noqa: E731
    q = rng.standard_normal((3, 6))
    assert qp.find_similar_many(q, 7, "ns", where=f) == qp.find_similar_many(q, 7, "ns", where=pred)
    one = VectorDTO(values=q[0].tolist(), metadata={})
    assert qp.find_similar_where(one, 4, f, "ns") == qp.find_similar_where(one, 4, pred, "ns")
    assert qp.find_in_radius(one, 0.9, "ns", where=f) == qp.find_in_radius(one, 0.9, "ns", where=pred)
    assert qp.count_where(f, "ns") == qp.count_where(pred, "ns") > 0
    assert qp.query_by_metadata(f, "ns") == qp.query_by_metadata(pred, "ns")


def test_upsert_arrays_extracts_declared_attributes():
    from mlvectordb_amd import ArrayStorage
    rng = np.random.default_rng(9)
    qp = QueryProcessor(ArrayStorage(), widx())
    metas = [{"genre": "jazz", "year": 1990}, {"genre": "rock"}, {"year": 2001, "x": 1}]
    qp.upsert_arrays(rng.standard_normal((3, 4)), "ns", metadata=metas)
    assert qp.count_where({"genre": "jazz"}, "ns") == 1 and qp.count_where({"year": {"$exists": True}}, "ns") == 2
    with pytest.raises(ValueError):
        qp.upsert_arrays(rng.standard_normal((1, 4)), "ns", metadata=[{"year": "1990"}])
    assert qp.count_where({}, "ns") == 3


# ---------------------------------------------------------------- the raw-program generator and the NumPy evaluator
def _scalar_match(program, cols, i):
    """One row through the program, op by op, with Python ints and floats: the semantics of include/mlvdb_where.h."""
    stack = []
    for op, attr, a, b in program.ops.tolist():
        if op in (W.AND, W.OR):
            y, x = stack.pop(), stack.pop()
            stack.append((x and y) if op == W.AND else (x or y))
        elif op == W.NOT:
            stack.append(not stack.pop())
        elif op == W.TRUE:
            stack.append(True)
        elif cols[attr].dtype == np.int64:
            v = int(cols[attr][i])
            have = v != -(2 ** 63)
            if op == W.IN:
                stack.append(have and v in program.set[a:a + b].tolist())
            elif op == W.EXISTS:
                stack.append(have)
            elif op == W.NE:
                stack.append(not (have and v == a))
            else:
                stack.append(have and {W.EQ: v == a, W.LT: v < a, W.LE: v <= a, W.GT: v > a, W.GE: v >= a}[op])
        else:
            v = float(cols[attr][i])
            lit = float(np.array([a], np.int64).view(np.float64)[0])
            stack.append({W.EQ: v == lit, W.NE: not v == lit, W.LT: v < lit, W.LE: v <= lit, W.GT: v > lit,
                          W.GE: v >= lit, W.EXISTS: v == v}[op])
    assert len(stack) == 1
    return stack[0]


def test_raw_programs_are_valid_and_the_numpy_evaluator_matches_a_scalar_one():
    from tests.where_helpers import eval_program, hostile_columns, program_depth, random_raw_program

    rng = np.random.default_rng(32)
    kinds = {0: "int64", 3: "float64", 7: "int64", 15: "float64"}
    n = 300
    cols = hostile_columns(rng, n, kinds)
    sizes = set()
    for j in range(60):
        size = [1, 2, 17, 63, 64][j % 5]
        prog = random_raw_program(rng, kinds, size, deep=j % 3 == 0, p_in=0.3)
        ops = prog.ops
        # the host validation of api.hip (where_prepare): exactly `size` ops, depth 1..32 throughout and 1 at the end,
        # IN on int64 columns only, every IN range inside the set table and sorted
        assert ops.size == size and program_depth(prog) <= W.MAX_DEPTH
        depth = 0
        for op, attr, a, b in ops.tolist():
            depth += 1 if op <= W.EXISTS else (-1 if op in (W.AND, W.OR) else 0)
            assert depth >= 1
            if W.EQ <= op <= W.EXISTS:
                assert attr in kinds
            if op == W.IN:
                assert kinds[attr] == "int64" and 0 <= a and 0 <= b and a + b <= prog.set.size
                r = prog.set[a:a + b]
                assert np.all(r[:-1] <= r[1:])
                sizes.add(min(b, 2))
        assert depth == 1
        if size == 64 and j % 3 == 0:
            assert program_depth(prog) == W.MAX_DEPTH
        got = eval_program(prog, cols, n)
        want = np.array([_scalar_match(prog, cols, i) for i in range(n)])
        assert np.array_equal(got, want), j
    assert sizes == {0, 1, 2}  # empty, single and longer IN ranges all drawn
