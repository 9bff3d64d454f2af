"""List-valued attributes without a GPU: the filter compiler, the encoder, ``Index`` on the model engine against the direct
evaluation of the filters, snapshots, the C entries' refusals of a null handle, and the kernels' resource report."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import uuid
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from mlvectordb_amd import where as W
from tests.mutate_helpers import MutateOracleEngine
from tests.tags_helpers import TAG_SCHEMA, TagsOracleEngine, py_match, random_tag_filter, random_tag_metadata

ROOT = Path(__file__).resolve().parents[1]
SCHEMA = {"tags": "str[]", "nums": "int[]", "year": "int"}
STRINGS = {"tags": {"jazz": 0, "live": 1, "1959": 2}}


def ops_of(where, schema=SCHEMA, strings=STRINGS):
    p = W.compile_where(where, schema, strings)
    return p.ops.tolist(), p.set.tolist()


FALSE = [(W.TRUE, 0, 0, 0), (W.NOT, 0, 0, 0)]


# ---------------------------------------------------------------- the compiler
@pytest.mark.parametrize("where, ops, table", [
    ({"tags": "live"}, [(W.HAS, 0, 1, 0)], []),
    ({"tags": {"$eq": "jazz"}}, [(W.HAS, 0, 0, 0)], []),
    ({"nums": 7}, [(W.HAS, 1, 7, 0)], []),
    ({"tags": {"$ne": "live"}}, [(W.HAS, 0, 1, 0), (W.NOT, 0, 0, 0)], []),
    ({"tags": {"$in": ["1959", "jazz", "jazz"]}}, [(W.HAS_ANY, 0, 0, 2)], [0, 2]),
    ({"tags": {"$nin": ["live"]}}, [(W.HAS_ANY, 0, 0, 1), (W.NOT, 0, 0, 0)], [1]),
    ({"tags": {"$all": ["live", "jazz", "live"]}}, [(W.HAS_ALL, 0, 0, 2)], [0, 1]),
    ({"nums": {"$all": [9, -3]}, "tags": {"$in": ["live"]}},
     [(W.HAS_ALL, 1, 0, 2), (W.HAS_ANY, 0, 2, 1), (W.AND, 0, 0, 0)], [-3, 9, 1]),
    ({"tags": {"$size": 3}}, [(W.LEN, 0, 3, 3)], []),
    ({"tags": {"$size": {"$gte": 1, "$lt": 4}}}, [(W.LEN, 0, 1, 3)], []),
    ({"tags": {"$size": {"$gt": 1}}}, [(W.LEN, 0, 2, 255)], []),
    ({"tags": {"$size": {"$lte": 2}}}, [(W.LEN, 0, 0, 2)], []),
    ({"tags": {"$size": {"$gt": 4, "$lt": 4}}}, FALSE, []),
    ({"tags": {"$size": 256}}, FALSE, []),
    ({"tags": {"$exists": True}}, [(W.EXISTS, 0, 0, 0)], []),
    ({"tags": {"$exists": False}}, [(W.EXISTS, 0, 0, 0), (W.NOT, 0, 0, 0)], []),
    # a string never ingested matches nothing; under $all the whole clause is false
    ({"tags": "zydeco"}, FALSE, []),
    ({"tags": {"$ne": "zydeco"}}, FALSE + [(W.NOT, 0, 0, 0)], []),
    ({"tags": {"$in": ["zydeco", "live"]}}, [(W.HAS_ANY, 0, 0, 1)], [1]),
    ({"tags": {"$in": ["zydeco"]}}, FALSE, []),
    ({"tags": {"$in": []}}, FALSE, []),
    ({"tags": {"$all": ["jazz", "zydeco"]}}, FALSE, []),
    ({"nums": 2 ** 70}, FALSE, []),
])
def test_list_operators_compile_to_the_list_ops(where, ops, table):
    assert ops_of(where) == (ops, table)


def test_a_program_of_list_ops_counts_its_depth():
    assert W.compile_where(_nest(W.MAX_DEPTH), SCHEMA, STRINGS).ops.size == 2 * W.MAX_DEPTH - 1
    with pytest.raises(ValueError, match="65 ops"):  # (a stack 33 deep takes 65 ops: the length limit speaks first)
        W.compile_where(_nest(W.MAX_DEPTH + 1), SCHEMA, STRINGS)


def _nest(depth):
    """A filter whose postfix form holds ``depth`` list ops on the stack at once."""
    node = {"tags": "jazz"}
    for _ in range(depth - 1):
        node = {"$and": [{"tags": "live"}, node]}
    return node


@pytest.mark.parametrize("where, message", [
    ({"tags": {"$lt": "jazz"}}, r"\$lt does not"),
    ({"nums": {"$gte": 3}}, r"\$gte does not"),
    ({"tags": {"$lte": "a"}}, r"\$lte does not"),
    ({"nums": {"$gt": 3}}, r"\$gt does not"),
    ({"year": {"$all": [1959]}}, r"\$all applies to list attributes"),
    ({"year": {"$size": 1}}, r"\$size applies to list attributes"),
    ({"tags": {"$all": []}}, "not empty"),
    ({"tags": {"$all": "jazz"}}, "takes a list"),
    ({"tags": {"$in": "jazz"}}, "takes a list"),
    ({"tags": 3}, "not a string"),
    ({"nums": "3"}, "not an int"),
    ({"nums": 2.0}, "not an int"),
    ({"tags": {"$size": "3"}}, r"\$size takes an int"),
    ({"tags": {"$size": True}}, r"\$size takes an int"),
    ({"tags": {"$size": {"$in": [1]}}}, r"\$size: unknown operator"),
    ({"tags": {"$size": {}}}, "empty operator dict"),
    ({"tags": {"$push": "x"}}, "unknown operator"),
])
def test_refused_list_filters(where, message):
    with pytest.raises(ValueError, match=message):
        W.compile_where(where, SCHEMA, STRINGS)


# ---------------------------------------------------------------- the encoder
def test_encoding_sorts_dedupes_and_tells_absent_from_empty():
    codes = {}
    col = W.encode_list_column("tags", "str[]", [["b", "a", "b"], None, [], ("c",), {"a"}], codes)
    assert codes == {"b": 0, "a": 1, "c": 2}
    assert col.offsets.tolist() == [0, 2, 2, 2, 3, 4] and col.values.tolist() == [0, 1, 2, 1]
    assert col.present.tolist() == [1, 0, 1, 1, 1]
    assert [col.row(i) for i in range(5)] == [[0, 1], None, [], [2], [1]]
    col = W.encode_list_column("nums", "int[]", [[5, -7, 5, 2 ** 63 - 1, -(2 ** 63) + 1]], {})
    assert col.values.tolist() == [-(2 ** 63) + 1, -7, 5, 2 ** 63 - 1]
    sub = W.encode_list_column("nums", "int[]", [[3], None, [1, 2], []], {}).take([2, 1, 3])
    assert (sub.offsets.tolist(), sub.values.tolist(), sub.present.tolist()) == ([0, 2, 2, 2], [1, 2], [1, 0, 1])


def test_the_255_limit_counts_distinct_elements():
    ok = W.encode_list_column("nums", "int[]", [list(range(255)) * 2], {})
    assert ok.values.tolist() == list(range(255))
    with pytest.raises(ValueError, match="256 distinct elements"):
        W.encode_list_column("nums", "int[]", [list(range(256))], {})
    with pytest.raises(ValueError, match="256 distinct elements"):
        W.encode_list_column("tags", "str[]", [[str(i) for i in range(256)]], {})


@pytest.mark.parametrize("kind, value, message", [
    ("str[]", "jazz", "not a list, tuple or set"),
    ("int[]", 3, "not a list, tuple or set"),
    ("str[]", {"a": 1}, "not a list, tuple or set"),
    ("str[]", ["a", 3], "the element 3"),
    ("int[]", [1, "2"], "the element '2'"),
    ("int[]", [1, 2.0], "the element 2.0"),
    ("int[]", [True], "the element True"),
    ("int[]", [-(2 ** 63)], "outside int64"),
    ("int[]", [2 ** 63], "outside int64"),
])
def test_refused_list_values(kind, value, message):
    with pytest.raises(ValueError, match=message):
        W.encode_list_column("x", kind, [[] if kind == "str[]" else [1], value], {})


# ---------------------------------------------------------------- Index on the model engine
def _index(space="cosine", schema=TAG_SCHEMA, engine=TagsOracleEngine):
    return Index(space=space, engine_factory=lambda dim, sp: engine(dim, sp), attributes=schema)


def _vectors(rng, metas, d=8):
    return [Vector(values=rng.standard_normal(d).astype(np.float32).tolist(), metadata=m) for m in metas]


@pytest.fixture(scope="module")
def tagged():
    rng = np.random.default_rng(11)
    metas = random_tag_metadata(rng, 400)
    vectors = _vectors(rng, metas)
    index = _index()
    index.add(vectors[:150], "ns")
    index.add(vectors[150:], "ns")
    dead = [v.id for v in vectors[::9]]
    index.remove(dead, "ns")
    live = [(v, m) for v, m in zip(vectors, metas) if v.id not in set(dead)]
    return index, live, rng


def test_filters_count_and_list_what_py_match_does(tagged):
    index, live, rng = tagged
    hits = 0
    for _ in range(150):
        where = random_tag_filter(rng)
        want = [v.id for v, m in live if py_match(where, m)]
        hits += bool(want)
        assert index.count("ns", where) == len(want), where
        assert index.query_by_metadata("ns", where) == want, where
    assert hits > 50


def test_search_many_with_a_list_filter_ranks_the_matching_rows(tagged):
    index, live, rng = tagged
    q = np.asarray(live[5][0].values, dtype=np.float32)[None]
    where = {"tags": {"$all": ["jazz"]}, "nums": {"$size": {"$gte": 1}}}
    allowed = {v.id for v, m in live if py_match(where, m)}
    assert 3 < len(allowed) < len(live)
    got = index.search_many(q, 5, "ns", "cosine", where=where)
    assert set(got.ids()[0].tolist()) <= allowed and int(got.counts[0]) == 5


def test_facets_count_rows_per_element(tagged):
    index, live, rng = tagged
    for by, where in (("tags", None), ("tags", {"year": {"$gte": 1960}}), ("nums", {"tags": "live"})):
        rows = [m for v, m in live if where is None or py_match(where, m)]
        counts = Counter(e for m in rows for e in set(m.get(by) or ()))
        got = index.facets("ns", by, where, order="value")
        assert got["values"] == sorted(counts.items())
        assert got["matched"] == len(rows) and got["absent"] == sum(not m.get(by) for m in rows)
    top = index.facets("ns", "tags", limit=2)["values"]
    assert top == sorted(Counter(e for v, m in live for e in set(m.get("tags") or ())).items(), key=lambda p: (-p[1], p[0]))[:2]
    with pytest.raises(ValueError, match="max_values"):
        index.facets("ns", "nums", max_values=3)


def test_updates_by_id_and_by_filter_follow_the_model():
    rng = np.random.default_rng(5)
    metas = random_tag_metadata(rng, 120)
    vectors = _vectors(rng, metas)
    index = _index()
    index.add(vectors, "ns")
    model = {v.id: dict(m) for v, m in zip(vectors, metas)}

    def check():
        for where in ({"tags": "fresh"}, {"tags": {"$size": 0}}, {"tags": {"$exists": False}}, {"nums": {"$all": [1, 2]}},
                      {"tags": {"$nin": ["jazz", "fresh"]}}):
            assert index.query_by_metadata("ns", where) == [v.id for v in vectors if py_match(where, model[v.id])], where

    ids = [v.id for v in vectors[:30]]
    patches = [{"tags": ["fresh", "jazz"]}, {"tags": None}, {"tags": []}] * 10
    assert index.update_attributes(ids, patches, "ns") == 30
    for i, p in zip(ids, patches):
        model[i].update(p)
    check()
    assert index.update_attributes([ids[0], ids[0], uuid.uuid4()], [{"nums": [9]}, {"nums": [1, 2, 1]}, {"nums": [4]}], "ns") == 1
    model[ids[0]]["nums"] = [1, 2]
    check()
    # by filter: the predicate reads the column it assigns
    where = {"tags": "fresh"}
    n = sum(py_match(where, m) for m in model.values())
    assert index.update_where("ns", where, {"tags": ["stale"]}) == n > 0
    for m in model.values():
        if py_match(where, m):
            m["tags"] = ["stale"]
    check()
    assert index.count("ns", {"tags": "stale"}) == n
    where = {"tags": {"$size": 0}}
    n = sum(py_match(where, m) for m in model.values())
    assert index.update_where("ns", where, {"tags": None}) == n > 0
    for m in model.values():
        if py_match(where, m):
            m["tags"] = None
    check()
    # a scalar and a list in one call: fine while the filter reads neither
    where = {"nums": {"$size": {"$gte": 2}}}
    n = sum(py_match(where, m) for m in model.values())
    assert index.update_where("ns", where, {"tags": ["big"], "year": 2000}) == n > 0
    assert index.count("ns", {"tags": "big", "year": 2000}) == n
    # remove_where with a list filter
    gone = index.remove_where("ns", {"tags": "big"}, return_ids=True)
    assert len(gone) == n and index.count("ns", {"tags": "big"}) == 0


@pytest.mark.parametrize("call, message", [
    (lambda ix: ix.update_where("ns", {}, {"tags": {"$inc": 1}}), r"\$inc adds to numbers"),
    (lambda ix: ix.update_where("ns", {}, {"tags": "bare"}), "not a list, tuple or set"),
    (lambda ix: ix.update_where("ns", {"tags": "a"}, {"tags": ["b"], "year": 1}), "several passes"),
    (lambda ix: ix.update_attributes([uuid.uuid4()], {"nums": [1.5]}, "ns"), "the element 1.5"),
    (lambda ix: ix.update_attributes([uuid.uuid4()], {"tags": list(map(str, range(300)))}, "ns"), "at most 255"),
    (lambda ix: ix.top_by("ns", "tags", 3), "needs a scalar attribute"),
    (lambda ix: ix.histogram("ns", "nums", [1, 2]), "needs a scalar attribute"),
    (lambda ix: ix.search_many(np.zeros((1, 8), np.float32), 3, "ns", "cosine", distinct="tags"), "needs a scalar attribute"),
    (lambda ix: ix.search_late([np.zeros((2, 8), np.float32)], 3, "ns", "cosine", by="nums"), "needs a scalar attribute"),
    (lambda ix: ix.add([Vector(values=[0.0] * 8, metadata={"tags": "bare"})], "ns"), "not a list, tuple or set"),
    (lambda ix: ix.add([Vector(values=[0.0] * 8, metadata={"nums": list(range(256))})], "ns"), "at most 255"),
])
def test_refusals_come_before_anything_is_mutated(call, message):
    rng = np.random.default_rng(2)
    index = _index()
    index.add(_vectors(rng, [{"tags": ["a"], "nums": [1], "year": 1}] * 4), "ns")
    before = (index.count("ns", {}), index.count("ns", {"tags": "a"}), index.facets("ns", "tags"), index.facets("ns", "nums"))
    with pytest.raises(ValueError, match=message):
        call(index)
    assert before == (index.count("ns", {}), index.count("ns", {"tags": "a"}), index.facets("ns", "tags"),
                      index.facets("ns", "nums"))
    assert index.count("ns", {"tags": {"$in": ["b", "bare"] + list(map(str, range(300)))}}) == 0  # no string leaked in


def test_unknown_list_type_is_refused():
    with pytest.raises(ValueError, match="not one of"):
        Index(attributes={"tags": "float[]"})


def test_query_processor_keeps_the_storage_in_step():
    rng = np.random.default_rng(3)
    qp = QueryProcessor(InMemoryStorage(), _index(schema={"tags": "str[]", "year": "int"}))
    metas = [{"tags": ["a", "b"], "year": 1, "note": "x"}, {"tags": ["b"], "year": 2}, {"tags": [], "year": 3}, {"year": 4}]
    qp.upsert_many([VectorDTO(values=rng.standard_normal(8).tolist(), metadata=m) for m in metas])
    ids = qp.query_by_metadata({})  # insertion order
    assert qp.facets("tags")["values"] == [("b", 2), ("a", 1)] == qp.facets("tags", where=lambda m: True)["values"]
    assert qp.facets("tags", where=lambda m: True)["absent"] == 2 == qp.facets("tags")["absent"]
    qp.update_metadata([ids[3]], {"tags": ["c", "a"]})
    assert qp.update_where({"tags": "b"}, {"tags": ["z"]}) == 2
    stored = [v.metadata.get("tags") for v in qp._storage.read_vectors(ids, "default")]
    assert stored == [["z"], ["z"], [], ["c", "a"]]
    assert qp.facets("tags", order="value")["values"] == [("a", 1), ("c", 1), ("z", 2)]
    assert qp.facets("tags", where=lambda m: True, order="value")["values"] == [("a", 1), ("c", 1), ("z", 2)]


# ---------------------------------------------------------------- snapshots
def _sha(path):
    return {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(Path(path).iterdir()) if p.is_file()}


def test_v3_snapshot_round_trip(tmp_path):
    rng = np.random.default_rng(8)
    metas = random_tag_metadata(rng, 90)
    vectors = _vectors(rng, metas)
    index = _index()
    index.add(vectors, "ns")
    index.remove([v.id for v in vectors[::7]], "ns")
    index.update_attributes([vectors[1].id, vectors[2].id], [{"tags": []}, {"tags": None}], "ns")  # leaves garbage behind
    metas[1]["tags"], metas[2]["tags"] = [], None
    index.save_index(str(tmp_path))
    manifest = json.loads((tmp_path / "index.json").read_text())
    assert manifest["format"] == "mlvdb-index-v3" and manifest["attributes"] == TAG_SCHEMA
    names = {p.name for p in tmp_path.iterdir()}
    assert {"ns0.attr0.i64", "ns0.attr0.offsets.i64", "ns0.attr0.values.i64", "ns0.attr1.offsets.i64", "ns0.attr2.i64",
            "ns0.attr3.f64"} <= names
    # the live CSR: exactly what the live rows hold
    live = [m for i, m in enumerate(metas) if i % 7]
    assert (tmp_path / "ns0.attr0.values.i64").stat().st_size == 8 * sum(len(set(m.get("tags") or ())) for m in live)
    loaded = _index(schema={})
    assert loaded.load_index(str(tmp_path)) and loaded.attributes == TAG_SCHEMA
    for _ in range(60):
        where = random_tag_filter(rng)
        assert loaded.query_by_metadata("ns", where) == index.query_by_metadata("ns", where) == \
            [v.id for i, (v, m) in enumerate(zip(vectors, metas)) if i % 7 and py_match(where, m)], where
    assert loaded.facets("ns", "tags") == index.facets("ns", "tags")
    loaded.save_index(str(tmp_path / "again"))
    assert _sha(tmp_path / "again") == _sha(tmp_path)
    (tmp_path / "ns0.attr0.values.i64").unlink()
    with pytest.raises(RuntimeError, match="list attribute files"):
        _index(schema={}).load_index(str(tmp_path))


# sha256 of every file ``_legacy_index`` saved before list attributes existed (v1: no attributes, v2: scalar ones)
LEGACY = {
    "v1": {
        "index.json": "09a5725fb6dbc4fdf14abeed9985324d4f8185a92b99f30cf13a2cc257fa2cc5",
        "ns0.deleted.i64": "d81ee2a043271a318af1f2a3255de6ce32fcda013767d9fc3d7b81c97dda6e77",
        "ns0.ids.u8": "86c4663bdfcb933c1fd080ffa0937a59624b8e4c1ed51c12cfa2fe5db6020e14",
        "ns0.rows.f32": "ce067778bb0daa94556fe26351851542ac0461559b624756afa6a2e81f35e1c3",
    },
    "v2": {
        "index.json": "6b95b191ff078ffb344d19adedbbad05009af88be845f9266c4d3eda0c44afe2",
        "ns0.attr0.i64": "b5cc9f4c63bed20d83feb7a60957b697470b870c9b7e48795ce2ecfb1fc26dd5",
        "ns0.attr1.i64": "517b0bf7b7bd144b2d6598f58cc2e825d4e5d73efa364bb1c62fcf80e8f8d378",
        "ns0.attr2.f64": "28ed31e0ab585df71505ca336f726de6323960bc2a623ba681051798d09c43ff",
        "ns0.deleted.i64": "d81ee2a043271a318af1f2a3255de6ce32fcda013767d9fc3d7b81c97dda6e77",
        "ns0.ids.u8": "86c4663bdfcb933c1fd080ffa0937a59624b8e4c1ed51c12cfa2fe5db6020e14",
        "ns0.rows.f32": "ce067778bb0daa94556fe26351851542ac0461559b624756afa6a2e81f35e1c3",
    },
}


def _legacy_index(version):
    rng = np.random.default_rng(21)
    schema = {} if version == "v1" else {"genre": "str", "year": "int", "price": "float"}
    index = Index(space="l2", engine_factory=lambda dim, sp: MutateOracleEngine(dim, sp), attributes=schema)
    vectors = [Vector(values=rng.standard_normal(6).astype(np.float32).tolist(),
                      metadata={"genre": ["jazz", "blues", None][i % 3], "year": 1950 + i, "price": i / 4 if i % 5 else None})
               for i in range(40)]
    for i, v in enumerate(vectors):
        v._id = uuid.UUID(int=1000 + i)  # (ids are random by default: fixed here, the files are hashed)
    index.add(vectors, "ns")
    index.remove([v.id for v in vectors[::6]], "ns")
    return index


@pytest.mark.parametrize("version", ["v1", "v2"])
def test_snapshots_without_list_attributes_are_byte_identical_to_before(tmp_path, version):
    _legacy_index(version).save_index(str(tmp_path))
    assert json.loads((tmp_path / "index.json").read_text())["format"] == f"mlvdb-index-{version}"
    assert _sha(tmp_path) == LEGACY[version]
    loaded = Index(space="l2", engine_factory=lambda dim, sp: MutateOracleEngine(dim, sp))
    assert loaded.load_index(str(tmp_path))
    loaded.save_index(str(tmp_path / "again"))
    assert _sha(tmp_path / "again") == LEGACY[version]


# ---------------------------------------------------------------- the C ABI without a device
def test_list_entries_are_declared_bound_and_refuse_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_list.h").read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(_native.LIST_SIGNATURES) and len(names) == 6
    others = [t for n, t in vars(_native).items() if n.endswith("SIGNATURES") and n != "LIST_SIGNATURES"]
    assert not any(set(names) & set(t) for t in others)
    for name in names:  # the parameter count of each prototype is the binding's
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert len(params) == len(_native.LIST_SIGNATURES[name][1]), name
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert int(consts["MLVDB_ATTR_INT64_LIST"]) == _native.ATTR_INT64_LIST == 3
    assert int(consts["MLVDB_LIST_MAX_LEN"]) == _native.LIST_MAX_LEN == W.LIST_MAX_LEN == 255
    assert [int(consts[f"MLVDB_WHERE_{n}"]) for n in ("HAS", "HAS_ANY", "HAS_ALL", "LEN")] == \
        [W.HAS, W.HAS_ANY, W.HAS_ALL, W.LEN] == [12, 13, 14, 15]
    lib = _native.load()
    assert lib.mlvdb_abi_version() == 7 == _native.ABI_VERSION
    null, z, buf = C.c_void_p(), C.c_int64(0), (C.c_int64 * 4)()
    w = _native.Where(None, 0, None, 0)
    calls = {
        "mlvdb_attr_list_set": (null, 0, 0, 1, buf, buf, None),
        "mlvdb_attr_list_set_at": (null, 0, buf, 1, buf, buf, None, C.byref(z)),
        "mlvdb_attr_list_get": (null, 0, 0, 1, buf, buf, None, 4, C.byref(z)),
        "mlvdb_attr_list_update_where": (null, C.byref(w), 0, buf, 1, 0, C.byref(z)),
        "mlvdb_attr_list_stats": (null, 0, C.byref(z), C.byref(z)),
        "mlvdb_facet_list_values": (null, 0, None, 4, buf, buf, C.byref(z), C.byref(z), C.byref(z)),
    }
    assert sorted(calls) == names
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 1, name  # MLVDB_ERR_INVALID_ARG
        assert b"null index handle" in lib.mlvdb_last_global_error(), name


def test_where_op_stays_32_bytes_and_every_new_entry_is_guarded():
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    for name in _native.LIST_SIGNATURES:
        body = re.search(r"^int " + name + r"\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
        assert body.lstrip().startswith("return guarded("), name
    assert "static_assert(sizeof(WhereOp) == 32" in (ROOT / "mlvectordb_amd" / "csrc" / "internal.h").read_text()


# ---------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_where_eval_and_the_list_kernels_use_no_scratch(tmp_path):
    """DESIGN 11.12 records the VGPR counts this report gives."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "mlvectordb_amd" / "csrc"
    seen = {}
    for src in ("kernels_where.hip", "kernels_list.hip", "kernels_facet.hip"):
        out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                              "-Rpass-analysis=kernel-resource-usage", "-c", str(csrc / src), "-o", str(tmp_path / "k.o")],
                             capture_output=True, text=True, cwd=csrc, check=True).stderr
        name = None
        for line in out.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and name:
                seen[name] = int(m.group(1))
    for kernel in ("where_eval_kernel", "list_block_sums_kernel", "list_scan_sums_kernel", "list_move_kernel",
                   "facet_list_values_kernel", "facet_values_kernel"):
        hits = [v for k, v in seen.items() if kernel in k]
        assert hits and all(v == 0 for v in hits), (kernel, seen)
