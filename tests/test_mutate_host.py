"""Attribute updates and deletes by filter (include/mlvdb_mutate.h): the C ABI's shape, ``Index`` over the NumPy engine
against a list-of-dicts model, the storages and ``QueryProcessor``.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import ArrayStorage, Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from oracle.engine import OracleScanEngine
from tests.mutate_helpers import MutateOracleEngine, UntouchableEngine, replay_history
from tests.where_helpers import SCHEMA, py_match, random_metadata

ROOT = Path(__file__).resolve().parents[1]


def mutate_header_functions():
    text = (ROOT / "include" / "mlvdb_mutate.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))


# ---------------------------------------------------------------- C ABI
def test_mutate_header_symbols_are_exported_and_bound():
    lib = _native.load()
    names = mutate_header_functions()
    assert names == ["mlvdb_attr_set_at", "mlvdb_attr_update_where", "mlvdb_tombstone_where"] == sorted(_native.MUTATE_SIGNATURES)
    for name in names:
        assert hasattr(lib, name), name
    others = [t for n, t in vars(_native).items() if n.endswith("SIGNATURES") and n != "MUTATE_SIGNATURES"]
    assert len(others) >= 9
    for table in others:
        assert not set(names) & set(table)
    text = (ROOT / "include" / "mlvdb_mutate.h").read_text()
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert (int(consts["MLVDB_SET_ASSIGN"]), int(consts["MLVDB_SET_ADD"])) == (_native.SET_ASSIGN, _native.SET_ADD) == (0, 1)
    assert np.dtype(_native.ASSIGN_DTYPE).itemsize == 16
    assert lib.mlvdb_abi_version() == _native.ABI_VERSION == 7


def test_every_mutate_entry_refuses_a_null_handle_with_a_status_code():
    lib = _native.load()
    null = C.c_void_p()
    z64, y64 = C.c_int64(0), C.c_int64(0)
    buf = (C.c_int64 * 4)()
    w = _native.Where()
    calls = {
        "mlvdb_attr_set_at": (null, 0, buf, 1, buf, C.byref(z64)),
        "mlvdb_attr_update_where": (null, C.byref(w), buf, 1, C.byref(z64), C.byref(y64)),
        "mlvdb_tombstone_where": (null, C.byref(w), buf, 1, C.byref(z64)),
    }
    assert sorted(calls) == sorted(_native.MUTATE_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 1, name  # MLVDB_ERR_INVALID_ARG
        assert b"null index handle" in lib.mlvdb_last_global_error(), name


def test_every_mutate_entry_runs_inside_the_exception_guard():
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    region = text[text.index('extern "C" {'):text.index('}  // extern "C"')]
    bodies = dict(re.findall(r"^int (mlvdb_\w+)\([^)]*\) \{\n(.*?)^\}", region, flags=re.S | re.M))
    for name in mutate_header_functions():
        assert name in bodies, name
        assert bodies[name].lstrip().startswith("return guarded("), f"{name} is not wrapped by guarded()"


def test_the_mutate_kernels_are_in_the_build():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_mutate\.hip\b", make, flags=re.M)
    hdrs = make[make.index("HDRS ="):make.index("# the filter scan")]
    assert "../../include/mlvdb_mutate.h" in hdrs


# ---------------------------------------------------------------- Index on the NumPy engine
def midx(space="l2", factory=MutateOracleEngine, **kw):
    return Index(space=space, engine_factory=factory, attributes=SCHEMA, **kw)


def filled(factory=MutateOracleEngine, n=40, seed=1, **kw):
    rng = np.random.default_rng(seed)
    index = midx(factory=factory, **kw)
    vecs = [Vector(values=rng.standard_normal(5), metadata=m) for m in random_metadata(rng, n)]
    index.add(vecs, "ns")
    return index, vecs


BAD_UPDATE_ATTRIBUTES = [
    {"colour": "red"},                      # not declared
    {"year": "1990"}, {"year": 1.5}, {"year": 2 ** 63}, {"year": -(2 ** 63)},
    {"genre": 3}, {"in_stock": 1}, {"price": "9"}, {"price": True},
    {"year": {"$inc": 1}},                  # per-row increments are update_where's
    [{"year": 1}],                          # one mapping for two ids
    [{"year": 1}, 7],
]
BAD_UPDATE_WHERE = [
    ({"colour": "red"}, {"year": 1}), ({"year": {"$almost": 1}}, {"year": 1}), ("year > 3", {"year": 1}),
    ({}, {}), ({}, {"colour": 1}), ({}, {"year": "x"}), ({}, {"year": {"$dec": 1}}), ({}, {"year": {"$inc": 1, "$x": 2}}),
    ({}, {"year": {"$inc": 1.5}}), ({}, {"year": {"$inc": True}}), ({}, {"year": {"$inc": 2 ** 63}}),
    ({}, {"price": {"$inc": float("nan")}}), ({}, {"price": {"$inc": "1"}}), ({}, {"price": {"$inc": True}}),
    ({}, {"genre": {"$inc": 1}}), ({}, {"in_stock": {"$inc": 1}}), ({}, [("year", 1)]),
]
BAD_REMOVE_WHERE = [{"colour": "red"}, {"year": {"$gt": "x"}}, None, [{"year": 1}]]


def test_every_refusal_comes_before_the_engine_and_the_dictionary_are_touched():
    index, vecs = filled(UntouchableEngine)
    ids = [vecs[0].id, vecs[1].id]
    strings = {k: dict(v) for k, v in index._ns["ns"].strings.items()}
    before = [index.query_by_metadata("ns", {k: {"$exists": True}}) for k in SCHEMA]
    UntouchableEngine.armed = True
    try:
        for values in BAD_UPDATE_ATTRIBUTES:
            with pytest.raises(ValueError):
                index.update_attributes(ids, values, "ns")
        with pytest.raises(ValueError):  # a new string next to a refused value: no code is minted
            index.update_attributes(ids, [{"genre": "gamelan"}, {"year": "x"}], "ns")
        for where, values in BAD_UPDATE_WHERE:
            with pytest.raises(ValueError):
                index.update_where("ns", where, values)
        with pytest.raises(ValueError):
            index.update_where("ns", {}, {"genre": "gamelan", "year": 1.5})
        for where in BAD_REMOVE_WHERE:
            with pytest.raises(ValueError):
                index.remove_where("ns", where)
        # unknown namespace: the arguments are checked all the same, then nothing happens
        for values in BAD_UPDATE_ATTRIBUTES:
            with pytest.raises(ValueError):
                index.update_attributes(ids, values, "nowhere")
        for where, values in BAD_UPDATE_WHERE:
            with pytest.raises(ValueError):
                index.update_where("nowhere", where, values)
        for where in BAD_REMOVE_WHERE:
            with pytest.raises(ValueError):
                index.remove_where("nowhere", where)
        assert index.update_attributes(ids, {"year": 1}, "nowhere") == 0
        assert index.update_where("nowhere", {}, {"year": 1}) == 0
        assert index.remove_where("nowhere", {}) == 0 and index.remove_where("nowhere", {}, return_ids=True) == []
        assert index.update_attributes([], {"year": 1}, "ns") == 0
    finally:
        UntouchableEngine.armed = False
    assert index._ns["ns"].strings == strings
    assert [index.query_by_metadata("ns", {k: {"$exists": True}}) for k in SCHEMA] == before


def test_an_engine_without_the_entries_is_a_value_error():
    from tests.where_helpers import WhereOracleEngine

    index, vecs = filled(WhereOracleEngine)
    strings = {k: dict(v) for k, v in index._ns["ns"].strings.items()}
    with pytest.raises(ValueError, match="set_attr_at"):
        index.update_attributes([vecs[0].id], {"genre": "gamelan"}, "ns")
    with pytest.raises(ValueError, match="update_where"):
        index.update_where("ns", {}, {"genre": "gamelan"})
    with pytest.raises(ValueError, match="tombstone_where"):
        index.remove_where("ns", {})
    assert index._ns["ns"].strings == strings and index.count("ns", {}) == len(vecs)


def test_update_attributes_semantics():
    index, vecs = filled()
    a, b, c = vecs[0].id, vecs[1].id, vecs[2].id
    index.remove([c], "ns")
    stranger = Vector(values=[0.0]).id
    # one mapping for every id; unknown and removed ids are skipped; a listed key with None clears, a missing key stays
    year_b = index.query_by_metadata("ns", {"year": {"$exists": True}})
    assert index.update_attributes([a, b, c, stranger], {"genre": "gamelan", "price": None}, "ns") == 2
    assert index.query_by_metadata("ns", {"genre": "gamelan"}) == [a, b]
    assert not set(index.query_by_metadata("ns", {"price": {"$exists": True}})) & {a, b}
    assert index.query_by_metadata("ns", {"year": {"$exists": True}}) == year_b
    # an id listed twice: the entries apply in order
    assert index.update_attributes([a, b, a], [{"year": 1, "in_stock": True}, {"year": 2}, {"year": 3}], "ns") == 2
    assert index.query_by_metadata("ns", {"year": 3}) == [a] and index.query_by_metadata("ns", {"year": 2}) == [b]
    assert a in index.query_by_metadata("ns", {"in_stock": True})
    assert index.count("ns", {"year": 1}) == 0
    assert index.update_attributes([a], {}, "ns") == 0


def test_update_where_is_all_or_nothing_and_sees_the_values_from_before():
    index, vecs = filled()
    ids = [v.id for v in vecs]
    index.update_attributes(ids, {"year": 2000}, "ns")
    index.update_attributes(ids[:3], [{"year": 2 ** 63 - 2}, {"year": None}, {"year": -(2 ** 63) + 2}], "ns")
    assert index.update_where("ns", {"year": {"$gte": 2000}}, {"year": 1999}) == len(ids) - 2
    assert index.update_where("ns", {"year": {"$gte": 2000}}, {"year": 1999}) == 0
    index.update_attributes(ids[:1], {"year": 2 ** 63 - 2}, "ns")
    with pytest.raises(ValueError, match="overflow on 1 of"):
        index.update_where("ns", {}, {"year": {"$inc": 2}, "genre": "gamelan"})
    assert index.count("ns", {"genre": "gamelan"}) == 0 and "gamelan" not in index._ns["ns"].strings["genre"]
    with pytest.raises(ValueError, match="overflow on 1 of"):  # INT64_MIN is the absent marker: a sum landing on it is refused
        index.update_where("ns", {}, {"year": {"$inc": -2}})
    assert index.update_where("ns", {}, {"year": {"$inc": 1}, "genre": "gamelan"}) == len(ids)
    assert index.query_by_metadata("ns", {"year": 2 ** 63 - 1}) == ids[:1]
    assert index.count("ns", {"year": 2000}) == len(ids) - 3 and index.count("ns", {"year": {"$exists": False}}) == 1
    assert index.count("ns", {"genre": "gamelan"}) == len(ids)
    index.update_attributes(ids[:2], [{"price": float("inf")}, {"price": 1.5}], "ns")
    with pytest.raises(ValueError, match="overflow"):
        index.update_where("ns", {"price": {"$exists": True}}, {"price": {"$inc": float("-inf")}})
    assert index.query_by_metadata("ns", {"price": 1.5}) == ids[1:2]
    assert index.update_where("ns", {"price": 1.5}, {"price": {"$inc": 1}}) == 1
    assert index.query_by_metadata("ns", {"price": 2.5}) == ids[1:2]


def test_remove_where_keeps_the_books_of_remove():
    index, vecs = filled(rebuild_threshold=0.5)
    twin, _ = filled(rebuild_threshold=0.5)
    f = {"year": {"$lt": 1990}}
    want = index.query_by_metadata("ns", f)
    assert 0 < len(want) < len(vecs) // 2
    assert index.remove_where("ns", f, return_ids=True) == want
    twin.remove(twin.query_by_metadata("ns", f), "ns")
    ns, tw = index._ns["ns"], twin._ns["ns"]
    assert (ns.total, ns.deleted, ns.rebuild_required) == (tw.total, tw.deleted, tw.rebuild_required) == (len(vecs), len(want), False)
    assert ns.engine.counts() == tw.engine.counts() and np.array_equal(ns.ids.live[:ns.total], tw.ids.live[:tw.total])
    assert index.remove_where("ns", f) == 0
    assert index.remove_where("ns", {}) == len(vecs) - len(want) and index.is_rebuild_required("ns")
    assert index.count("ns", {}) == 0


@pytest.mark.parametrize("seed,space", [(1, "l2"), (2, "cosine"), (3, "ip")])
def test_seeded_histories_against_the_list_of_dicts_model(seed, space):
    ran = replay_history(midx(space=space), space, seed, n_rows=120, d=6)
    assert sum(v for k, v in ran.items() if k != "refused") == 40 and len(ran) >= 4


def test_the_histories_reach_every_operation_and_a_refused_increment():
    total = {}
    for seed in (13, 18, 19):
        for k, v in replay_history(midx(), "l2", seed, n_rows=60, d=4, n_ops=30).items():
            total[k] = total.get(k, 0) + v
    assert set(total) == {"update_attributes", "update_where", "remove_where", "add", "compact", "refused"}, total


def test_save_and_load_return_the_updated_values(tmp_path):
    index, vecs = filled()
    ids = [v.id for v in vecs]
    index.update_attributes(ids[:5], {"genre": "gamelan", "year": None}, "ns")
    index.update_where("ns", {"price": {"$gte": 50}}, {"price": {"$inc": 0.5}, "in_stock": True})
    index.remove_where("ns", {"year": {"$lt": 1960}})
    assert index.save_index(str(tmp_path))
    back = Index(engine_factory=MutateOracleEngine)
    assert back.load_index(str(tmp_path))
    for f in ({"genre": "gamelan"}, {"price": {"$gte": 50.5}}, {"year": {"$exists": False}}, {"in_stock": True}, {}):
        assert back.query_by_metadata("ns", f) == index.query_by_metadata("ns", f), f
    assert back.query_by_metadata("ns", {"genre": "gamelan"}) == [u for u in ids[:5] if u in set(back.query_by_metadata("ns", {}))]
    assert back.update_where("ns", {"genre": "gamelan"}, {"genre": "jazz"}) == index.count("ns", {"genre": "gamelan"})


# ---------------------------------------------------------------- storages
@pytest.mark.parametrize("storage_type", [InMemoryStorage, ArrayStorage])
def test_storage_update_metadata_builds_a_new_dict(storage_type):
    st = storage_type()
    shared = {"a": 1, "b": 2}
    rows = [Vector(values=[1.0, 2.0], metadata=shared), Vector(values=[3.0, 4.0], metadata=shared)]
    st.write_vectors(rows, "ns")
    assert st.update_metadata(rows[0].id, {"a": None, "c": 3}, "ns")
    one, two = st.read_vectors([rows[0].id, rows[1].id], "ns")
    assert one.metadata == {"b": 2, "c": 3} and two.metadata == {"a": 1, "b": 2} and shared == {"a": 1, "b": 2}
    assert np.array_equal(one.values, [1.0, 2.0]) and one.id == rows[0].id
    assert not st.update_metadata(Vector(values=[0.0]).id, {"a": 1}, "ns")
    assert not st.update_metadata(rows[0].id, {"a": 1}, "elsewhere")
    st.delete(rows[1].id, "ns")
    assert not st.update_metadata(rows[1].id, {"a": 1}, "ns")


def test_array_storage_materialises_a_chunk_written_without_metadata():
    from mlvectordb_amd.idtable import mint_uuid4_bytes
    from uuid import UUID

    st = ArrayStorage()
    ids = mint_uuid4_bytes(6)
    st.write_arrays(ids[:3], "ns", np.zeros((3, 2), np.float32))
    st.write_arrays(ids[3:], "ns", np.ones((3, 2), np.float32), [{"k": i} for i in range(3)])
    u = [UUID(bytes=ids[i].tobytes()) for i in range(6)]
    assert st.update_metadata(u[1], {"x": 1}, "ns") and st.update_metadata(u[4], {"k": None}, "ns")
    assert [r.metadata for r in st.read_vectors(u, "ns")] == [{}, {"x": 1}, {}, {"k": 0}, {}, {"k": 2}]
    st.write_arrays(mint_uuid4_bytes(2), "ns", np.ones((2, 2), np.float32))  # after the materialised chunk: still absent
    assert [dict(m) for m in st.read_rows_at(np.arange(8), "ns")[2]] == [{}, {"x": 1}, {}, {"k": 0}, {}, {"k": 2}, {}, {}]


# ---------------------------------------------------------------- QueryProcessor
def _agree(qp, rng, f, d):
    """find_similar_many's metadata, the dict where and the equivalent predicate tell one story."""
    q = rng.standard_normal((3, d))
    strip = lambda res: [[(h["id"], h["metadata"], h["score"]) for h in row] for row in res]  # noqa: E731
    got = strip(qp.find_similar_many(q, 6, "ns", where=f))
    assert got == strip(qp.find_similar_many(q, 6, "ns", where=lambda m: py_match(f, m)))
    assert all(py_match(f, meta) for row in got for _, meta, _ in row)
    assert qp.query_by_metadata(f, "ns") == qp.query_by_metadata(lambda m: py_match(f, m), "ns")
    assert qp.count_where(f, "ns") == qp.count_where(lambda m: py_match(f, m), "ns")
    for row in strip(qp.find_similar_many(q, 6, "ns")):  # and the index holds what the storage says, row by row
        for u, meta, _ in row:
            for key, kind in SCHEMA.items():
                v = meta.get(key)
                if v is None or (kind == "float" and v != v):
                    assert u in qp.query_by_metadata({key: {"$exists": False}}, "ns"), (key, meta)
                else:
                    assert u in qp.query_by_metadata({key: v}, "ns"), (key, meta)


@pytest.mark.parametrize("storage_type", [InMemoryStorage, ArrayStorage])
def test_query_processor_updates_and_deletes_by_filter(storage_type):
    rng = np.random.default_rng(21)
    d = 6
    qp = QueryProcessor(storage_type(), midx(space="cosine"))
    qp.upsert_many([VectorDTO(values=rng.standard_normal(d).tolist(), metadata=m) for m in random_metadata(rng, 80)], "ns")
    filters = [{"year": {"$gte": 1980}}, {"genre": {"$in": ["jazz", "gamelan"]}}, {"in_stock": True}, {"price": {"$lt": 60}}]
    ids = qp.query_by_metadata({}, "ns")
    # update_metadata: declared keys reach the index, undeclared ones the storage only; None deletes / clears
    assert qp.update_metadata(ids[:4] + [Vector(values=[0.0]).id], {"genre": "gamelan", "other": "patched", "year": None}, "ns") == ids[:4]
    assert qp.query_by_metadata({"genre": "gamelan"}, "ns") == ids[:4]
    stored = qp._storage.read_vectors(ids[:5], "ns")
    assert all(v.metadata["other"] == "patched" and "year" not in v.metadata for v in stored[:4])
    assert stored[4].metadata["other"] != "patched"
    with pytest.raises(ValueError):  # the index's refusal comes before the storage is written
        qp.update_metadata(ids[:2], {"other": "never", "year": "x"}, "ns")
    assert all(v.metadata["other"] == "patched" for v in qp._storage.read_vectors(ids[:2], "ns"))
    assert qp.update_metadata(ids[5:7], [{"other": 1}, {"price": 12.5}], "ns") == ids[5:7]
    for f in filters:
        _agree(qp, rng, f, d)
    # update_where: dict filter on the device, predicate on the host, $inc per row
    f = {"year": {"$gte": 1990}}
    n = qp.count_where(f, "ns")
    years = {v.id: v.metadata.get("year") for v in qp._storage.namespace_map["ns"]}
    assert qp.update_where(f, {"year": {"$inc": -100}, "other": {"$inc": 1000}, "in_stock": False, "note": "old"}, "ns") == n > 0
    for v in qp._storage.namespace_map["ns"]:
        y = years[v.id]
        if y is not None and y >= 1990:
            assert v.metadata["year"] == y - 100 and v.metadata["other"] >= 1000 and v.metadata["note"] == "old"
            assert v.metadata["in_stock"] is False
        else:
            assert v.metadata.get("year") == y and "note" not in v.metadata
    assert qp.count_where({"year": {"$gte": 1990}}, "ns") == 0
    m = qp.update_where(lambda meta: meta.get("note") == "old", {"price": {"$inc": 0.5}, "note": None, "genre": "ska"}, "ns")
    assert m == n and qp.count_where({"genre": "ska"}, "ns") == n
    assert not any("note" in v.metadata for v in qp._storage.namespace_map["ns"])
    assert qp.update_where({"genre": "ska"}, {"other": 555}, "ns") == n  # undeclared keys only: the storage alone changes
    assert sum(v.metadata["other"] == 555 for v in qp._storage.namespace_map["ns"]) == n
    some = qp.query_by_metadata({"year": {"$exists": True}}, "ns")[:1]
    qp.update_metadata(some, {"year": 2 ** 63 - 1}, "ns")
    before = [dict(v.metadata) for v in qp._storage.namespace_map["ns"]]
    with pytest.raises(ValueError, match="overflow"):
        qp.update_where({}, {"year": {"$inc": 1}, "other": 0}, "ns")
    assert [dict(v.metadata) for v in qp._storage.namespace_map["ns"]] == before
    qp.update_metadata(some, {"year": 1900}, "ns")
    for f in filters + [{"genre": "ska"}, {"year": {"$lt": 1900}}]:
        _agree(qp, rng, f, d)
    # delete_where
    f = {"genre": "ska"}
    want = qp.query_by_metadata(f, "ns")
    assert qp.delete_where(f, "ns") == want and qp.count_where(f, "ns") == 0
    assert qp.get_namespace_count("ns") == 80 - n
    gone = qp.delete_where(lambda meta: meta.get("in_stock") is True, "ns")
    assert gone and qp.count_where({"in_stock": True}, "ns") == 0 and qp.get_namespace_count("ns") == 80 - n - len(gone)
    for f in filters:
        _agree(qp, rng, f, d)


@pytest.mark.parametrize("storage_type", [InMemoryStorage, ArrayStorage])
def test_delete_where_fires_the_compaction_trigger_exactly_as_delete_does(storage_type):
    def build():
        rng = np.random.default_rng(5)
        qp = QueryProcessor(storage_type(), midx(rebuild_threshold=0.25))
        qp.upsert_many([VectorDTO(values=rng.standard_normal(4).tolist(), metadata={"year": 1900 + i, "genre": "jazz"})
                        for i in range(40)], "ns")
        return qp

    a, b = build(), build()
    for lo, hi in ((1900, 1905), (1905, 1909), (1909, 1910), (1910, 1925)):  # 5, 9 of 40 stay below 25 %; the 10th fires it
        f = {"year": {"$gte": lo, "$lt": hi}}
        ids_b = b.query_by_metadata(f, "ns")
        assert len(a.delete_where(f, "ns")) == len(b.delete(ids_b, "ns")) == hi - lo
        na, nb = a._index._ns["ns"], b._index._ns["ns"]
        assert (na.total, na.deleted, na.rebuild_required) == (nb.total, nb.deleted, nb.rebuild_required)
        assert na.engine.counts() == nb.engine.counts()
        assert (na.total, na.deleted) == {1905: (40, 5), 1909: (40, 9), 1910: (30, 0), 1925: (15, 0)}[hi]
    assert a.count_where({}, "ns") == 15
