"""Sparse vector attributes without a GPU: the encoder, the filter compiler, ``Index`` / ``QueryProcessor`` on the model
engine, snapshots, the C entries' refusals of a null handle, and the scan kernel's resource report."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.index import Index
from mlvectordb_amd.interfaces import VectorDTO
from mlvectordb_amd.query_processor import QueryProcessor
from mlvectordb_amd.storage import InMemoryStorage
from mlvectordb_amd.vector import Vector
from tests.mutate_helpers import UntouchableEngine
from tests.sparse_helpers import SparseOracleEngine, dense_scores, legacy_index, random_corpus, random_vector, rank

ROOT = Path(__file__).resolve().parent.parent
SCHEMA = {"lexical": "sparse", "year": "int", "tags": "str[]"}


# ---------------------------------------------------------------- the encoder
def test_encoder_sorts_drops_zeros_and_tells_absent_from_empty():
    col = W.encode_sparse_column("lexical", [{7: 1.5, 2: -0.25, 9: 0.0}, None, {}, ([5, 1], [2.0, 3.0]),
                                             (np.array([4]), np.array([0.5], np.float32)), {3: 0, 4: -0.0}])
    assert col.offsets.tolist() == [0, 2, 2, 2, 4, 5, 5] and col.present.tolist() == [1, 0, 1, 1, 1, 1]
    assert col.terms.tolist() == [2, 7, 1, 5, 4] and col.weights.tolist() == [-0.25, 1.5, 3.0, 2.0, 0.5]
    assert col.terms.dtype == np.int32 and col.weights.dtype == np.float32 and col.offsets.dtype == np.int64
    assert col.row(0) == {2: -0.25, 7: 1.5} and col.row(1) is None and col.row(2) == {}
    taken = col.take([3, 1, 0])
    assert taken.offsets.tolist() == [0, 2, 2, 4] and taken.terms.tolist() == [1, 5, 2, 7] and taken.present.tolist() == [1, 0, 1]
    ends = W.encode_sparse_column("lexical", [{0: 1.0, 2 ** 31 - 1: 2.0}])
    assert ends.terms.tolist() == [0, 2 ** 31 - 1]
    assert W.encode_sparse_column("lexical", []).offsets.tolist() == [0]


@pytest.mark.parametrize("value, match", [
    (([1, 1], [1.0, 2.0]), "appears twice"),
    ({-1: 1.0}, r"outside \[0, 2\^31\)"),
    ({2 ** 31: 1.0}, r"outside \[0, 2\^31\)"),
    ({1.5: 1.0}, "not an integer"),
    ({"a": 1.0}, "not an integer"),
    ({True: 1.0}, "not an integer"),
    ({1: float("nan")}, "finite"),
    ({1: float("inf")}, "finite"),
    ({1: 1e39}, "finite"),  # finite as a double, not as the float32 the column holds
    ({1: "x"}, "not a number"),
    (([1, 2], [1.0]), "2 indices but 1 values"),
    (5, "not a mapping"),
    ({t: 1.0 for t in range(256)}, "256 nonzeros"),
])
def test_encoder_refusals(value, match):
    with pytest.raises(ValueError, match=match):
        W.encode_sparse_column("lexical", [{1: 1.0}, value])


def test_encoder_takes_255_nonzeros_and_zeros_do_not_count():
    row = {t: 1.0 for t in range(255)}
    row.update({t: 0.0 for t in range(300, 400)})
    assert W.encode_sparse_column("lexical", [row]).terms.size == 255


# ---------------------------------------------------------------- filters
def test_filters_on_a_sparse_attribute_compile_to_exists_and_len():
    def ops(where):
        return [tuple(o) for o in W.compile_where(where, SCHEMA, {}).ops.tolist()]
    assert ops({"lexical": {"$exists": True}}) == [(W.EXISTS, 0, 0, 0)]
    assert ops({"lexical": {"$exists": False}}) == [(W.EXISTS, 0, 0, 0), (W.NOT, 0, 0, 0)]
    assert ops({"lexical": {"$size": 3}}) == [(W.LEN, 0, 3, 3)]
    assert ops({"lexical": {"$size": {"$gte": 2, "$lt": 17}}}) == [(W.LEN, 0, 2, 16)]
    assert ops({"lexical": {"$size": 0}, "year": 3}) == [(W.LEN, 0, 0, 0), (W.EQ, 1, 3, 0), (W.AND, 0, 0, 0)]
    assert W.column_kind("sparse") == "sparse" and W.is_pooled("sparse") and not W.is_list("sparse")


@pytest.mark.parametrize("where", [
    {"lexical": 3}, {"lexical": {"$eq": 3}}, {"lexical": {"$ne": 3}}, {"lexical": {"$in": [1]}}, {"lexical": {"$nin": [1]}},
    {"lexical": {"$all": [1]}}, {"lexical": {"$lt": 1}}, {"lexical": {"$gte": 1}}, {"lexical": {3: 1.0}},
    {"lexical": {"$size": "x"}}, {"lexical": {"$exists": 1}}, {"year": {"$size": 1}},
])
def test_filter_refusals(where):
    with pytest.raises(ValueError):
        W.compile_where(where, SCHEMA, {})


# ---------------------------------------------------------------- Index and QueryProcessor on the model engine
def _index(schema=SCHEMA, engine=SparseOracleEngine):
    return Index(space="cosine", engine_factory=lambda dim, sp: engine(dim, sp), attributes=schema)


def _filled(seed=5, n=160, vocab=48):
    rng = np.random.default_rng(seed)
    rows = random_corpus(rng, n, vocab, exact=True)
    metas = [{"lexical": r, "year": 2000 + i % 7, "tags": ["a"] if i % 2 else []} for i, r in enumerate(rows)]
    for m in metas[::13]:
        del m["lexical"]  # a missing key is absent too
    vectors = [Vector(values=rng.standard_normal(8).astype(np.float32).tolist(), metadata=m) for m in metas]
    index = _index()
    index.add(vectors[:100], "ns")
    index.add(vectors[100:], "ns")
    return rng, index, vectors, metas


def _expect(queries, vectors, metas, live, k, keep=lambda m: True):
    """The model's answer straight from the metadata dicts: [(id, score)] per query."""
    rows = [m.get("lexical") for m in metas]
    clean = [None if r is None else {t: w for t, w in r.items() if w != 0} for r in rows]
    scores, _ = dense_scores(queries, clean)
    cand = np.array([live[i] and clean[i] is not None and keep(metas[i]) for i in range(len(metas))], dtype=bool)
    labels, s64, counts = rank(scores, cand, k)
    return [[(vectors[l].id, s) for l, s in zip(labels[q, :counts[q]].tolist(), s64[q, :counts[q]].tolist())]
            for q in range(len(queries))]


def test_index_search_sparse_against_the_metadata():
    rng, index, vectors, metas = _filled()
    live = [True] * len(vectors)
    queries = [random_vector(rng, n, 48, exact=True) for n in (1, 3, 8, 20)] + [{}]

    def check(where=None, keep=lambda m: True, k=10):
        got = index.search_sparse(queries, k, "ns", "lexical", where=where)
        want = _expect(queries, vectors, metas, live, min(k, 64), keep)  # (top_k is clamped to the list's length)
        assert [[(h.vector_id, h.score) for h in hits] for hits in got] == want
        assert got.scores.dtype == np.float64
        return got

    check()
    check({"year": {"$gte": 2003}}, lambda m: m["year"] >= 2003)
    check({"lexical": {"$size": {"$gte": 1, "$lt": 16}}}, lambda m: m.get("lexical") is not None and 1 <= len(m["lexical"]) < 16)
    check({"tags": "a"}, lambda m: "a" in m["tags"], k=64)
    assert check(k=1000).labels.shape[1] == 64  # clamped like search_many clamps: to the live rows and to the list's length
    index.remove([v.id for v in vectors[::5]], "ns")
    live = [i % 5 != 0 for i in range(len(vectors))]
    check()
    # pairs (indices, values) are the same queries
    pairs = [(list(q), list(q.values())) for q in queries]
    assert index.search_sparse(pairs, 10, "ns", "lexical") == index.search_sparse(queries, 10, "ns", "lexical")
    # updates by id: a new vector, an empty one, none
    ids = [vectors[1].id, vectors[2].id, vectors[3].id]
    new = [{"lexical": {4: 2.0, 1: -1.0}}, {"lexical": {}}, {"lexical": None}]
    assert index.update_attributes(ids, new, "ns") == 3
    for i, p in zip((1, 2, 3), new):
        metas[i]["lexical"] = p["lexical"]
    check()
    assert index.count("ns", {"lexical": {"$exists": True}}) == sum(live[i] and m.get("lexical") is not None
                                                                    for i, m in enumerate(metas))
    assert index.compact("ns")
    vectors = [v for i, v in enumerate(vectors) if live[i]]
    metas = [m for i, m in enumerate(metas) if live[i]]
    live = [True] * len(vectors)
    check()
    assert index.search_sparse([], 5, "ns", "lexical").labels.shape[0] == 0
    assert index.search_sparse(queries, 5, "nowhere", "lexical") == [[] for _ in queries]


def test_refusals_happen_before_anything_is_mutated():
    index = _index(engine=UntouchableEngine)
    good = Vector(values=[1.0, 2.0], metadata={"lexical": {1: 1.0}})
    for bad in ({1: float("nan")}, ([1, 1], [1.0, 1.0]), {-3: 1.0}, {t: 1.0 for t in range(256)}, {1.5: 2.0}):
        with pytest.raises(ValueError):
            index.add([good, Vector(values=[1.0, 2.0], metadata={"lexical": bad})], "ns")
    assert index.namespace_counts("ns") is None or index.namespace_counts("ns")[0] == 0
    rng, index, vectors, metas = _filled(n=40)
    before = index.search_sparse([{1: 1.0, 5: 2.0}], 64, "ns", "lexical")
    with pytest.raises(ValueError, match="finite"):
        index.update_attributes([vectors[0].id, vectors[1].id], [{"lexical": {1: 1.0}}, {"lexical": {2: float("inf")}}], "ns")
    with pytest.raises(ValueError, match="sparse attribute"):
        index.update_where("ns", {"year": 2001}, {"lexical": {1: 1.0}})
    with pytest.raises(ValueError, match="sparse attribute"):
        index.update_where("ns", {"year": 2001}, {"year": 5, "lexical": None})
    assert index.search_sparse([{1: 1.0, 5: 2.0}], 64, "ns", "lexical") == before
    assert index.count("ns", {"year": 5}) == 0
    for call in (lambda: index.facets("ns", "lexical"), lambda: index.facets("ns", ["year", "lexical"]),
                 lambda: index.top_by("ns", "lexical", 3), lambda: index.histogram("ns", "lexical", [1, 2]),
                 lambda: index.search_many(np.zeros((1, 8), np.float32), 3, "ns", "cosine", distinct="lexical"),
                 lambda: index.search_late([np.zeros((1, 8), np.float32)], 3, "ns", "cosine", "lexical")):
        with pytest.raises(ValueError, match="sparse column"):
            call()
    for kw, match in ((dict(by="year"), "needs a sparse attribute"), (dict(by="nope"), "not a declared attribute"),
                      (dict(by="lexical", where=[{}]), "one dict filter"), (dict(by="lexical", where={"lexical": 3}), "sparse")):
        with pytest.raises(ValueError, match=match):
            index.search_sparse([{1: 1.0}], 3, "ns", **kw)
    for q, match in (({1: float("nan")}, "finite"), ({t: 1.0 for t in range(1025)}, "1025 nonzeros"), ({-1: 1.0}, "outside")):
        with pytest.raises(ValueError, match=match):
            index.search_sparse([{1: 1.0}, q], 3, "ns", "lexical")
    with pytest.raises(ValueError, match="wrap it in a list"):
        index.search_sparse({1: 1.0}, 3, "ns", "lexical")
    assert len(index.search_sparse([{t: 1.0 for t in range(1024)}], 3, "ns", "lexical")[0]) == 3


def test_sparse_attributes_on_a_row_sharded_index_are_refused():
    with pytest.raises(ValueError, match="row-sharded"):
        Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine, attributes={"lexical": "sparse"})
    with pytest.raises(ValueError, match="is not one of"):
        Index(attributes={"lexical": "sparse[]"})


def test_query_processor_find_similar_sparse():
    rng = np.random.default_rng(9)
    qp = QueryProcessor(InMemoryStorage(), _index(schema={"lexical": "sparse", "year": "int"}))
    metas = [{"lexical": {1: 1.0, 2: 0.5}, "year": 1, "note": "x"}, {"lexical": {2: 2.0}, "year": 2}, {"lexical": {}, "year": 3},
             {"year": 4}, {"lexical": {1: -1.0}, "year": 5}]
    qp.upsert_many([VectorDTO(values=rng.standard_normal(8).tolist(), metadata=m) for m in metas])
    got = qp.find_similar_sparse({1: 2.0, 2: 1.0}, 10, by="lexical")
    assert [(h["metadata"]["year"], h["score"]) for h in got] == [(1, 2.5), (2, 2.0), (3, 0.0), (5, -2.0)]
    assert set(got[0]) == {"id", "values", "metadata", "score"} and got[0]["metadata"]["note"] == "x"
    many = qp.find_similar_sparse_many([{2: 1.0}, ([1], [1.0])], 2, by="lexical", where={"year": {"$lt": 5}})
    assert [[h["metadata"]["year"] for h in hits] for hits in many] == [[2, 1], [1, 2]]
    with pytest.raises(ValueError, match="one dict filter"):
        qp.find_similar_sparse({1: 1.0}, 3, by="lexical", where=lambda m: True)
    ids = qp.query_by_metadata({})
    qp.update_metadata([ids[3]], {"lexical": {2: 8.0}})
    assert qp.find_similar_sparse({2: 1.0}, 1, by="lexical")[0]["metadata"] == {"year": 4, "lexical": {2: 8.0}}


# ---------------------------------------------------------------- snapshots
def _sha(path):
    return {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(Path(path).iterdir()) if p.is_file()}


def test_v4_snapshot_round_trip(tmp_path):
    rng, index, vectors, metas = _filled(seed=12, n=90)
    index.remove([v.id for v in vectors[::7]], "ns")
    index.update_attributes([vectors[1].id, vectors[2].id], [{"lexical": {}}, {"lexical": None}], "ns")  # leaves garbage behind
    metas[1]["lexical"], metas[2]["lexical"] = {}, None
    index.save_index(str(tmp_path))
    manifest = json.loads((tmp_path / "index.json").read_text())
    assert manifest["format"] == "mlvdb-index-v4" and manifest["attributes"] == SCHEMA
    names = {p.name for p in tmp_path.iterdir()}
    assert {"ns0.attr0.i64", "ns0.attr0.offsets.i64", "ns0.attr0.terms.i32", "ns0.attr0.weights.f32", "ns0.attr1.i64",
            "ns0.attr2.values.i64"} <= names
    live = [m for i, m in enumerate(metas) if i % 7]
    nnz = sum(len(m.get("lexical") or ()) for m in live)  # the live CSR: exactly what the live rows hold
    assert (tmp_path / "ns0.attr0.terms.i32").stat().st_size == 4 * nnz == (tmp_path / "ns0.attr0.weights.f32").stat().st_size
    lens = np.fromfile(tmp_path / "ns0.attr0.i64", dtype=np.int64)
    assert lens.tolist() == [len(m["lexical"]) if i % 7 and m.get("lexical") is not None else W.INT64_ABSENT
                             for i, m in enumerate(metas)]
    loaded = _index(schema={})
    assert loaded.load_index(str(tmp_path)) and loaded.attributes == SCHEMA
    queries = [random_vector(rng, n, 48, exact=True) for n in (2, 9, 30)]
    for where in (None, {"year": {"$lt": 2004}}, {"lexical": {"$size": {"$gte": 3}}}):
        a = index.search_sparse(queries, 20, "ns", "lexical", where=where)
        b = loaded.search_sparse(queries, 20, "ns", "lexical", where=where)
        assert a == b and a.scores.tobytes() == b.scores.tobytes() and a.counts.sum() > 0
    loaded.save_index(str(tmp_path / "again"))
    assert _sha(tmp_path / "again") == _sha(tmp_path)
    (tmp_path / "ns0.attr0.terms.i32").unlink()
    with pytest.raises(RuntimeError, match="sparse attribute files"):
        _index(schema={}).load_index(str(tmp_path))


# sha256 of every file ``sparse_helpers.legacy_index`` saved with the code from before sparse attributes existed
LEGACY = {
    "v1": {
        "index.json": "9fed6633197aa0d7b022a4ee5ed1df624ede755431b476e5eb9a642326cb5844",
        "ns0.deleted.i64": "ad3bc4b1b5506d22ac3279e13227c91d4845a45702c4a5c1b842b302efe0c617",
        "ns0.ids.u8": "3594cb7f3b4007f6ac426c33a8fbcc8a7acbefb9584638aecf54c92ebf8e414f",
        "ns0.rows.f32": "44c3cbfe4c82d3e1007eeed80ba443453e71a50aaba74570f39790c502b7befd",
    },
    "v2": {
        "index.json": "9e095e0b7c7b4f5940773a8ac256782e163ebc90efe0c03a0393a248c715723e",
        "ns0.attr0.i64": "4257e2c49ad631da105851e2dabcc0dc3a7adf0f20ead2b1e869aa5a2aa3c7a4",
        "ns0.attr1.i64": "3ff5e7e79924ae21ce541cd5f19472ca9397c16e232e9a05b44c342d8232c24d",
        "ns0.attr2.f64": "69f603e3e26edcd482b9ff8673821023c6763325810ab6c656820b3f45db19d2",
        "ns0.deleted.i64": "ad3bc4b1b5506d22ac3279e13227c91d4845a45702c4a5c1b842b302efe0c617",
        "ns0.ids.u8": "3594cb7f3b4007f6ac426c33a8fbcc8a7acbefb9584638aecf54c92ebf8e414f",
        "ns0.rows.f32": "44c3cbfe4c82d3e1007eeed80ba443453e71a50aaba74570f39790c502b7befd",
    },
    "v3": {
        "index.json": "6591ab88453c62daf8bc29ed62ce613398a56d383a47e3f1a59e2e5e4d743745",
        "ns0.attr0.i64": "4257e2c49ad631da105851e2dabcc0dc3a7adf0f20ead2b1e869aa5a2aa3c7a4",
        "ns0.attr1.i64": "361d156e55872ce10700d6ca3e15c59ffcb978f22deb9dd324d068cb9fa55fb6",
        "ns0.attr1.offsets.i64": "df6cadcbc6276878ce3d50b6a0e7f2937dee31be42204d722c9dbd2cf74c6ad8",
        "ns0.attr1.values.i64": "37a2ce90ce1c966bc3a9c609e3c651ae1d2c5f9c61b4fbb69f755ece1787227c",
        "ns0.attr2.i64": "6bf0d47cf1a318cff0c5aaa30c13de3aebc622b106b35046156749221e4891b6",
        "ns0.attr2.offsets.i64": "67c1b08a8e4eb7f472020349b2b6bdfc95fb3646ad52224e791446012d598279",
        "ns0.attr2.values.i64": "8626de6ed476699bc194894be679aade2c5c9f5b656a6a975b096af69d73aa41",
        "ns0.attr3.f64": "69f603e3e26edcd482b9ff8673821023c6763325810ab6c656820b3f45db19d2",
        "ns0.deleted.i64": "ad3bc4b1b5506d22ac3279e13227c91d4845a45702c4a5c1b842b302efe0c617",
        "ns0.ids.u8": "3594cb7f3b4007f6ac426c33a8fbcc8a7acbefb9584638aecf54c92ebf8e414f",
        "ns0.rows.f32": "44c3cbfe4c82d3e1007eeed80ba443453e71a50aaba74570f39790c502b7befd",
    },
}


@pytest.mark.parametrize("version", ["v1", "v2", "v3"])
def test_snapshots_without_sparse_attributes_are_byte_identical_to_before(tmp_path, version):
    legacy_index(version).save_index(str(tmp_path))
    assert json.loads((tmp_path / "index.json").read_text())["format"] == f"mlvdb-index-{version}"
    assert _sha(tmp_path) == LEGACY[version]
    loaded = Index(space="cosine", engine_factory=lambda dim, sp: SparseOracleEngine(dim, sp))
    assert loaded.load_index(str(tmp_path))
    loaded.save_index(str(tmp_path / "again"))
    assert _sha(tmp_path / "again") == LEGACY[version]


# ---------------------------------------------------------------- the C ABI without a device
def test_sparse_entries_are_declared_bound_and_refuse_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_sparse.h").read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(_native.SPARSE_SIGNATURES) and len(names) == 4
    others = [t for n, t in vars(_native).items() if n.endswith("SIGNATURES") and n != "SPARSE_SIGNATURES"]
    assert not any(set(names) & set(t) for t in others)
    for name in names:  # the parameter count of each prototype is the binding's
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert len(params) == len(_native.SPARSE_SIGNATURES[name][1]), name
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert int(consts["MLVDB_ATTR_SPARSE"]) == _native.ATTR_SPARSE == _native.LIST_ATTR_CODES["sparse"] == 4
    assert int(consts["MLVDB_SPARSE_MAX_QUERY_TERMS"]) == _native.SPARSE_MAX_QUERY_TERMS == W.SPARSE_MAX_QUERY_TERMS == 1024
    assert _native.SPARSE_MAX_NNZ == W.SPARSE_MAX_NNZ == _native.LIST_MAX_LEN == 255
    lib = _native.load()
    assert lib.mlvdb_abi_version() == 7 == _native.ABI_VERSION
    null, z, buf = C.c_void_p(), C.c_int64(0), (C.c_int64 * 4)()
    calls = {
        "mlvdb_sparse_set": (null, 0, 0, 1, buf, buf, buf, None),
        "mlvdb_sparse_set_at": (null, 0, buf, 1, buf, buf, buf, None, C.byref(z)),
        "mlvdb_sparse_get": (null, 0, 0, 1, buf, buf, buf, None, 4, C.byref(z)),
        "mlvdb_search_batch_sparse": (null, 0, buf, buf, buf, 1, 1, None, buf, buf, buf, None),
    }
    assert sorted(calls) == names
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 1, name  # MLVDB_ERR_INVALID_ARG
        assert b"null index handle" in lib.mlvdb_last_global_error(), name


def test_every_new_entry_is_guarded():
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    for name in _native.SPARSE_SIGNATURES:
        body = re.search(r"^int " + name + r"\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
        assert body.lstrip().startswith("return guarded("), name


# ---------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_sparse_kernels_use_no_scratch(tmp_path):
    """DESIGN 11.13 records the VGPR, SGPR and LDS figures this report gives."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "mlvectordb_amd" / "csrc"
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(csrc / "kernels_sparse.hip"), "-o",
                          str(tmp_path / "k.o")], capture_output=True, text=True, cwd=csrc, check=True).stderr
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    # (the merge is the exact scan's, instantiated in this unit with the signs turned back: exact_merge_kernel<true>)
    for kernel in ("sparse_scan_kernel", "exact_merge_kernelILb1E"):
        hits = [v for k, v in seen.items() if kernel in k]
        assert hits and all(v == 0 for v in hits), (kernel, seen)
