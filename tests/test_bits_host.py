"""Binary vector attributes without a GPU: the encoder, the filter compiler, ``Index`` / ``QueryProcessor`` on the model
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
from tests import geo_helpers
from tests.bits_helpers import BitsOracleEngine, distances, legacy_index, near, random_codes, unpack
from tests.mutate_helpers import UntouchableEngine

ROOT = Path(__file__).resolve().parent.parent
SCHEMA = {"sig": "bits128", "year": "int", "tags": "str[]"}


def forms(words):
    """One code (uint64 words) in its three value forms: bytes, a uint8 array, a bool array."""
    raw = np.asarray(words, dtype="<u8").tobytes()
    return raw, np.frombuffer(raw, dtype=np.uint8), unpack(np.asarray(words, np.uint64)[None, :])[0].astype(bool)


# ---------------------------------------------------------------- the encoder
def test_the_three_forms_of_a_code_give_the_same_words():
    rng = np.random.default_rng(1)
    for nbits in (64, 128, 320, 16320):
        words = rng.integers(0, 2 ** 64, size=nbits // 64, dtype=np.uint64)
        raw, u8, bits = forms(words)
        assert len(raw) == nbits // 8 and u8.size == nbits // 8 and bits.size == nbits
        for value in (raw, bytearray(raw), u8, bits, bits.astype(np.uint8), bits.astype(np.int64), bits.tolist(),
                      [int(b) for b in bits]):
            got = W.encode_bits_code(value, nbits, "x")
            assert got.dtype == np.uint64 and got.tolist() == words.tolist(), type(value)
    # word w holds bits 64w .. 64w + 63: bit 0 is the lowest bit of word 0, bit 64 the lowest of word 1
    one = np.zeros(128, dtype=bool)
    one[0] = one[64 + 3] = True
    assert W.encode_bits_code(one, 128, "x").tolist() == [1, 8]
    assert W.encode_bits_code(bytes([1] + [0] * 15), 128, "x").tolist() == [1, 0]  # little-endian words
    assert W.encode_bits_code(bytes([0] * 7 + [0x80] + [0] * 8), 128, "x").tolist() == [1 << 63, 0]


def test_a_column_tells_absent_rows_and_takes_rows():
    rng = np.random.default_rng(2)
    words = rng.integers(0, 2 ** 64, size=(3, 2), dtype=np.uint64)
    col = W.encode_bits_column("sig", "bits128", [forms(words[0])[0], None, forms(words[2])[2]])
    assert col.present.tolist() == [1, 0, 1] and col.words.dtype == np.uint64 and col.words.shape == (3, 2)
    assert col.words[0].tolist() == words[0].tolist() and col.words[2].tolist() == words[2].tolist() and not col.words[1].any()
    assert col.row(0) == forms(words[0])[0] and col.row(1) is None and len(col) == 3
    taken = col.take([2, 1])
    assert taken.present.tolist() == [1, 0] and taken.words[0].tolist() == words[2].tolist()
    assert len(W.encode_bits_column("sig", "bits128", [])) == 0


@pytest.mark.parametrize("value, match", [
    (b"\x00" * 15, "15 bytes"),
    (b"\x00" * 17, "17 bytes"),
    (np.zeros(15, np.uint8), "15 entries"),
    (np.zeros(127, bool), "127 entries"),
    (np.zeros(129, bool), "129 entries"),
    (np.zeros(16, np.int64), "16 entries"),  # bytes come as uint8 only: an int64 array is a bit array, and too short
    (np.full(128, 2, np.uint8), "0 and 1 only"),
    (np.full(128, -1, np.int64), "0 and 1 only"),
    (np.zeros(128, np.float32), "dtype float32"),
    (np.zeros((2, 64), bool), r"shape \(2, 64\)"),
    ("ab" * 8, "not a bit code"),
    ({1: 1.0}, "not a bit code"),
    (5, "shape"),
])
def test_encoder_refusals(value, match):
    with pytest.raises(ValueError, match=match):
        W.encode_bits_column("sig", "bits128", [b"\x01" * 16, value])


def test_width_parsing():
    for kind, n in (("bits64", 64), ("bits128", 128), ("bits16320", 16320)):
        assert W.is_bits(kind) and W.bits_width(kind) == n and W.is_pooled(kind) and W.column_kind(kind) == "bits"
        assert not W.is_list(kind) and not W.is_sparse(kind) and not W.is_geo(kind)
    for kind in ("bits0", "bits100", "bits16384", "bits", "bits-64", "bits64 ", "bits064", "Bits64", "bits64[]", "bits6.4e1"):
        assert not W.is_bits(kind) and not W.is_pooled(kind), kind
        with pytest.raises(ValueError, match="not a bits type"):
            W.bits_width(kind)
    assert W.BITS_MAX_WORDS == _native.BITS_MAX_WORDS == 255 and 64 * W.BITS_MAX_WORDS == 16320
    for kind in ("bits0", "bits100", "bits16384"):
        with pytest.raises(ValueError, match="is not one of"):
            Index(attributes={"sig": kind})
    assert Index(attributes={"a": "bits64", "b": "bits16320"}, engine_factory=UntouchableEngine).attributes == \
        {"a": "bits64", "b": "bits16320"}


# ---------------------------------------------------------------- filters
def test_filters_on_a_bits_attribute_compile_to_exists():
    def ops(where):
        return [tuple(o) for o in W.compile_where(where, SCHEMA, {}).ops.tolist()]
    assert ops({"sig": {"$exists": True}}) == [(W.EXISTS, 0, 0, 0)]
    assert ops({"sig": {"$exists": False}}) == [(W.EXISTS, 0, 0, 0), (W.NOT, 0, 0, 0)]
    assert ops({"sig": {"$exists": True}, "year": 3}) == [(W.EXISTS, 0, 0, 0), (W.EQ, 1, 3, 0), (W.AND, 0, 0, 0)]


@pytest.mark.parametrize("where", [
    {"sig": b"\x00" * 16}, {"sig": 3}, {"sig": {"$eq": 3}}, {"sig": {"$ne": 3}}, {"sig": {"$in": [1]}}, {"sig": {"$nin": [1]}},
    {"sig": {"$all": [1]}}, {"sig": {"$size": 2}}, {"sig": {"$lt": 1}}, {"sig": {"$gte": 1}}, {"sig": {"$exists": 1}},
    {"sig": {"$geo_radius": {"center": (0, 0), "radius": 1}}}, {"sig": {"$geo_box": {"sw": (0, 0), "ne": (1, 1)}}},
])
def test_filter_refusals(where):
    with pytest.raises(ValueError):
        W.compile_where(where, SCHEMA, {})


# ---------------------------------------------------------------- Index and QueryProcessor on the model engine
def _index(schema=SCHEMA, engine=BitsOracleEngine):
    return Index(space="cosine", engine_factory=lambda dim, sp: engine(dim, sp), attributes=schema)


def _filled(seed=5, n=160):
    rng = np.random.default_rng(seed)
    codes, base = random_codes(rng, n, 2, alphabet=6)
    metas = [{"sig": forms(c)[i % 3], "year": 2000 + i % 7, "tags": ["a"] if i % 2 else []} for i, c in enumerate(codes)]
    for m in metas[::13]:
        del m["sig"]  # a missing key is absent too
    for m in metas[5::17]:
        m["sig"] = None
    vectors = [Vector(values=rng.standard_normal(8).astype(np.float32).tolist(), metadata=m) for m in metas]
    index = _index()
    index.add(vectors[:100], "ns")
    index.add(vectors[100:], "ns")
    return rng, index, vectors, metas, base


def _expect(queries, vectors, metas, live, k, metric, keep=lambda m: True):
    """The model's answer straight from the metadata dicts: [(id, distance)] per query."""
    rows = [i for i, m in enumerate(metas) if live[i] and m.get("sig") is not None and keep(m)]
    codes = np.array([W.encode_bits_code(metas[i]["sig"], 128, "x") for i in rows], dtype=np.uint64).reshape(len(rows), 2)
    dist = distances(np.asarray(queries, np.uint64), codes, metric)
    out = []
    for q in range(len(queries)):
        order = np.lexsort((np.array(rows), dist[q]))[:k]
        out.append([(vectors[rows[j]].id, float(dist[q, j])) for j in order.tolist()])
    return out


def test_index_search_bits_against_the_metadata():
    rng, index, vectors, metas, base = _filled()
    live = [True] * len(vectors)
    queries = np.stack([base[0], base[1], base[3], near(rng, base[4], 3), rng.integers(0, 2 ** 64, 2, dtype=np.uint64)])

    def check(where=None, keep=lambda m: True, k=10, metric="hamming"):
        got = index.search_bits([forms(q)[0] for q in queries], k, "ns", "sig", metric=metric, where=where)
        want = _expect(queries, vectors, metas, live, min(k, 64), metric, keep)  # (top_k is clamped to the list's length)
        assert [[(h.vector_id, h.score) for h in hits] for hits in got] == want
        assert got.scores.dtype == np.float64
        return got

    for metric in ("hamming", "jaccard"):
        check(metric=metric)
        check({"year": {"$gte": 2003}}, lambda m: m["year"] >= 2003, metric=metric)
        check({"tags": "a", "sig": {"$exists": True}}, lambda m: "a" in m["tags"], k=64, metric=metric)
    assert check(k=1000).labels.shape[1] == 64  # clamped like search_many clamps: to the live rows and to the list's length
    ties = check(k=64).scores[0]
    assert (np.diff(ties[np.isfinite(ties)]) == 0).sum() > 10  # the alphabet's groups: the label decides inside them
    index.remove([v.id for v in vectors[::5]], "ns")
    live = [i % 5 != 0 for i in range(len(vectors))]
    check()
    # every form of the queries is the same queries
    a = index.search_bits([forms(q)[0] for q in queries], 10, "ns", "sig")
    assert index.search_bits([forms(q)[1] for q in queries], 10, "ns", "sig") == a
    assert index.search_bits([forms(q)[2] for q in queries], 10, "ns", "sig") == a
    assert index.search_bits(np.stack([forms(q)[1] for q in queries]), 10, "ns", "sig") == a  # uint8 [nq, N / 8]
    assert index.search_bits(np.stack([forms(q)[2] for q in queries]), 10, "ns", "sig") == a  # bool [nq, N]
    # updates by id: a new code, none
    ids = [vectors[1].id, vectors[2].id, vectors[3].id]
    new = [{"sig": forms(base[2])[0]}, {"sig": None}, {"sig": forms(queries[4])[2], "year": 1999}]
    assert index.update_attributes(ids, new, "ns") == 3
    for i, p in zip((1, 2, 3), new):
        metas[i].update(p)
    check()
    check(metric="jaccard")
    assert index.count("ns", {"sig": {"$exists": True}}) == sum(live[i] and m.get("sig") is not None for i, m in enumerate(metas))
    assert index.remove_where("ns", {"year": 2006}) > 0
    live = [ok and m["year"] != 2006 for ok, m in zip(live, metas)]
    check()
    assert index.compact("ns")
    vectors = [v for i, v in enumerate(vectors) if live[i]]
    metas = [m for i, m in enumerate(metas) if live[i]]
    live = [True] * len(vectors)
    check()
    check(metric="jaccard")
    assert index.search_bits([], 5, "ns", "sig").labels.shape[0] == 0
    assert index.search_bits([forms(q)[0] for q in queries], 5, "nowhere", "sig") == [[] for _ in queries]


def test_refusals_happen_before_anything_is_mutated():
    index = _index(engine=UntouchableEngine)
    good = Vector(values=[1.0, 2.0], metadata={"sig": b"\x01" * 16})
    for bad in (b"\x01" * 15, np.zeros(64, bool), np.full(128, 2), np.zeros(128, np.float64), "x", 7):
        with pytest.raises(ValueError):
            index.add([good, good, Vector(values=[1.0, 2.0], metadata={"sig": bad})], "ns")  # the last vector is the bad one
        with pytest.raises(ValueError):
            index.add_arrays(np.ones((2, 2), np.float32), "ns", attributes={"sig": [b"\x01" * 16, bad]})
    assert index.namespace_counts("ns") is None or index.namespace_counts("ns")[0] == 0
    rng, index, vectors, metas, base = _filled(n=40)
    probe = [forms(base[1])[0], forms(base[3])[2]]
    before = index.search_bits(probe, 64, "ns", "sig")
    total = index.namespace_counts("ns")
    with pytest.raises(ValueError, match="15 bytes"):
        index.add([Vector(values=[0.0] * 8, metadata={"sig": b"\x01" * 16}), Vector(values=[0.0] * 8, metadata={"sig": b"\x01" * 15})],
                  "ns")
    with pytest.raises(ValueError, match="17 bytes"):
        index.update_attributes([vectors[0].id, vectors[1].id], [{"sig": b"\x00" * 16}, {"sig": b"\x00" * 17}], "ns")
    with pytest.raises(ValueError, match="bits128 attribute"):
        index.update_where("ns", {"year": 2001}, {"sig": b"\x00" * 16})
    with pytest.raises(ValueError, match="bits128 attribute"):
        index.update_where("ns", {"year": 2001}, {"year": 5, "sig": None})
    after = index.search_bits(probe, 64, "ns", "sig")
    assert after == before and after.scores.tobytes() == before.scores.tobytes() and index.namespace_counts("ns") == total
    assert index.count("ns", {"year": 5}) == 0
    zero = np.zeros((1, 8), np.float32)
    for call in (lambda: index.facets("ns", "sig"), lambda: index.facets("ns", ["year", "sig"]),
                 lambda: index.top_by("ns", "sig", 3), lambda: index.histogram("ns", "sig", [1, 2]),
                 lambda: index.stats("ns", "sig"), lambda: index.stats("ns", "year", by="sig"),
                 lambda: index.search_many(zero, 3, "ns", "cosine", distinct="sig"),
                 lambda: index.search_late([zero], 3, "ns", "cosine", "sig")):
        with pytest.raises(ValueError, match="bits128 column"):
            call()
    for call in (lambda: index.nearest("ns", "sig", (0.0, 0.0), 3), lambda: index.search_sparse([{1: 1.0}], 3, "ns", "sig"),
                 lambda: index.search_hybrid(zero, [{1: 1.0}], 3, "ns", "cosine", "sig")):
        with pytest.raises(ValueError, match="bits128"):
            call()
    for kw, match in ((dict(by="year"), "needs a bits attribute"), (dict(by="nope"), "not a declared attribute"),
                      (dict(by="sig", where=[{}]), "one dict filter"), (dict(by="sig", where={"sig": 3}), "bits128"),
                      (dict(by="sig", metric="l2"), "metric must be one of")):
        with pytest.raises(ValueError, match=match):
            index.search_bits([b"\x00" * 16], 3, "ns", **kw)
    for q, match in ((b"\x00" * 8, "8 bytes"), (np.zeros(64, bool), "64 entries"), (np.zeros(128), "dtype float64")):
        with pytest.raises(ValueError, match="search_bits: query 1: .*" + match):
            index.search_bits([b"\x00" * 16, q], 3, "ns", "sig")
    for single in (b"\x00" * 16, np.zeros(16, np.uint8), np.zeros(128, bool)):
        with pytest.raises(ValueError, match="wrap it in a list"):
            index.search_bits(single, 3, "ns", "sig")


def test_bits_attributes_on_a_row_sharded_index_are_refused():
    with pytest.raises(ValueError, match="row-sharded"):
        Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine, attributes={"sig": "bits64"})


def test_query_processor_find_similar_bits():
    rng = np.random.default_rng(9)
    qp = QueryProcessor(InMemoryStorage(), _index(schema={"sig": "bits64", "year": "int"}))

    def code(*bits):
        out = np.zeros(64, dtype=bool)
        out[list(bits)] = True
        return out

    metas = [{"sig": code(0, 1, 2), "year": 1, "note": "x"}, {"sig": code(0, 1), "year": 2}, {"sig": code(), "year": 3},
             {"year": 4}, {"sig": code(5, 6, 7, 8), "year": 5}]
    qp.upsert_many([VectorDTO(values=rng.standard_normal(8).tolist(),
                              metadata={**m, **({"sig": m["sig"].tolist()} if "sig" in m else {})}) for m in metas])
    got = qp.find_similar_bits(code(0, 1, 2), 10, by="sig")
    assert [(h["metadata"]["year"], h["score"]) for h in got] == [(1, 0.0), (2, 1.0), (3, 3.0), (5, 7.0)]
    assert set(got[0]) == {"id", "values", "metadata", "score"} and got[0]["metadata"]["note"] == "x"
    got = qp.find_similar_bits(code(0, 1, 2), 10, by="sig", metric="jaccard")
    assert [(h["metadata"]["year"], h["score"]) for h in got] == [(1, 0.0), (2, 1 / 3), (3, 1.0), (5, 1.0)]
    many = qp.find_similar_bits_many([code(0, 1), code()], 2, by="sig", metric="jaccard", where={"year": {"$lt": 5}})
    assert [[(h["metadata"]["year"], h["score"]) for h in hits] for hits in many] == [[(2, 0.0), (1, 1 / 3)], [(3, 0.0), (1, 1.0)]]
    with pytest.raises(ValueError, match="one dict filter"):
        qp.find_similar_bits(code(), 3, by="sig", where=lambda m: True)
    ids = qp.query_by_metadata({})
    qp.update_metadata([ids[3]], {"sig": code(0, 1, 2).tolist()})
    assert [h["metadata"]["year"] for h in qp.find_similar_bits(code(0, 1, 2), 2, by="sig")] == [1, 4]


# ---------------------------------------------------------------- snapshots
def _sha(path):
    return {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(Path(path).iterdir()) if p.is_file()}


def test_v6_snapshot_round_trip(tmp_path):
    rng, index, vectors, metas, base = _filled(seed=12, n=90)
    index.remove([v.id for v in vectors[::7]], "ns")
    index.update_attributes([vectors[1].id, vectors[2].id], [{"sig": forms(base[3])[0]}, {"sig": None}], "ns")  # leaves garbage
    metas[1]["sig"], metas[2]["sig"] = forms(base[3])[0], None
    index.save_index(str(tmp_path))
    manifest = json.loads((tmp_path / "index.json").read_text())
    assert manifest["format"] == "mlvdb-index-v6" and manifest["attributes"] == SCHEMA
    names = {p.name for p in tmp_path.iterdir()}
    assert {"ns0.attr0.i64", "ns0.attr0.bits.u64", "ns0.attr1.i64", "ns0.attr2.values.i64"} <= names
    held = [i for i, m in enumerate(metas) if i % 7 and m.get("sig") is not None]
    has = np.fromfile(tmp_path / "ns0.attr0.i64", dtype=np.int64)
    assert has.tolist() == [1 if i in set(held) else W.INT64_ABSENT for i in range(len(metas))]
    dense = np.fromfile(tmp_path / "ns0.attr0.bits.u64", dtype="<u8")  # the live present rows' codes, dense, in row order
    assert dense.tolist() == [int(w) for i in held for w in W.encode_bits_code(metas[i]["sig"], 128, "x")]
    loaded = _index(schema={})
    assert loaded.load_index(str(tmp_path)) and loaded.attributes == SCHEMA
    queries = [forms(q)[0] for q in (base[0], base[3], near(rng, base[4], 5))]
    for metric in ("hamming", "jaccard"):
        for where in (None, {"year": {"$lt": 2004}}, {"sig": {"$exists": True}, "tags": "a"}):
            a = index.search_bits(queries, 20, "ns", "sig", metric=metric, where=where)
            b = loaded.search_bits(queries, 20, "ns", "sig", metric=metric, where=where)
            assert a == b and a.scores.tobytes() == b.scores.tobytes() and a.counts.sum() > 0
    loaded.save_index(str(tmp_path / "again"))
    assert _sha(tmp_path / "again") == _sha(tmp_path)
    assert loaded.compact("ns")
    a = index.search_bits(queries, 20, "ns", "sig")
    b = loaded.search_bits(queries, 20, "ns", "sig")
    assert a == b and a.scores.tobytes() == b.scores.tobytes()
    with open(tmp_path / "ns0.attr0.bits.u64", "ab") as f:
        f.write(b"\x00" * 8)
    with pytest.raises(RuntimeError, match="bits attribute files"):
        _index(schema={}).load_index(str(tmp_path))
    (tmp_path / "ns0.attr0.bits.u64").unlink()
    with pytest.raises(RuntimeError, match="bits attribute files"):
        _index(schema={}).load_index(str(tmp_path))


def test_a_bits_attribute_in_an_older_format_is_refused(tmp_path):
    rng, index, vectors, metas, base = _filled(seed=3, n=20)
    index.save_index(str(tmp_path))
    manifest = json.loads((tmp_path / "index.json").read_text())
    manifest["format"] = "mlvdb-index-v5"
    (tmp_path / "index.json").write_text(json.dumps(manifest))
    with pytest.raises(RuntimeError, match="only mlvdb-index-v6 holds them"):
        _index(schema={}).load_index(str(tmp_path))


# sha256 of every file ``bits_helpers.legacy_index`` saved with the code from before bits attributes existed
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
    "v4": {
        "index.json": "ce56a8a3c1b11097a4b539421819686f9dd6aa8b3038e31becc4e3141ec93ba2",
        "ns0.attr0.i64": "40c83f29accd1970c2cd725c1d85cda11d00da771372f76d6823f0c2714bb2f8",
        "ns0.attr1.i64": "b2567f8b25a1c2fed921a731502095352f6e8fd0b42969a6ee63363058547bd4",
        "ns0.attr1.offsets.i64": "77c30ece54adab205cb8cfb9a474b52eee8ece4210265e16a0fee0fbc279448a",
        "ns0.attr1.terms.i32": "e547461bcbd4c474d3c8b2a433d4a3f7d5667b5d7e27a40f3031f79ae3c7b475",
        "ns0.attr1.weights.f32": "9f278cd0bdd1fc1b48b9f9ede698defb3d3f44c0f86459e71839f7cb4770ed18",
        "ns0.attr2.i64": "c7717289c44df33154ee6284c7e3fcd41ed17aedd2b6cf9cd0ecf5f449fa7de7",
        "ns0.attr2.offsets.i64": "f42ab8ddcda4bdf10e5dd661bb32754af6d664f4e5f203faa57aa6a49dcd171f",
        "ns0.attr2.values.i64": "de072efd979f52c91c3817861f059fe3f0fc5713205ad6e5df096e10c000bcd9",
        "ns0.deleted.i64": "669a981310064377d9256ecc7ed21360ecfff3d57f18ac27014f3e52fc7e4098",
        "ns0.ids.u8": "4ade590d2e9965bab16020792f119d8f7ef03524d0ae0c346468e80527b92b09",
        "ns0.rows.f32": "6e7e4d1ba09938fe0bef6b719dfb4ab6197c3ab876d871175da22ae268544635",
    },
    "v5": {
        "index.json": "d680b471bd21135d8274d0e7cfcd28b05ffe451a3cef1d04e7b44ad8016b447c",
        "ns0.attr0.i64": "40c83f29accd1970c2cd725c1d85cda11d00da771372f76d6823f0c2714bb2f8",
        "ns0.attr1.i64": "8aa44e3a212728b98f9419e9096023342aeea1e403dc4fa815e89d8fa295ff35",
        "ns0.attr2.f64": "0a31eb6dab416326699a98379099ceda7547f3da4265b6dd7693377a405accc5",
        "ns0.deleted.i64": "669a981310064377d9256ecc7ed21360ecfff3d57f18ac27014f3e52fc7e4098",
        "ns0.ids.u8": "4ade590d2e9965bab16020792f119d8f7ef03524d0ae0c346468e80527b92b09",
        "ns0.rows.f32": "6e7e4d1ba09938fe0bef6b719dfb4ab6197c3ab876d871175da22ae268544635",
    },
}


@pytest.mark.parametrize("version", ["v1", "v2", "v3", "v4", "v5"])
def test_snapshots_without_bits_attributes_are_byte_identical_to_before(tmp_path, version):
    legacy_index(version).save_index(str(tmp_path))
    assert json.loads((tmp_path / "index.json").read_text())["format"] == f"mlvdb-index-{version}"
    assert _sha(tmp_path) == LEGACY[version]
    engine = geo_helpers.oracle_engine_class() if version == "v5" else BitsOracleEngine
    loaded = Index(space="cosine", engine_factory=lambda dim, sp: engine(dim, sp))
    assert loaded.load_index(str(tmp_path))
    loaded.save_index(str(tmp_path / "again"))
    assert _sha(tmp_path / "again") == LEGACY[version]


# ---------------------------------------------------------------- the C ABI without a device
def test_bits_entries_are_declared_bound_and_refuse_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_bits.h").read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(_native.BITS_SIGNATURES) and len(names) == 4
    assert names == ["mlvdb_bits_get", "mlvdb_bits_set", "mlvdb_bits_set_at", "mlvdb_search_batch_bits"]
    others = [t for n, t in vars(_native).items() if n.endswith("SIGNATURES") and n != "BITS_SIGNATURES"]
    assert not any(set(names) & set(t) for t in others)
    for name in names:  # the parameter count of each prototype is the binding's
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert len(params) == len(_native.BITS_SIGNATURES[name][1]), name
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert int(consts["MLVDB_ATTR_BITS"]) == _native.ATTR_BITS == _native.LIST_ATTR_CODES["bits"] == 6
    assert int(consts["MLVDB_BITS_MAX_WORDS"]) == _native.BITS_MAX_WORDS == 255
    assert int(consts["MLVDB_BITS_HAMMING"]) == _native.BITS_HAMMING == _native.BITS_METRIC_CODES["hamming"] == 0
    assert int(consts["MLVDB_BITS_JACCARD"]) == _native.BITS_JACCARD == _native.BITS_METRIC_CODES["jaccard"] == 1
    lib = _native.load()
    assert lib.mlvdb_abi_version() == 7 == _native.ABI_VERSION
    null, z, buf = C.c_void_p(), C.c_int64(0), (C.c_int64 * 4)()
    calls = {
        "mlvdb_bits_set": (null, 0, 0, 1, 1, buf, None),
        "mlvdb_bits_set_at": (null, 0, buf, 1, 1, buf, None, C.byref(z)),
        "mlvdb_bits_get": (null, 0, 0, 1, buf, buf, 4, C.byref(z)),
        "mlvdb_search_batch_bits": (null, 0, buf, 1, 1, 0, 1, None, buf, buf, buf, None),
    }
    assert sorted(calls) == names
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == 1, name  # MLVDB_ERR_INVALID_ARG
        assert b"null index handle" in lib.mlvdb_last_global_error(), name


def test_every_new_entry_is_guarded():
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    for name in _native.BITS_SIGNATURES:
        body = re.search(r"^int " + name + r"\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
        assert body.lstrip().startswith("return guarded("), name


def test_the_new_unit_and_header_are_in_the_build():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "kernels_bits.hip" in srcs and "../../include/mlvdb_bits.h" in make


# ---------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_bits_kernels_use_no_scratch(tmp_path):
    """DESIGN 11.17 records the VGPR, SGPR and LDS figures this report gives."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "mlvectordb_amd" / "csrc"
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(csrc / "kernels_bits.hip"), "-o",
                          str(tmp_path / "k.o")], capture_output=True, text=True, cwd=csrc, check=True).stderr
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    hits = [v for k, v in seen.items() if "bits_scan_kernel" in k]
    assert len(hits) == 6 and all(v == 0 for v in hits), seen  # five group sizes with the queries in registers, one through LDS
