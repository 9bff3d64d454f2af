"""Search by stored examples (include/mlvdb_like.h) without a GPU: the NumPy query rule against the definition in Python
floats, the default weights, the refusals of ``Index.search_like`` / ``QueryProcessor.find_similar_to`` before the engine is
touched, the surface over an oracle engine, and the C ABI's shape."""
import ctypes as C
import re
import uuid
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from tests.like_helpers import LikeOracleEngine, example_sets, like_queries, like_strip, most_examples, oracle_index
from tests.where_helpers import WhereOracleEngine

ROOT = Path(__file__).resolve().parents[1]
SCHEMA = {"doc": "int", "flag": "bool"}


# ---------------------------------------------------------------- the helper against the definition
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_the_numpy_rule_equals_the_definition_in_python_floats(space):
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((9, 5)).astype(np.float32)
    labels = np.array([0, 8, 3, 3, 5, 2], np.int64)
    weights = np.array([0.5, -0.25, 1.0, 1.0, 1 / 3, -1.0])
    offsets = np.array([0, 2, 2, 5, 6], np.int64)
    base = rng.standard_normal((4, 5)).astype(np.float32)
    for b in (None, base):
        got, scale = like_queries(rows, labels, weights, offsets, space, b)
        for i in range(4):
            for c in range(5):
                acc = 0.0 if b is None else float(b[i, c])
                mag = 0.0
                for j in range(offsets[i], offsets[i + 1]):
                    x = [float(v) for v in rows[labels[j]]]
                    t = float(weights[j])
                    if space == "cosine":
                        t = t * (1.0 / (float(np.sqrt(np.sum(np.array(x) * np.array(x)))) + 1e-30))
                    acc = acc + t * x[c]
                    mag += abs(t * x[c])
                assert got[i, c] == np.float32(acc) and scale[i, c] == mag
    assert np.array_equal(like_queries(rows, labels, weights, offsets, space, base)[0][1], base[1])  # no example: the base row
    # the same row once for and once against: exactly zero, in every space
    zero, _ = like_queries(rows, [4, 4], [1.0, -1.0], [0, 2], space)
    assert not zero.any()


def test_the_host_strip_keeps_the_order_and_pads():
    lab = np.array([[5, 2, 9, 7, -1], [1, 2, 3, 4, 6]], np.int64)
    d64 = np.array([[0.1, 0.2, 0.3, 0.4, np.inf], [1, 2, 3, 4, 5]], np.float64)
    cnt = np.array([4, 5], np.int32)
    out = like_strip(lab, d64.astype(np.float32), cnt, d64, [{2, 7, 11}, set()], 3)
    assert out[0].tolist() == [[5, 9, -1], [1, 2, 3]] and out[2].tolist() == [2, 3]
    assert out[3][0].tolist() == [0.1, 0.3, np.inf] and out[1].dtype == np.float32
    assert example_sets([3, 3, 4, 9], [0, 3, 3, 4]) == [{3, 4}, set(), {9}] and most_examples([3, 3, 4, 9], [0, 3, 3, 4]) == 2


def test_the_default_weights_are_the_average_vector_rule_in_python_floats():
    assert Index.like_weights(1, 0) == (1.0, 0.0)
    assert Index.like_weights(3, 0) == (1.0 / 3, 0.0)
    assert Index.like_weights(3, 2) == (2.0 / 3, -0.5)
    assert Index.like_weights(7, 1) == (2.0 / 7, -1.0)
    assert Index.like_weights(0, 4) == (0.0, -0.25)


# ---------------------------------------------------------------- refusals, before the engine is touched
class UntouchableEngine(WhereOracleEngine):
    """Fails the test if a search of any kind reaches the engine."""

    def search(self, *a, **kw):
        raise AssertionError("the engine was touched")

    search64 = search_like = search


def _filled(factory=LikeOracleEngine, n=300, d=8, seed=1, space="l2", **kw):
    rng = np.random.default_rng(seed)
    index = Index(space=space, engine_factory=factory, attributes=SCHEMA, **kw)
    metas = [{"doc": int(rng.integers(0, 40)), "flag": bool(i % 2)} for i in range(n)]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs, "ns")
    return rng, index, vecs, rows, metas


def test_like_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, vecs, _, _ = _filled(UntouchableEngine)
    ids = [v.id for v in vecs]
    stranger = uuid.uuid4()
    with pytest.raises(ValueError, match=f"{stranger} is unknown or removed"):
        index.search_like([ids[:2], [ids[3], stranger]], 5, "ns", "l2")
    index.remove([ids[7]], "ns")
    with pytest.raises(ValueError, match=f"{ids[7]} is unknown or removed"):
        index.search_like([ids[7]], 5, "ns", "l2")
    with pytest.raises(ValueError, match=f"{ids[7]} is unknown or removed"):
        index.search_like([ids[1]], 5, "ns", "l2", negative=[ids[7]])
    with pytest.raises(ValueError, match="names 65 examples, at most 64"):
        index.search_like([ids[10:75]], 5, "ns", "l2")
    with pytest.raises(ValueError, match="names 65 examples, at most 64"):
        index.search_like([ids[10:50]], 5, "ns", "l2", negative=[ids[50:75]])
    with pytest.raises(ValueError, match=r"top_k \+ examples must be <= 1024 \(got 1021 \+ 4\)"):
        index.search_like([ids[10:12], ids[20:24]], 1021, "ns", "l2")
    with pytest.raises(ValueError, match="per-query where list"):
        index.search_like([ids[:1], ids[1:2]], 5, "ns", "l2", where=[None, {"doc": 1}])
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.search_like([ids[:1]], 5, "ns", "l2", where={"nope": 1})
    with pytest.raises(ValueError, match="cannot be combined with negative"):
        index.search_like([ids[:2]], 5, "ns", "l2", negative=[ids[2:3]], weights=[[1.0, 2.0]])
    with pytest.raises(ValueError, match="one number per positive id"):
        index.search_like([ids[:2]], 5, "ns", "l2", weights=[[1.0]])
    with pytest.raises(ValueError, match="weights must be finite"):
        index.search_like([ids[:2]], 5, "ns", "l2", weights=[[1.0, float("nan")]])
    with pytest.raises(ValueError, match="2 positive entries, 1 negative entries"):
        index.search_like([ids[:1], ids[1:2]], 5, "ns", "l2", negative=[ids[2:3]])
    with pytest.raises(ValueError, match="query 1 has no example"):
        index.search_like([ids[:1], []], 5, "ns", "l2")
    with pytest.raises(ValueError, match="2 positive entries, 3 queries"):
        index.search_like([ids[:1], []], 5, "ns", "l2", queries=np.zeros((3, 8), np.float32))
    # nothing to search: empty answers, the engine still untouched
    assert [len(h) for h in index.search_like([ids[:1], ids[1:3]], 5, "other", "l2")] == [0, 0]
    assert [len(h) for h in index.search_like([ids[:1], ids[1:3]], 0, "ns", "l2")] == [0, 0]
    assert [len(h) for h in index.search_like([ids[:1]], 5, "ns", "l2", queries=np.zeros((1, 9), np.float32))] == [0]
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="where must be one dict filter"):
        qp.find_similar_to(ids[:2], 5, "ns", where=lambda m: True)
    with pytest.raises(ValueError, match=f"{stranger} is unknown or removed"):
        qp.find_similar_to([stranger], 5, "ns")


def test_like_on_a_row_sharded_index_or_an_engine_without_it_is_refused():
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    with pytest.raises(ValueError, match="row-sharded"):
        sharded.search_like([uuid.uuid4()], 3, "ns", "l2")
    _, index, vecs, _, _ = _filled(WhereOracleEngine)
    with pytest.raises(ValueError, match="needs an engine with search_like"):
        index.search_like([vecs[0].id], 3, "ns", "l2")


# ---------------------------------------------------------------- Index / QueryProcessor over the oracle engine
class RecordingEngine(LikeOracleEngine):
    calls = []

    def search_like(self, labels, weights, offsets, k, **kw):
        RecordingEngine.calls.append((np.asarray(labels).tolist(), np.asarray(weights).tolist(), np.asarray(offsets).tolist(),
                                      k, kw["exclude"], kw["base"] is not None, kw["where"] is not None))
        return super().search_like(labels, weights, offsets, k, **kw)


def test_index_hands_the_engine_labels_default_weights_and_a_clamped_top_k():
    RecordingEngine.calls = []
    _, index, vecs, _, _ = _filled(RecordingEngine, n=30)
    ids = [v.id for v in vecs]
    index.search_like(ids[4:7], 5, "ns", "l2")                                         # a flat sequence: one query
    index.search_like([ids[4:7], [ids[9]]], 5, "ns", "l2", negative=[ids[1:3], []])
    index.search_like([[ids[2], ids[2]]], 100, "ns", "l2", weights=[[0.25, 3]], exclude_examples=False,
                      queries=np.ones((1, 8)), where={"flag": True})
    third = 1.0 / 3
    assert RecordingEngine.calls == [
        ([4, 5, 6], [third] * 3, [0, 3], 5, True, False, False),
        ([4, 5, 6, 1, 2, 9], [2.0 / 3] * 3 + [-0.5] * 2 + [1.0], [0, 5, 6], 5, True, False, False),
        ([2, 2], [0.25, 3.0], [0, 2], 30, False, True, True)]                           # top_k clamps to the live count


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_index_search_like_equals_search_many_of_the_helpers_query_without_the_examples(space):
    rng, index, vecs, rows, metas = _filled(space=space)
    ids = [v.id for v in vecs]
    pos = [[3], [10, 11, 12], [40, 41], [7, 7, 8]]
    neg = [[], [20], [50, 51, 52], [9]]
    labels, weights, offsets = [], [], [0]
    for p, n in zip(pos, neg):
        wp, wn = Index.like_weights(len(p), len(n))
        labels += p + n
        weights += [wp] * len(p) + [wn] * len(n)
        offsets.append(len(labels))
    base = rng.standard_normal((4, 8)).astype(np.float32)
    for b in (None, base):
        for where, allowed in ((None, np.ones(len(metas), bool)), ({"flag": True}, np.array([m["flag"] for m in metas]))):
            qs, _ = like_queries(rows, labels, weights, offsets, space, b)
            got = index.search_like([[ids[j] for j in p] for p in pos], 6, "ns", space,
                                    negative=[[ids[j] for j in n] for n in neg], queries=b, where=where)
            plain = index.search_many(qs, 6 + 5, "ns", space, where=where)
            for i, hits in enumerate(got):
                named = {ids[j] for j in pos[i] + neg[i]}
                want = [h for h in plain[i] if h.vector_id not in named][:6]
                assert [(h.vector_id, h.score) for h in hits] == [(h.vector_id, h.score) for h in want] and len(hits) == 6
            kept = index.search_like([[ids[j] for j in p] for p in pos], 6, "ns", space,
                                     negative=[[ids[j] for j in n] for n in neg], queries=b, where=where, exclude_examples=False)
            assert kept == index.search_many(qs, 6, "ns", space, where=where)
    one = index.search_like([ids[3]], 4, "ns", space)  # a stored vector's neighbours: itself left out
    assert len(one) == 1 and ids[3] not in [h.vector_id for h in one[0]]
    if space != "ip":  # (the largest inner product need not be a row's own)
        assert index.search_like([ids[3]], 4, "ns", space, exclude_examples=False)[0][0].vector_id == ids[3]


def test_query_processor_find_similar_to_returns_enriched_hits_without_the_examples():
    rng = np.random.default_rng(4)
    qp = QueryProcessor(InMemoryStorage(), oracle_index({"doc": "int"}, space="cosine"))
    dtos = [VectorDTO(values=rng.standard_normal(6).tolist(), metadata={"doc": int(i % 9), "i": i}) for i in range(120)]
    qp.upsert_many(dtos, "ns")
    stored = sorted(qp.get_namespace_vectors("ns"), key=lambda v: v["metadata"]["i"])
    ids = [v["id"] for v in stored]
    rows = np.array([d.values for d in dtos], np.float32)
    hits = qp.find_similar_to(ids[:3], 5, "ns", negative_ids=ids[3:5])
    qs, _ = like_queries(rows, [0, 1, 2, 3, 4], [2 / 3] * 3 + [-0.5] * 2, [0, 5], "cosine")
    near = [h for h in qp.find_similar_many(qs, 10, "ns")[0] if h["id"] not in ids[:5]][:5]
    assert [(h["id"], h["score"], h["metadata"]) for h in hits] == [(h["id"], h["score"], h["metadata"]) for h in near]
    assert len(hits) == 5 and all(np.array_equal(h["values"], rows[h["metadata"]["i"]]) for h in hits)
    only = qp.find_similar_to(ids[:3], 5, "ns", where={"doc": 3}, query=VectorDTO(values=rows[50].tolist()))
    assert len(only) == 5 and all(h["metadata"]["doc"] == 3 for h in only)
    many = qp.find_similar_to_many([ids[:3], ids[7:8]], 5, "ns", negative_ids=[ids[3:5], []])
    assert [h["id"] for h in many[0]] == [h["id"] for h in hits] and ids[7] not in [h["id"] for h in many[1]]
    qp.delete([ids[1]], "ns")
    with pytest.raises(ValueError, match=f"{ids[1]} is unknown or removed"):
        qp.find_similar_to(ids[:3], 5, "ns")


# ---------------------------------------------------------------- C ABI
def _header_text():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_like.h").read_text(), flags=re.S)


def test_like_header_declares_what_the_binding_binds():
    lib = _native.load()
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", _header_text())))
    assert names == ["mlvdb_search_batch_like"] == sorted(_native.LIKE_SIGNATURES)
    assert hasattr(lib, names[0])
    params = re.search(r"mlvdb_search_batch_like\((.*?)\);", _header_text(), flags=re.S).group(1).split(",")
    restype, argtypes = _native.LIKE_SIGNATURES[names[0]]
    assert len(params) == len(argtypes) == 14 and restype is C.c_int
    assert argtypes[5:8] == [C.c_int64, C.c_int32, C.c_int32] and "exclude_examples" in params[7]
    assert int(re.search(r"#define MLVDB_LIKE_MAX_FETCH (\d+)", _header_text()).group(1)) == _native.LIKE_MAX_FETCH == 1024
    assert int(re.search(r"#define MLVDB_LIKE_MAX_EXAMPLES (\d+)", _header_text()).group(1)) == _native.LIKE_MAX_EXAMPLES == 64
    assert Index._MAX_LIKE_FETCH == 1024 and Index._MAX_LIKE_EXAMPLES == 64
    assert lib.mlvdb_abi_version() == 7


def test_like_entry_refuses_a_null_handle_inside_the_exception_guard():
    lib = _native.load()
    buf = (C.c_double * 4)()
    assert lib.mlvdb_search_batch_like(C.c_void_p(), buf, buf, buf, None, 1, 1, 1, None, buf, buf, buf, None, None) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()


def test_the_like_kernels_and_header_are_in_the_build():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_like\.hip\b", make, flags=re.M)
    assert "mlvdb_like.h" in make and "-ffp-contract=off" in make
    kern = (ROOT / "mlvectordb_amd" / "csrc" / "kernels_like.hip").read_text()
    assert "#pragma clang fp contract(off)" in kern and "query_aux_from_sums" in kern and "query_norm_wave_sum" in kern
    assert "atomic" not in kern.split("#include", 1)[1]
