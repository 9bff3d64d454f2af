"""Similarity join (include/mlvdb_join.h) without a GPU: the strip rule against a brute-force double loop, the union-find
groups against a hand-made graph, every refusal of ``Index.join_within`` / ``duplicate_groups`` and the ``QueryProcessor``
entries before the engine is touched, the surface over an oracle engine, and the C ABI's shape."""
import ctypes as C
import re
import uuid
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from mlvectordb_amd.engine import JoinOverflow
from mlvectordb_amd.join import PairHits, connected_groups, gather_segments
from oracle import exact_scan
from tests.join_helpers import LATER, OTHERS, JoinOracleEngine, join_model, oracle_index, strip
from tests.where_helpers import WhereOracleEngine

ROOT = Path(__file__).resolve().parents[1]
SCHEMA = {"doc": "int", "flag": "bool"}


# ---------------------------------------------------------------- the rule and the groups
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_the_numpy_model_equals_a_brute_force_double_loop(space):
    rng = np.random.default_rng(11)
    rows = rng.integers(-2, 3, (60, 6)).astype(np.float32)  # small integers: plenty of exact ties and identical rows
    rows[rows.any(axis=1) == 0] = 1.0                        # (no zero row: cosine of a zero row is a rule of its own)
    deleted = np.zeros(60, bool)
    deleted[[3, 17, 40]] = True
    matching = rng.random(60) < 0.7
    dm = exact_scan.exact_distances(rows, rows, space)
    radius = float(np.float32(np.quantile(dm, 0.15)))
    left = np.array([0, 3, 4, 17, 18, 30, 59])              # tombstoned left rows are valid queries
    for mode in (OTHERS, LATER):
        for match in (None, matching):
            got, counts = join_model(rows, left, radius, space, mode, deleted=deleted, matching=match)
            for (gl, gd), a, c in zip(got, left, counts):
                want = []
                for b in range(60):
                    visible = not deleted[b] and (match is None or match[b])
                    excluded = b <= a if mode == LATER else b == a
                    if visible and not excluded and dm[a, b] <= radius:
                        want.append((dm[a, b], b))
                want.sort()
                assert gl.tolist() == [b for _, b in want] and c == len(want)
                assert gd.tolist() == [float(np.float32(d)) for d, _ in want]
    lab, d = np.array([4, 9, 2, 7], np.int64), np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    assert strip(lab, d, 4, _native.JOIN_OTHERS)[0].tolist() == [9, 2, 7]
    assert strip(lab, d, 4, _native.JOIN_LATER)[0].tolist() == [9, 7]
    assert strip(lab, d, 4, _native.JOIN_LATER)[1].tolist() == [np.float32(0.2), np.float32(0.4)]


def test_union_find_groups_of_a_hand_made_graph():
    #   1 - 5 - 9      2 - 3      7 alone (no edge)      20 - 4, 4 - 11, 11 - 20 (a cycle)      6 - 6 (a loop)
    left = [5, 1, 2, 20, 4, 11, 6, 9]
    right = [9, 5, 3, 4, 11, 20, 6, 1]
    assert connected_groups(left, right) == [[1, 5, 9], [2, 3], [4, 11, 20]]
    assert connected_groups([], []) == []
    chain = list(range(0, 2000))
    assert connected_groups(chain[:-1], chain[1:]) == [chain]
    assert connected_groups(chain[1:][::-1], chain[:-1][::-1]) == [chain]


def test_gather_segments_lists_the_segments_in_the_order_asked():
    offsets = np.array([0, 2, 2, 5, 6], np.int64)
    assert gather_segments(offsets, np.array([2, 0, 3, 1])).tolist() == [2, 3, 4, 0, 1, 5]
    assert gather_segments(offsets, np.array([1])).tolist() == []
    assert gather_segments(np.array([0], np.int64), np.zeros(0, np.int64)).tolist() == []


# ---------------------------------------------------------------- refusals, before the engine is touched
class UntouchableEngine(WhereOracleEngine):
    """Fails the test if a join or anything it would lean on reaches the engine."""

    def join_within(self, *a, **kw):
        raise AssertionError("the engine was touched")

    range = search = search64 = where_labels = get_rows_at = join_within


def _filled(factory=JoinOracleEngine, n=120, d=8, seed=1, space="l2", **kw):
    rng = np.random.default_rng(seed)
    index = Index(space=space, engine_factory=factory, attributes=SCHEMA, **kw)
    metas = [{"doc": int(rng.integers(0, 4)), "flag": bool(i % 2), "i": i} for i in range(n)]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    for a, b in ((3, 50), (3, 77), (10, 11), (20, 119), (41, 60)):  # identical rows: {3, 50, 77}, {10, 11}, {20, 119}, {41, 60}
        rows[b] = rows[a]
    rows[90] = rows[10] * np.float32(1.001)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs, "ns")
    return rng, index, vecs, rows, metas


def test_join_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, vecs, _, _ = _filled(UntouchableEngine)
    ids = [v.id for v in vecs]
    stranger = uuid.uuid4()
    for entry in (index.join_within, index.duplicate_groups):
        with pytest.raises(ValueError, match="metric must be one of"):
            entry("ns", "manhattan", 0.5)
        with pytest.raises(ValueError, match="radius must be >= 0"):
            entry("ns", "l2", -0.5)
        with pytest.raises(ValueError, match="radius must be >= 0"):
            entry("ns", "cosine", -1e-9)
        with pytest.raises(ValueError, match="radius must be a number"):
            entry("ns", "l2", float("nan"))
        with pytest.raises(ValueError, match="radius must be a number"):
            entry("ns", "l2", "near")
        for bad in (0, -1, _native.JOIN_MAX_CAPACITY + 1, 2.5, True):
            with pytest.raises(ValueError, match="max_per_row must be an int in"):
                entry("ns", "l2", 0.5, max_per_row=bad)
        with pytest.raises(ValueError, match="predicate has no device form"):
            entry("ns", "l2", 0.5, where=lambda m: True)
        with pytest.raises(ValueError, match="where must be one dict filter or None"):
            entry("ns", "l2", 0.5, where=[{"doc": 1}])
        with pytest.raises(ValueError, match="not a declared attribute"):
            entry("ns", "l2", 0.5, where={"nope": 1})
    with pytest.raises(ValueError, match="order must be one of"):
        index.join_within("ns", "l2", 0.5, order="score")
    with pytest.raises(ValueError, match="ids must not repeat"):
        index.join_within("ns", "l2", 0.5, ids=[ids[1], ids[2], ids[1]])
    with pytest.raises(ValueError, match=f"{stranger} is unknown or removed"):
        index.join_within("ns", "l2", 0.5, ids=[ids[1], stranger])
    with pytest.raises(ValueError, match=f"{stranger} is unknown or removed"):
        index.join_within("other", "l2", 0.5, ids=[stranger])
    index.remove([ids[7]], "ns")
    with pytest.raises(ValueError, match=f"{ids[7]} is unknown or removed"):
        index.join_within("ns", "l2", 0.5, ids=[ids[7]])
    # nothing to join: empty answers, the engine still untouched
    assert len(index.join_within("other", "l2", 0.5)) == 0 and index.join_within("other", "l2", 0.5).complete
    assert index.duplicate_groups("other", "l2", 0.5) == []
    qp = QueryProcessor(InMemoryStorage(), index)
    for entry in (qp.find_near_pairs, qp.find_duplicates):
        with pytest.raises(ValueError, match="where must be a dict filter, a predicate or None"):
            entry(0.5, "ns", "l2", where=[{"doc": 1}])
        with pytest.raises(ValueError, match="metric must be one of"):
            entry(0.5, "ns", "manhattan")
        with pytest.raises(ValueError, match="radius must be >= 0"):
            entry(-1.0, "ns", "l2")
        with pytest.raises(ValueError, match="max_per_row must be an int in"):
            entry(0.5, "ns", "l2", max_per_row=0)


def test_join_on_a_row_sharded_index_or_an_engine_without_it_is_refused():
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    with pytest.raises(ValueError, match="row-sharded"):
        sharded.join_within("ns", "l2", 0.5)
    with pytest.raises(ValueError, match="row-sharded"):
        sharded.duplicate_groups("ns", "l2", 0.5)
    _, index, _, _, _ = _filled(WhereOracleEngine)
    with pytest.raises(ValueError, match="needs an engine with join_within"):
        index.join_within("ns", "l2", 0.5)


def test_a_negative_radius_is_a_radius_on_an_ip_namespace():
    _, index, vecs, rows, _ = _filled(space="ip")
    pairs = index.join_within("ns", "ip", -3.0)
    dm = exact_scan.exact_distances(rows, rows, "ip")
    want = {(a, b) for a in range(len(rows)) for b in range(a + 1, len(rows)) if dm[a, b] <= -3.0}
    assert want and set(zip(pairs.left_labels.tolist(), pairs.right_labels.tolist())) == want


# ---------------------------------------------------------------- Index / QueryProcessor over the oracle engine
@pytest.mark.parametrize("space,metric,radius", [("l2", "l2", 1e-3), ("l2", "euclidean", 0.03), ("cosine", "cosine", 1e-5)])
def test_index_self_join_lists_every_pair_once_with_the_earlier_row_on_the_left(space, metric, radius):
    _, index, vecs, rows, metas = _filled(space=space)
    ids = [v.id for v in vecs]
    pairs = index.join_within("ns", metric, radius)
    assert isinstance(pairs, PairHits) and pairs.complete
    got = list(zip(pairs.left_labels.tolist(), pairs.right_labels.tolist()))
    want = [(3, 50), (3, 77), (10, 11), (10, 90), (11, 90), (20, 119), (41, 60), (50, 77)]
    assert sorted(got) == want and all(a < b for a, b in got)
    assert got == sorted(got, key=lambda p: p[0]) and pairs.left_ids.tolist() == [ids[a] for a, _ in got]
    assert pairs.right_ids.tolist() == [ids[b] for _, b in got]
    native = radius ** 2 if metric == "euclidean" else radius
    ref = index.range_search_many(rows, radius, "ns", metric)
    assert pairs.counts.tolist() == [sum(1 for h in ref[a] if ids.index(h.vector_id) > a) for a in range(len(rows))]
    for a, b, s in zip(pairs.left_ids, pairs.right_ids, pairs.scores):  # the scores are range_search_many's own
        assert s == next(h.score for h in ref[ids.index(a)] if h.vector_id == b)
    assert (pairs.distances <= np.float32(native)).all()
    # order="distance": nearest pair first, ties by left then right
    by_distance = index.join_within("ns", metric, radius, order="distance")
    keys = list(zip(by_distance.distances.tolist(), by_distance.left_labels.tolist(), by_distance.right_labels.tolist()))
    assert keys == sorted(keys) and sorted(k[1:] for k in keys) == want
    # a dict where: both sides match it
    flagged = index.join_within("ns", metric, radius, where={"flag": True})
    want_flag = [(a, b) for a, b in want if metas[a]["flag"] and metas[b]["flag"]]
    assert sorted(zip(flagged.left_labels.tolist(), flagged.right_labels.tolist())) == want_flag
    assert flagged.counts.size == sum(m["flag"] for m in metas)


def test_index_join_by_ids_answers_in_the_callers_order_without_the_row_itself():
    _, index, vecs, rows, metas = _filled()
    ids = [v.id for v in vecs]
    asked = [77, 5, 10, 3]
    pairs = index.join_within("ns", "l2", 1e-3, ids=[ids[j] for j in asked])
    assert pairs.left_row_ids.tolist() == [ids[j] for j in asked] and pairs.counts.tolist() == [2, 0, 2, 2]
    assert list(zip(pairs.left_labels.tolist(), pairs.right_labels.tolist())) == [(77, 3), (77, 50), (10, 11), (10, 90),
                                                                                 (3, 50), (3, 77)]
    # the partners must match `where`, the ids themselves need not
    odd = index.join_within("ns", "l2", 1e-3, ids=[ids[50], ids[10]], where={"flag": True})
    assert list(zip(odd.left_labels.tolist(), odd.right_labels.tolist())) == [(50, 3), (50, 77), (10, 11)]
    # max_per_row cuts the nearest, the counts stay exact
    cut = index.join_within("ns", "l2", 1e-3, ids=[ids[3], ids[5]], max_per_row=1)
    assert not cut.complete and cut.counts.tolist() == [2, 0] and cut.right_labels.tolist() == [50]
    assert len(index.join_within("ns", "l2", 1e-3, ids=[])) == 0


def test_duplicate_groups_are_the_components_in_insertion_order_and_raise_when_truncated():
    _, index, vecs, rows, metas = _filled()
    ids = [v.id for v in vecs]
    groups = index.duplicate_groups("ns", "l2", 1e-3)
    assert groups == [[ids[3], ids[50], ids[77]], [ids[10], ids[11], ids[90]], [ids[20], ids[119]], [ids[41], ids[60]]]
    assert index.duplicate_groups("ns", "l2", 0.0) == [[ids[3], ids[50], ids[77]], [ids[10], ids[11]], [ids[20], ids[119]],
                                                       [ids[41], ids[60]]]
    assert index.duplicate_groups("ns", "l2", 1e-3, where={"flag": True}) == [[ids[3], ids[77]]]
    with pytest.raises(JoinOverflow) as e:
        index.duplicate_groups("ns", "l2", 1e-3, max_per_row=1)
    assert e.value.max_per_row == 1 and e.value.most == 2
    index.remove([ids[50]], "ns")  # a removed row is nobody's partner
    assert index.duplicate_groups("ns", "l2", 1e-3)[0] == [ids[3], ids[77]]


def test_query_processor_entries_enrich_and_take_a_predicate_on_the_host_path():
    rng = np.random.default_rng(4)
    index = oracle_index({"doc": "int"}, space="cosine")
    qp = QueryProcessor(InMemoryStorage(), index)
    rows = rng.standard_normal((80, 6)).astype(np.float32)
    rows[40] = rows[2]
    rows[41] = rows[2]
    rows[70] = rows[9]
    qp.upsert_many([VectorDTO(values=r.tolist(), metadata={"doc": int(i % 3), "i": i}) for i, r in enumerate(rows)], "ns")
    stored = sorted(qp.get_namespace_vectors("ns"), key=lambda v: v["metadata"]["i"])
    ids = [v["id"] for v in stored]
    found = qp.find_near_pairs(1e-6, "ns")
    assert found["complete"] and [(p["left"]["metadata"]["i"], p["right"]["metadata"]["i"]) for p in found["pairs"]] == \
        [(2, 40), (2, 41), (9, 70), (40, 41)]
    first = found["pairs"][0]
    assert first["left"]["id"] == ids[2] and np.array_equal(np.asarray(first["right"]["values"], np.float32), rows[40])
    assert abs(first["score"] - 1.0) < 1e-6
    groups = qp.find_duplicates(1e-6, "ns")
    assert [[m["metadata"]["i"] for m in g] for g in groups] == [[2, 40, 41], [9, 70]] and groups[0][1]["id"] == ids[40]
    # a dict filter runs on the device path, a predicate on the host path: the same pairs
    on_device = qp.find_near_pairs(1e-6, "ns", where={"doc": 2})
    on_host = qp.find_near_pairs(1e-6, "ns", where=lambda m: m["doc"] == 2)
    assert [(p["left"]["id"], p["right"]["id"], p["score"]) for p in on_device["pairs"]] == \
        [(p["left"]["id"], p["right"]["id"], p["score"]) for p in on_host["pairs"]] == [(ids[2], ids[41], on_host["pairs"][0]["score"])]
    assert [[m["metadata"]["i"] for m in g] for g in qp.find_duplicates(1e-6, "ns", where=lambda m: m["doc"] == 2)] == [[2, 41]]
    assert [[m["metadata"]["i"] for m in g] for g in qp.find_duplicates(1e-6, "ns", where={"doc": 2})] == [[2, 41]]
    with pytest.raises(JoinOverflow):
        qp.find_duplicates(1e-6, "ns", max_per_row=1)


# ---------------------------------------------------------------- C ABI
def _header_text():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_join.h").read_text(), flags=re.S)


def test_join_header_declares_what_the_binding_binds():
    lib = _native.load()
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", _header_text())))
    assert names == ["mlvdb_join_within"] == sorted(_native.JOIN_SIGNATURES)
    assert hasattr(lib, names[0])
    params = [p.strip() for p in re.search(r"mlvdb_join_within\((.*?)\);", _header_text(), flags=re.S).group(1).split(",")]
    restype, argtypes = _native.JOIN_SIGNATURES[names[0]]
    assert len(params) == len(argtypes) == 12 and restype is C.c_int
    ctype_of = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}
    for text, ctype in zip(params, argtypes):
        if "*" in text:
            assert ctype in (C.c_void_p, C.POINTER(_native.Where)), text
            assert ("mlvdb_where" in text) == (ctype is not C.c_void_p), text
        else:
            assert ctype is ctype_of[text.split()[0]], text
    assert [p.split()[-1].lstrip("*") for p in params] == ["h", "left_labels", "n_left", "mode", "radius", "capacity",
                                                          "total_capacity", "where", "out_labels", "out_dist", "out_offsets",
                                                          "out_counts"]
    defines = dict(re.findall(r"#define (MLVDB_JOIN_[A-Z_]+) (.+)", _header_text()))
    assert int(defines["MLVDB_JOIN_OTHERS"]) == _native.JOIN_OTHERS == 0 and int(defines["MLVDB_JOIN_LATER"]) == _native.JOIN_LATER == 1
    assert defines["MLVDB_JOIN_MAX_CAPACITY"].strip() == "(MLVDB_MAX_TOPK_PAGED - 256)"
    assert _native.JOIN_MAX_CAPACITY == _native.MAX_TOPK_PAGED - 256 == Index._MAX_JOIN_PER_ROW
    assert lib.mlvdb_abi_version() == 7


def test_join_entry_refuses_a_null_handle_inside_the_exception_guard():
    lib = _native.load()
    buf = (C.c_int64 * 4)()
    assert lib.mlvdb_join_within(C.c_void_p(), buf, 1, 0, 0.5, 1, 1, None, buf, buf, buf, buf) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()


def test_the_join_kernels_and_header_are_in_the_build():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_join\.hip\b", make, flags=re.M) and "mlvdb_join.h" in make
    kern = (ROOT / "mlvectordb_amd" / "csrc" / "kernels_join.hip").read_text()
    for name in ("join_gather_queries_kernel", "join_mask_advance_kernel", "join_strip_kernel", "join_pack_kernel"):
        assert name in kern
    assert "atomic" not in kern.split("#include", 1)[1]
