"""Recommend / discover (include/mlvdb_examples.h) without a GPU: the NumPy model against hand-computed cases, the refusals
of ``Index`` / ``QueryProcessor`` before an engine is reached, the surface over the oracle engine, the shape of the ABI, and
the entry's argument check and tile cut (csrc/examples_plan.h) in a stand-alone program under the sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import uuid
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from oracle import exact_scan
from tests.examples_helpers import (BEST, CONTEXT, DISCOVER, NEG, NO_TIER, POS, TARGET, ExamplesOracleEngine, bag_keys,
                                    model_search, tiered_topk)
from tests.where_helpers import SCHEMA, random_metadata

ROOT = Path(__file__).resolve().parents[1]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
INF = float("inf")
NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------- the model, by hand
def test_best_takes_the_nearest_liked_example_and_p_equal_n_goes_to_tier_1():
    #            row0  row1  row2  row3
    D = np.array([[1.0, 5.0, 2.0, 4.0],    # POS
                  [3.0, 0.5, 9.0, 4.0],    # POS
                  [2.0, 0.5, 1.0, 4.0],    # NEG
                  [7.0, 6.0, 8.0, 9.0]])   # NEG
    tier, value = bag_keys(BEST, D, [POS, POS, NEG, NEG])
    # row0: p 1 < n 2; row1: p 0.5 == n 0.5 -> tier 1, -0.5; row2: p 2 > n 1 -> -1; row3: 4 == 4 -> -4
    assert tier.tolist() == [0, 1, 1, 1] and value.tolist() == [1.0, -0.5, -1.0, -4.0]
    lab, tr, val, cnt = tiered_topk(tier, value, 4, np.ones(4, bool))
    assert lab.tolist() == [0, 3, 2, 1] and tr.tolist() == [0, 1, 1, 1] and cnt == 4  # tier 1: the farthest from n first


def test_best_without_negatives_and_without_positives():
    D = np.array([[3.0, 1.0, INF], [2.0, 4.0, INF]])
    tier, value = bag_keys(BEST, D, [POS, POS])
    assert tier.tolist() == [0, 0, 0] and value.tolist() == [2.0, 1.0, INF]  # +inf is an ordinary value
    tier, value = bag_keys(BEST, D, [NEG, NEG])  # no liked example: every row in tier 1, the farthest first
    assert tier.tolist() == [1, 1, 1] and value.tolist() == [-2.0, -1.0, -INF]
    assert tiered_topk(tier, value, 3, np.ones(3, bool))[0].tolist() == [2, 0, 1]
    # p = +inf against a finite n is not nearer; against n = +inf neither (inf < inf is false)
    tier, value = bag_keys(BEST, np.array([[INF, INF], [1.0, INF]]), [POS, NEG])
    assert tier.tolist() == [1, 1] and value.tolist() == [-1.0, -INF]


def test_signed_zeros_nan_and_padding():
    tier, value = bag_keys(BEST, np.array([[0.0, 0.0, 1.0], [0.0, 5.0, 1.0]]), [POS, NEG])
    assert tier.tolist() == [1, 0, 1] and bits(value).tolist() == bits([-0.0, 0.0, -1.0]).tolist()  # -n of n = 0 is -0.0
    # -0.0 == +0.0 in the ranking: among equal keys the lower label
    lab, tr, val, cnt = tiered_topk(np.zeros(3, np.int32), np.array([0.0, -0.0, 0.0]), 5, np.ones(3, bool))
    assert lab.tolist() == [0, 1, 2, -1, -1] and bits(val[:3]).tolist() == bits([0.0, -0.0, 0.0]).tolist()
    assert tr.tolist() == [0, 0, 0, NO_TIER, NO_TIER] and np.isposinf(val[3:]).all() and cnt == 3
    # a NaN value is no candidate; a NaN distance makes its minimum NaN wherever it stands
    assert bag_keys(BEST, np.array([[NAN], [1.0]]), [POS, POS])[1].tolist() != [1.0]
    assert np.isnan(bag_keys(BEST, np.array([[1.0], [NAN]]), [POS, POS])[1]).all()
    lab, _, _, cnt = tiered_topk(np.zeros(3, np.int32), np.array([2.0, NAN, 1.0]), 3, np.ones(3, bool))
    assert lab.tolist() == [2, 0, -1] and cnt == 2


def test_discover_counts_the_missed_pairs_and_with_no_pair_is_the_plain_search():
    D = np.array([[5.0, 4.0, 3.0, 2.0],    # target
                  [1.0, 2.0, 2.0, NAN],    # pos
                  [2.0, 2.0, 1.0, 1.0],    # neg   row1: equal -> missed; row3: NaN -> missed
                  [1.0, 1.0, 9.0, 0.0],    # pos
                  [3.0, 0.0, 9.5, INF]])   # neg
    tier, value = bag_keys(DISCOVER, D, [TARGET, POS, NEG, POS, NEG])
    assert tier.tolist() == [0, 2, 1, 1] and value.tolist() == [5.0, 4.0, 3.0, 2.0]
    assert tiered_topk(tier, value, 4, np.ones(4, bool))[0].tolist() == [0, 3, 2, 1]
    tier, value = bag_keys(DISCOVER, D[:1], [TARGET])
    assert tier.tolist() == [0] * 4 and tiered_topk(tier, value, 2, np.ones(4, bool))[0].tolist() == [3, 2]


def test_context_sums_in_pair_order_with_one_rounding_per_step():
    big, one = 2.0 ** 53, 1.0
    # pairs in this order: +1, +2^53, +1: ((0 + 1) + 2^53) + 1 = 2^53 + 2 in exact arithmetic; rounded per step it is
    # (1 + 2^53 -> 2^53) + 1 -> 2^53 (ties to even), and with the pairs reversed 2^53 + 1 -> 2^53, + 1 -> 2^53 as well, but
    # +2^53 last gives (1 + 1) + 2^53 = 2^53 + 2: the order is the contract
    D = np.array([[one], [0.0], [big], [0.0], [one], [0.0]])
    roles = [POS, NEG] * 3
    assert bag_keys(CONTEXT, D, roles)[1].tolist() == [big]
    assert bag_keys(CONTEXT, D[[0, 1, 4, 5, 2, 3]], roles)[1].tolist() == [big + 2]
    # a step is (dp - dn) rounded, then the sum rounded: 0.1 - (-0.2 is no distance; use) 0.3 - 0.1, then + (0.7 - 0.1)
    D = np.array([[0.3], [0.1], [0.7], [0.1]])
    assert bag_keys(CONTEXT, D, [POS, NEG] * 2)[1].tolist() == [(0.0 + (0.3 - 0.1)) + (0.7 - 0.1)]
    # inside every half-space the sum stays 0.0; dp == dn adds nothing; inf - inf is never formed
    D = np.array([[1.0, 2.0, INF], [2.0, 2.0, INF]])
    tier, value = bag_keys(CONTEXT, D, [POS, NEG])
    assert tier.tolist() == [0, 0, 0] and bits(value).tolist() == bits([0.0, 0.0, 0.0]).tolist()
    assert bag_keys(CONTEXT, np.array([[INF], [1.0]]), [POS, NEG])[1].tolist() == [INF]


def test_exclusion_drops_the_querys_own_stored_examples_only():
    D = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [5.0, 5.0, 5.0]])
    labels, roles, offsets = np.array([0, -1, 1]), np.array([POS, POS, POS]), np.array([0, 2, 3])
    live = np.ones(3, bool)
    lab, tr, val, cnt = model_search(BEST, D, labels, roles, offsets, 3, live, exclude=True)
    assert lab.tolist() == [[1, 2, -1], [0, 2, -1]] and cnt.tolist() == [2, 2]  # row 1 is query 0's raw twin: it stays
    lab, _, _, cnt = model_search(BEST, D, labels, roles, offsets, 3, live, exclude=False)
    assert lab.tolist() == [[0, 1, 2], [0, 1, 2]] and cnt.tolist() == [3, 3]


# ---------------------------------------------------------------- refusals, before the engine is touched
class UntouchableEngine(ExamplesOracleEngine):
    """Fails the test if a search of any kind reaches the engine."""

    def search(self, *a, **kw):
        raise AssertionError("the engine was touched")

    search64 = search_examples = search


def _filled(factory=ExamplesOracleEngine, n=300, d=8, seed=3, space="l2", **kw):
    rng = np.random.default_rng(seed)
    index = Index(space=space, engine_factory=factory, attributes=SCHEMA, **kw)
    metas = random_metadata(rng, n)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs, "ns")
    return rng, index, vecs, rows, metas


def test_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, vecs, rows, _ = _filled(UntouchableEngine)
    ids = [v.id for v in vecs]
    index.remove([ids[7]], "ns")
    pos = [[ids[0], ids[1]]]
    ghost = uuid.uuid4()
    with pytest.raises(ValueError, match=f"search_examples: id {ghost} is unknown or removed"):
        index.search_examples([[ids[0], ghost]], 5, "ns", "l2")
    with pytest.raises(ValueError, match=f"search_examples: id {ids[7]} is unknown or removed"):
        index.search_examples(pos, 5, "ns", "l2", negative=[[ids[7]]])
    with pytest.raises(ValueError, match=f"search_discover: id {ghost} is unknown or removed"):
        index.search_discover(5, "ns", "l2", target=[ids[0]], context=[[(ids[1], ghost)]])
    with pytest.raises(ValueError, match="query 0 holds 65 examples, at most 64"):
        index.search_examples([ids[:40]], 5, "ns", "l2", negative=[ids[40:65]])
    with pytest.raises(ValueError, match="query 0 holds 65 examples, at most 64"):
        index.search_discover(5, "ns", "l2", target=[ids[0]], context=[[(ids[1], ids[2])] * 32])
    with pytest.raises(ValueError, match="search_examples: query 1 has no example"):
        index.search_examples([[ids[0]], []], 5, "ns", "l2")
    with pytest.raises(ValueError, match="1 positive entries, 2 negative entries"):
        index.search_examples(pos, 5, "ns", "l2", negative=[[ids[2]], [ids[3]]])
    with pytest.raises(ValueError, match="query 0 has neither a target nor a context pair"):
        index.search_discover(5, "ns", "l2", context=[[]])
    with pytest.raises(ValueError, match="every context entry must be a \\(positive, negative\\) pair"):
        index.search_discover(5, "ns", "l2", context=[[(ids[0], ids[1], ids[2])]])
    with pytest.raises(ValueError, match="2 targets, 1 context entries"):
        index.search_discover(5, "ns", "l2", target=[ids[0], ids[1]], context=[[(ids[2], ids[3])]])
    with pytest.raises(ValueError, match="no finite vector of the namespace's dimensionality"):
        index.search_examples([[np.zeros(5, np.float32)]], 5, "ns", "l2")
    with pytest.raises(ValueError, match=r"positive\[0\] is one vector where the examples of query 0 are expected"):
        index.search_examples([[0.1] * 8], 5, "ns", "l2")
    with pytest.raises(ValueError, match="neither the UUID of a stored vector nor a vector"):
        index.search_examples([["not-an-id"]], 5, "ns", "l2")
    with pytest.raises(ValueError, match="neither the UUID of a stored vector nor a vector"):
        index.search_discover(5, "ns", "l2", target=[ids[0]], context=[[(ids[1], 7)]])
    with pytest.raises(ValueError, match="no finite vector of the namespace's dimensionality"):
        index.search_examples([[np.full(8, np.inf, np.float32)]], 5, "ns", "l2")
    for call in (lambda **kw: index.search_examples(pos, 5, "ns", kw.pop("metric", "l2"), **kw),
                 lambda **kw: index.search_discover(5, "ns", kw.pop("metric", "l2"), context=[[(ids[0], ids[1])]], **kw)):
        with pytest.raises(ValueError, match='metric "euclidean" is not supported'):
            call(metric="euclidean")
        with pytest.raises(ValueError, match="a per-query where list is not supported"):
            call(where=[{"year": 2000}])
        with pytest.raises(ValueError, match="where must be one dict filter"):
            call(where=lambda m: True)
        with pytest.raises(ValueError, match="allowed_ids is not supported"):
            call(allowed_ids=[ids[0]])
        with pytest.raises(ValueError, match="'nope' is not a declared attribute"):
            call(where={"nope": 1})
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="recommend: where must be one dict filter"):
        qp.recommend([ids[0]], 5, "ns", "l2", where=lambda m: True)
    with pytest.raises(ValueError, match="discover: where must be one dict filter"):
        qp.discover(5, "ns", "l2", context=[(ids[0], ids[1])], where=[{"year": 1}])


def test_a_row_sharded_index_and_an_engine_without_the_entry_are_refused():
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    with pytest.raises(ValueError, match="search_examples is not supported on a row-sharded index"):
        sharded.search_examples([[np.zeros(8, np.float32)]], 5, "ns", "l2")
    with pytest.raises(ValueError, match="search_discover is not supported on a row-sharded index"):
        sharded.search_discover(5, "ns", "l2", context=[[(np.zeros(8, np.float32), np.ones(8, np.float32))]])
    from tests.where_helpers import WhereOracleEngine

    rng = np.random.default_rng(1)
    plain = Index(space="l2", engine_factory=WhereOracleEngine)
    plain.add([Vector(values=rng.standard_normal(8).astype(np.float32), metadata={}) for _ in range(5)], "ns")
    with pytest.raises(ValueError, match="search_examples needs an engine with search_examples"):
        plain.search_examples([[np.zeros(8, np.float32)]], 5, "ns", "l2")


# ---------------------------------------------------------------- the surface, over the oracle engine
def _by_hand(D, pos, neg, skip, live):
    """BEST in Python floats for one query: sorted (tier, value, label)."""
    out = []
    for x in range(D.shape[1]):
        if x in skip or not live[x]:
            continue
        p = min((float(D[j, x]) for j in pos), default=INF)
        n = min((float(D[j, x]) for j in neg), default=INF)
        out.append((0, p, x) if pos and (not neg or p < n) else (1, -n, x))
    return sorted(out)


@pytest.mark.parametrize("space", ["l2", "cosine"])
def test_index_search_examples_returns_the_definition_by_hand(space):
    rng, index, vecs, rows, metas = _filled(space=space)
    ids = [v.id for v in vecs]
    index.remove([ids[5]], "ns")
    raw = rng.standard_normal(8).astype(np.float32)
    positive, negative = [[ids[3], raw], [ids[10]]], [[ids[20], ids[21]], []]
    hits = index.search_examples(positive, 6, "ns", space, negative=negative, where={"in_stock": True})
    live = np.array([m.get("in_stock") is True for m in metas])
    live[5] = False
    ex = np.stack([rows[3], raw, rows[20], rows[21], rows[10]])
    D = exact_scan.exact_distances(ex, rows, space)
    want = [_by_hand(D[:4], [0, 1], [2, 3], {3, 20, 21}, live)[:6], _by_hand(D[4:], [0], [], {10}, live)[:6]]
    for q in range(2):
        assert hits.labels[q].tolist() == [x for _, _, x in want[q]]
        assert hits.tiers[q].tolist() == [t for t, _, _ in want[q]]
        assert hits.values[q].tolist() == [v for _, v, _ in want[q]] == hits.scores[q].tolist()
        assert [h.vector_id for h in hits[q]] == [ids[x] for _, _, x in want[q]]
    kept = index.search_examples(positive, 6, "ns", space, negative=negative, exclude_examples=False)
    assert kept.labels[1, 0] == 10 and kept.tiers[1, 0] == 0  # the example is its own nearest row
    one = index.search_examples([ids[3], ids[10]], 4, "ns", space)  # a flat list of ids: one query
    assert one.labels.shape == (1, 4)


def test_index_search_discover_in_both_modes():
    rng, index, vecs, rows, _ = _filled(space="l2")
    ids = [v.id for v in vecs]
    target = rng.standard_normal(8).astype(np.float32)
    context = [[(ids[1], ids[2]), (rows[3] + 0.5, ids[4])]]
    hits = index.search_discover(5, "ns", "l2", target=[target], context=context)
    ex = np.stack([target, rows[1], rows[2], rows[3] + 0.5, rows[4]])
    D = exact_scan.exact_distances(ex, rows, "l2")
    keys = sorted(((int(not D[1, x] < D[2, x]) + int(not D[3, x] < D[4, x]), float(D[0, x]), x)
                   for x in range(rows.shape[0]) if x not in (1, 2, 4)))[:5]
    assert hits.labels[0].tolist() == [x for _, _, x in keys] and hits.tiers[0].tolist() == [t for t, _, _ in keys]
    assert hits.values[0].tolist() == [v for _, v, _ in keys]
    ctx = index.search_discover(5, "ns", "l2", context=context)
    sums = sorted((((0.0 + (float(D[1, x] - D[2, x]) if D[1, x] > D[2, x] else 0.0))
                    + (float(D[3, x] - D[4, x]) if D[3, x] > D[4, x] else 0.0)), x)
                  for x in range(rows.shape[0]) if x not in (1, 2, 4))[:5]
    assert ctx.labels[0].tolist() == [x for _, x in sums] and ctx.values[0].tolist() == [s for s, _ in sums]
    assert (ctx.tiers == 0).all()
    for one in (target, target.tolist(), [target.tolist()]):  # one vector in any form is the target of one query
        same = index.search_discover(5, "ns", "l2", target=one, context=context)
        assert np.array_equal(same.labels, hits.labels) and np.array_equal(same.values, hits.values)
    by_id = index.search_discover(5, "ns", "l2", target=ids[9], context=context)
    assert np.array_equal(by_id.labels, index.search_discover(5, "ns", "l2", target=[ids[9]], context=context).labels)
    plain = index.search_discover(5, "ns", "l2", target=[target], context=[[]])  # no pair: the plain search
    assert plain.labels[0].tolist() == np.argsort(D[0], kind="stable")[:5].tolist() and (plain.tiers == 0).all()


def test_top_k_is_clamped_and_the_empty_answers():
    rng, index, vecs, rows, _ = _filled(n=20)
    v = [[rows[0] + 1]]
    assert index.search_examples(v, 100, "ns", "cosine").labels.shape == (1, 20)
    assert index.search_examples(v, 5, "other", "l2").labels.shape == (1, 0)
    assert index.search_examples(v, 0, "ns", "l2").tiers.shape == (1, 0)
    assert len(index.search_examples([], 5, "ns", "l2")) == 0
    _, big, _, rows2, _ = _filled(n=100)
    assert big.search_examples(v, 100, "ns", "l2").labels.shape == (1, 64)
    hits = index.search_examples(v, 5, "ns", "l2", where={"year": {"$lt": -5}})
    assert hits.counts.tolist() == [0] and (hits.labels == -1).all() and (hits.tiers == NO_TIER).all()
    assert np.isposinf(hits.values).all() and hits[0] == []


def test_query_processor_returns_the_usual_hit_dicts_with_a_tier():
    rng = np.random.default_rng(9)
    index = Index(space="cosine", engine_factory=ExamplesOracleEngine, attributes=SCHEMA)
    qp = QueryProcessor(InMemoryStorage(), index)
    metas = random_metadata(rng, 200)
    dtos = [VectorDTO(values=rng.standard_normal(6).astype(np.float32).tolist(), metadata=m) for m in metas]
    qp.upsert_many(dtos, "ns")
    ids = index._ns["ns"].ids.uuids_at(np.arange(200)).tolist()
    positive, negative = [[ids[0], ids[1]], [ids[2]]], [[ids[3]], [ids[4], ids[5]]]
    hits = index.search_examples(positive, 7, "ns", "cosine", negative=negative)
    many = qp.recommend_many(positive, 7, "ns", "cosine", negative=negative)
    for q in range(2):
        assert [h["score"] for h in many[q]] == hits.values[q].tolist()
        assert [h["tier"] for h in many[q]] == hits.tiers[q].tolist()
        assert [h["id"] for h in many[q]] == [h.vector_id for h in hits[q]]
        assert all(set(h) == {"id", "values", "metadata", "score", "tier"} for h in many[q])
    one = qp.recommend(positive[1], 7, "ns", "cosine", negative=negative[1])
    assert [(h["id"], h["score"], h["tier"]) for h in one] == [(h["id"], h["score"], h["tier"]) for h in many[1]]
    context = [(ids[6], ids[7]), (ids[8], ids[9])]
    disc = qp.discover(5, "ns", "cosine", target=ids[10], context=context)
    want = index.search_discover(5, "ns", "cosine", target=[ids[10]], context=[context])
    assert [(h["id"], h["score"], h["tier"]) for h in disc] == [(h.vector_id, s, t) for h, s, t in
                                                                 zip(want[0], want.values[0].tolist(), want.tiers[0].tolist())]
    ctx = qp.discover_many(5, "ns", "cosine", context=[context, context[:1]])
    assert len(ctx) == 2 and all(h["tier"] == 0 for row in ctx for h in row)


# ---------------------------------------------------------------- the ABI's shape
def test_the_symbol_is_exported_and_the_prototype_matches_the_header():
    lib = _native.load()
    assert hasattr(lib, "mlvdb_search_batch_examples")
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_examples.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == sorted(_native.EXAMPLES_SIGNATURES)
    proto = re.search(r"int\s+mlvdb_search_batch_examples\s*\(([^)]*)\)", text).group(1)
    kinds = {"mlvdb_index*": _native._P, "const float*": _native._P, "const int64_t*": _native._P, "const int32_t*": _native._P,
             "int64_t": C.c_int64, "int32_t": C.c_int32, "const mlvdb_where*": C.POINTER(_native.Where),
             "int64_t*": _native._P, "double*": _native._P, "int32_t*": _native._P}
    params = [" ".join(p.split()[:-1]) for p in proto.split(",")]
    restype, argtypes = _native.EXAMPLES_SIGNATURES["mlvdb_search_batch_examples"]
    assert restype is C.c_int and argtypes == [kinds[p] for p in params]
    consts = dict(re.findall(r"#define\s+(MLVDB_EXAMPLES?_[A-Z0-9_]+)\s+(-?\d+)", text))
    for name in ("EXAMPLES_MAX", "EXAMPLES_BEST", "EXAMPLES_DISCOVER", "EXAMPLES_CONTEXT", "EXAMPLE_POS", "EXAMPLE_NEG",
                 "EXAMPLE_TARGET"):
        assert int(consts[f"MLVDB_{name}"]) == getattr(_native, name)
    assert Index._MAX_EXAMPLES == _native.EXAMPLES_MAX
    abi = (ROOT / "include" / "mlvdb_hip.h").read_text()
    assert re.search(r"#define\s+MLVDB_ABI_VERSION\s+7\b", abi) and _native.ABI_VERSION == 7


def test_the_unit_is_built_and_its_tuning_knob_is_declared():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    srcs = make[make.index("SRCS ="):make.index("OBJS =")].split()
    hdrs = make[make.index("HDRS ="):make.index("# the filter scan's body")]
    assert "kernels_examples.hip" in srcs
    assert all(h in hdrs.split() for h in ("wave_topk_tiered.h", "examples_plan.h", "../../include/mlvdb_examples.h"))
    internal = (ROOT / "mlvectordb_amd" / "csrc" / "internal.h").read_text()
    assert re.search(r'X\(examples_ws_mb, "EXAMPLES_WS_MB", 1024\)', internal)
    kernels = (ROOT / "mlvectordb_amd" / "csrc" / "kernels_examples.hip").read_text()
    assert "asm" not in re.sub(r"//.*", "", kernels) and "#pragma clang fp contract(off)" in kernels


# ---------------------------------------------------------------- the entry's host half under the sanitizers
def test_the_argument_check_and_the_tile_cut_under_the_sanitizers(tmp_path):
    # the host compiler: g++, or the clang++ that the ROCm toolchain the library is built with brings along; none is an error
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("clang++", path=f"{ROCM}/llvm/bin:{ROCM}/bin")
    assert cxx, "no host C++ compiler (g++, clang++, or the ROCm toolchain's clang++)"
    exe = tmp_path / "examples_plan_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'mlvectordb_amd' / 'csrc'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "examples_plan_main.cpp"), "-o", str(exe)],
                   capture_output=True, text=True, check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "examples_plan ok" and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr
