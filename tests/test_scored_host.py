"""Scored kNN (include/mlvdb_score.h) without a GPU: the NumPy model against hand-computed cases, the expression compiler,
the refusals of ``Index`` / ``QueryProcessor`` before an engine is reached, the surface over the oracle engine, and the
shape of the ABI."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from mlvectordb_amd import score as S
from mlvectordb_amd import where as W
from tests.scored_helpers import ScoredOracleEngine, random_score, score_eval, scored_topk
from tests.where_helpers import SCHEMA, random_metadata

ROOT = Path(__file__).resolve().parents[1]
ABSENT = W.INT64_ABSENT
NAN = float("nan")
INF = float("inf")


def P(ops, conds=()):
    return S.ScoreProgram(np.array(ops, dtype=S.OP_DTYPE), list(conds))


def c(x):
    return (S.CONST, 0, W.float_bits(x))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------- the model, by hand
def test_signed_zeros_through_min_max_neg():
    D = np.zeros((1, 1))
    ev = lambda ops: score_eval(P(ops), D, {}, [])[0, 0]
    # x <= y takes x, so MIN(-0, +0) = -0 and MIN(+0, -0) = +0: the first operand of two equal zeros
    assert bits(ev([c(-0.0), c(0.0), (S.MIN, 0, 0)])) == bits(-0.0)
    assert bits(ev([c(0.0), c(-0.0), (S.MIN, 0, 0)])) == bits(0.0)
    assert bits(ev([c(-0.0), c(0.0), (S.MAX, 0, 0)])) == bits(-0.0)
    assert bits(ev([c(0.0), c(-0.0), (S.MAX, 0, 0)])) == bits(0.0)
    assert bits(ev([c(0.0), (S.NEG, 0, 0)])) == bits(-0.0)
    assert bits(ev([c(-0.0), (S.NEG, 0, 0)])) == bits(0.0)
    assert bits(ev([c(-0.0), (S.ABS, 0, 0)])) == bits(0.0)
    assert bits(ev([c(-3.5), (S.ABS, 0, 0), (S.NEG, 0, 0)])) == bits(-3.5)
    for op in (S.MIN, S.MAX):  # a NaN on either side is NaN, unlike fmin / fmax
        assert np.isnan(ev([c(NAN), c(1.0), (op, 0, 0)])) and np.isnan(ev([c(1.0), c(NAN), (op, 0, 0)]))
    assert ev([c(2.0), c(-INF), (S.MIN, 0, 0)]) == -INF and ev([c(2.0), c(INF), (S.MAX, 0, 0)]) == INF


def test_nan_rows_are_dropped_and_infinities_rank_at_the_ends():
    # rows: 0 -> 0/0, 1 -> 1/0 = +inf, 2 -> -1/0 = -inf, 3 -> absent without a default, 4 -> 2.0, 5 -> tombstoned
    num = np.array([0.0, 1.0, -1.0, 5.0, 4.0, 1.0])
    den = np.array([0.0, 0.0, 0.0, NAN, 2.0, 1.0])
    prog = P([(S.ATTR, 0, W.float_bits(NAN)), (S.ATTR, 1, W.float_bits(NAN)), (S.DIV, 0, 0)])
    sc = score_eval(prog, np.zeros((2, 6)), {0: num, 1: den}, [])
    assert np.isnan(sc[0, 0]) and sc[0, 1] == INF and sc[0, 2] == -INF and np.isnan(sc[0, 3]) and sc[0, 4] == 2.0
    live = np.array([1, 1, 1, 1, 1, 0], bool)
    labels, scores, counts, _ = scored_topk(sc, 5, live)
    assert labels.tolist() == [[2, 4, 1, -1, -1]] * 2 and counts.tolist() == [3, 3]
    assert scores[0].tolist() == [-INF, 2.0, INF, INF, INF]  # a real +inf at rank 3, padding behind it: counts tells them apart
    # a default stands in for the absent value
    with_default = P([(S.ATTR, 0, W.float_bits(NAN)), (S.ATTR, 1, W.float_bits(5.0)), (S.DIV, 0, 0)])
    assert score_eval(with_default, np.zeros((1, 6)), {0: num, 1: den}, [])[0, 3] == 1.0
    # -0.0 == +0.0: the tie goes to the lower label
    z = np.array([[0.0, -0.0, 0.0, -0.0]])
    assert scored_topk(z, 4, np.ones(4, bool))[0].tolist() == [[0, 1, 2, 3]]


def test_ints_above_2_53_round_to_even_and_absent_ints_take_the_default():
    col = np.array([2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53) - 1, 2 ** 63 - 1, ABSENT, 7], dtype=np.int64)
    sc = score_eval(P([(S.ATTR, 0, W.float_bits(-1.5))]), np.zeros((1, 6)), {0: col}, [])[0]
    assert sc.tolist() == [float(2 ** 53), float(2 ** 53 + 4), float(-(2 ** 53)), float(2 ** 63), -1.5, 7.0]
    assert np.isnan(score_eval(P([(S.ATTR, 0, W.float_bits(NAN))]), np.zeros((1, 6)), {0: col}, [])[0, 4])


def test_every_op_is_one_rounded_operation():
    # (0.1 * 3) - 0.3: the product rounds to 0.30000000000000004 first; one fused multiply-subtract would give 2^-55
    got = score_eval(P([c(0.1), c(3.0), (S.MUL, 0, 0), c(0.3), (S.SUB, 0, 0)]), np.zeros((1, 1)), {}, [])[0, 0]
    assert got == 0.1 * 3.0 - 0.3 == 5.551115123125783e-17
    D = np.array([[0.25, 3.0]])
    m = [np.array([True, False])]
    bonus = P([(S.DIST, 0, 0), c(0.2), (S.MATCH, 0, 0), (S.MUL, 0, 0), (S.SUB, 0, 0)], [None])
    assert score_eval(bonus, D, {}, m)[0].tolist() == [0.25 - 0.2, 3.0]


# ---------------------------------------------------------------- the compiler
def ops_of(e, schema=SCHEMA):
    return [tuple(o) for o in S.compile_score(e, schema).ops.tolist()]


def test_every_grammar_form_and_the_folding_order():
    fb = W.float_bits
    assert ops_of(3) == [(S.CONST, 0, fb(3.0))] and ops_of(0.25) == [(S.CONST, 0, fb(0.25))]
    assert ops_of("$distance") == [(S.DIST, 0, 0)]
    assert ops_of({"$attr": "year"}) == [(S.ATTR, 1, fb(NAN))]
    assert ops_of({"$attr": "price", "$default": 2}) == [(S.ATTR, 2, fb(2.0))]
    assert ops_of({"$attr": "in_stock", "$default": 0.5}) == [(S.ATTR, 3, fb(0.5))]
    assert ops_of({"$neg": "$distance"}) == [(S.DIST, 0, 0), (S.NEG, 0, 0)]
    assert ops_of({"$abs": 1}) == [(S.CONST, 0, fb(1.0)), (S.ABS, 0, 0)]
    assert ops_of({"$sub": [1, 2]}) == [c(1.0), c(2.0), (S.SUB, 0, 0)]
    assert ops_of({"$div": ["$distance", 2]}) == [(S.DIST, 0, 0), c(2.0), (S.DIV, 0, 0)]
    for name, op in (("$add", S.ADD), ("$mul", S.MUL), ("$min", S.MIN), ("$max", S.MAX)):  # n-ary: ((1 op 2) op 3) op 4
        assert ops_of({name: [1, 2, 3, 4]}) == [c(1.0), c(2.0), (op, 0, 0), c(3.0), (op, 0, 0), c(4.0), (op, 0, 0)]
        assert ops_of({name: [7]}) == [c(7.0)]
    prog = S.compile_score({"$add": [{"$match": {"genre": "jazz"}}, {"$match": {"year": {"$gte": 2000}}}]}, SCHEMA,
                           {"genre": {"jazz": 4}})
    assert [tuple(o) for o in prog.ops.tolist()] == [(S.MATCH, 0, 0), (S.MATCH, 0, 1), (S.ADD, 0, 0)]
    assert [tuple(o) for o in prog.conds[0].ops.tolist()] == [(W.EQ, 0, 4, 0)]
    assert [tuple(o) for o in prog.conds[1].ops.tolist()] == [(W.GE, 1, 2000, 0)]
    # the three recipes compile, and fold as written
    bonus = {"$sub": ["$distance", {"$mul": [0.2, {"$match": {"genre": "jazz"}}]}]}
    assert ops_of(bonus) == [(S.DIST, 0, 0), c(0.2), (S.MATCH, 0, 0), (S.MUL, 0, 0), (S.SUB, 0, 0)]
    pop = {"$div": ["$distance", {"$add": [1, {"$attr": "year", "$default": 0}]}]}
    assert ops_of(pop) == [(S.DIST, 0, 0), c(1.0), (S.ATTR, 1, fb(0.0)), (S.ADD, 0, 0), (S.DIV, 0, 0)]
    age = {"$add": ["$distance", {"$mul": [0.3, {"$min": [1, {"$div": [{"$abs": {"$sub": [{"$attr": "year"}, 2024]}}, 10]}]}]}]}
    assert ops_of(age) == [(S.DIST, 0, 0), c(0.3), c(1.0), (S.ATTR, 1, fb(NAN)), c(2024.0), (S.SUB, 0, 0), (S.ABS, 0, 0),
                           c(10.0), (S.DIV, 0, 0), (S.MIN, 0, 0), (S.MUL, 0, 0), (S.ADD, 0, 0)]


def right_nested(n):
    """An expression whose evaluation holds n values at once: 1 - (1 - (1 - ... ))."""
    e = 1
    for _ in range(n - 1):
        e = {"$sub": [1, e]}
    return e


def test_limits_of_depth_length_and_filters():
    assert len(ops_of(right_nested(8))) == 15  # depth 8: accepted
    with pytest.raises(ValueError, match="a stack 9 deep; the device evaluates at most 8"):
        S.compile_score(right_nested(9), SCHEMA)
    assert len(ops_of({"$add": [1] * 16})) == 31
    assert len(ops_of({"$neg": {"$add": [1] * 16}})) == 32  # 32 ops: accepted
    with pytest.raises(ValueError, match="compiles to 33 ops; the device evaluates at most 32"):
        S.compile_score({"$add": [1] * 17}, SCHEMA)
    match = {"$match": {"year": 2000}}
    assert len(S.compile_score({"$add": [match] * 8}, SCHEMA).conds) == 8
    with pytest.raises(ValueError, match=r"9 \$match filters; the device evaluates at most 8"):
        S.compile_score({"$add": [match] * 9}, SCHEMA)
    wide = {"$match": {"$or": [{"year": y} for y in range(20)]}}  # 39 filter ops each
    with pytest.raises(ValueError, match=r"\$match filters compile to 78 ops; the device evaluates at most 64"):
        S.compile_score({"$add": [wide, wide]}, SCHEMA)


def test_compile_errors_name_the_offending_sub_expression():
    wide = dict(SCHEMA, tags="str[]", loc="geo", terms="sparse", code="bits64")
    for name, kind in (("genre", "str"), ("tags", r"str\[\]"), ("loc", "geo"), ("terms", "sparse"), ("code", "bits64")):
        with pytest.raises(ValueError, match=f"'{name}' is a {kind} attribute"):
            S.compile_score({"$add": ["$distance", {"$attr": name}]}, wide)
    for bad, what in ((("$distance", 1), "is not an expression"), ("$dist", "'\\$dist' is not an expression"),
                      (None, "None is not an expression"), (True, "True is not an expression"),
                      ({"$pow": [1, 2]}, "unknown operator '\\$pow'"), ({"$sub": [1]}, "\\$sub takes a list of exactly two"),
                      ({"$div": [1, 2, 3]}, "\\$div takes a list of exactly two"), ({"$add": []}, "\\$add takes a list of at least one"),
                      ({"$add": 1}, "\\$add takes a list"), ({"$neg": 1, "$abs": 2}, "exactly one operator"),
                      ({"$attr": "nope"}, "'nope' is not a declared attribute"),
                      ({"$attr": "year", "$default": "x"}, "\\$default must be a number"),
                      ({"$attr": "year", "$else": 1}, "takes '\\$attr' and '\\$default' only"),
                      ({"$match": 3}, "\\$match takes a filter dict"),
                      ({"$match": {"nope": 1}}, "in \\{'\\$match': \\{'nope': 1\\}\\}: 'nope' is not a declared attribute")):
        with pytest.raises(ValueError, match=what):
            S.compile_score({"$add": [1, bad]}, SCHEMA)


def test_random_scores_stay_within_the_limits():
    rng = np.random.default_rng(5)
    for _ in range(200):
        _, prog = random_score(rng, SCHEMA)
        assert 1 <= prog.ops.size <= S.MAX_OPS and len(prog.conds) <= S.MAX_CONDS
        depth = deepest = 0
        for op, _, _ in prog.ops.tolist():
            depth += 1 if op <= S.MATCH else -1 if op <= S.MAX else 0
            assert depth >= 1
            deepest = max(deepest, depth)
        assert depth == 1 and deepest <= S.MAX_DEPTH


# ---------------------------------------------------------------- refusals, before the engine is touched
class UntouchableEngine(ScoredOracleEngine):
    """Fails the test if a search of any kind reaches the engine."""

    def search(self, *a, **kw):
        raise AssertionError("the engine was touched")

    search64 = search_scored = search


def _filled(factory=ScoredOracleEngine, n=500, d=8, seed=3, space="l2", **kw):
    rng = np.random.default_rng(seed)
    index = Index(space=space, engine_factory=factory, attributes=SCHEMA, **kw)
    metas = random_metadata(rng, n)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs, "ns")
    return rng, index, vecs, rows, metas


def test_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, vecs, _, _ = _filled(UntouchableEngine)
    qs = np.zeros((3, 8), np.float32)
    with pytest.raises(ValueError, match='metric "euclidean" is not supported'):
        index.search_scored(qs, 5, "ns", "euclidean", "$distance")
    with pytest.raises(ValueError, match="a per-query where list is not supported"):
        index.search_scored(qs, 5, "ns", "l2", "$distance", where=[{"year": 2000}] * 3)
    with pytest.raises(ValueError, match="where must be a dict filter"):
        index.search_scored(qs, 5, "ns", "l2", "$distance", where=lambda m: True)
    with pytest.raises(ValueError, match="allowed_ids is not supported"):
        index.search_scored(qs, 5, "ns", "l2", "$distance", allowed_ids=[vecs[0].id])
    with pytest.raises(ValueError, match="'genre' is a str attribute"):
        index.search_scored(qs, 5, "ns", "l2", {"$attr": "genre"})
    with pytest.raises(ValueError, match="a stack 9 deep"):
        index.search_scored(qs, 5, "ns", "l2", right_nested(9))
    with pytest.raises(ValueError, match="compiles to 33 ops"):
        index.search_scored(qs, 5, "ns", "l2", {"$add": [1] * 17})
    with pytest.raises(ValueError, match=r"9 \$match filters"):
        index.search_scored(qs, 5, "ns", "l2", {"$add": [{"$match": {"year": 1}}] * 9})
    with pytest.raises(ValueError, match="'nope' is not a declared attribute"):
        index.search_scored(qs, 5, "ns", "l2", "$distance", where={"nope": 1})
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="find_similar_scored: where must be one dict filter"):
        qp.find_similar_scored_many(qs, 5, "$distance", "ns", "l2", where=lambda m: True)
    with pytest.raises(ValueError, match="find_similar_scored: where must be one dict filter"):
        qp.find_similar_scored(VectorDTO(values=[0.0] * 8, metadata={}), 5, "$distance", "ns", "l2", where=[{"year": 1}])


def test_a_row_sharded_index_is_refused():
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    with pytest.raises(ValueError, match="search_scored is not supported on a row-sharded index"):
        sharded.search_scored(np.zeros((1, 8), np.float32), 5, "ns", "l2", "$distance")


# ---------------------------------------------------------------- the surface, over the oracle engine
RECIPES = {
    "bonus": {"$sub": ["$distance", {"$mul": [0.2, {"$match": {"genre": "jazz"}}]}]},
    "popularity": {"$div": ["$distance", {"$add": [1, {"$attr": "price", "$default": 0}]}]},
    "age": {"$add": ["$distance", {"$mul": [0.3, {"$min": [1, {"$div": [{"$abs": {"$sub": [{"$attr": "year"}, 2024]}}, 10]}]}]}]},
}


def recipe_by_hand(name, d, meta):
    """The recipe's value for one row in Python floats (IEEE doubles), from its metadata dict; None = dropped."""
    if name == "bonus":
        return d - 0.2 * (1.0 if meta.get("genre") == "jazz" else 0.0)
    if name == "popularity":
        p = meta.get("price")
        return d / (1.0 + (0.0 if p is None or p != p else float(p)))
    y = meta.get("year")
    return None if y is None else d + 0.3 * min(1.0, abs(float(y) - 2024.0) / 10.0)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_index_search_scored_returns_the_recipes_by_hand(name):
    from oracle import exact_scan

    rng, index, vecs, rows, metas = _filled()
    qs = rng.standard_normal((4, 8)).astype(np.float32)
    D = exact_scan.exact_distances(qs, rows, "l2")
    hits = index.search_scored(qs, 10, "ns", "l2", RECIPES[name], where={"in_stock": True})
    for q in range(4):
        want = sorted((s, i) for i, m in enumerate(metas) if m.get("in_stock") is True
                      for s in [recipe_by_hand(name, float(D[q, i]), m)] if s is not None)[:10]
        assert hits.labels[q].tolist() == [i for _, i in want]
        assert hits.scores[q].tolist() == [s for s, _ in want]
        assert hits.distances[q].tolist() == [float(D[q, i]) for _, i in want]
        assert [h.vector_id for h in hits[q]] == [vecs[i].id for _, i in want]
    assert hits.counts.tolist() == [10] * 4


def test_top_k_is_clamped_and_the_empty_answers():
    rng, index, vecs, rows, _ = _filled(n=20)
    qs = rng.standard_normal((2, 8)).astype(np.float32)
    assert index.search_scored(qs, 100, "ns", "cosine", "$distance").labels.shape == (2, 20)
    assert len(index.search_scored(qs, 5, "other", "l2", "$distance")) == 2
    assert index.search_scored(qs, 5, "other", "l2", "$distance").distances.shape == (2, 0)
    assert index.search_scored(qs[:0], 5, "ns", "l2", "$distance").labels.shape == (0, 0)
    assert index.search_scored(qs, 0, "ns", "l2", "$distance").labels.shape == (2, 0)
    _, big, _, _, _ = _filled(n=100)
    assert big.search_scored(qs, 100, "ns", "l2", "$distance").labels.shape == (2, 64)
    hits = index.search_scored(qs, 5, "ns", "l2", {"$attr": "year"}, where={"year": {"$exists": False}})
    assert hits.counts.tolist() == [0, 0] and (hits.labels == -1).all() and np.isinf(hits.scores).all()


def test_query_processor_returns_the_usual_hit_dicts():
    rng = np.random.default_rng(9)
    index = Index(space="cosine", engine_factory=ScoredOracleEngine, attributes=SCHEMA)
    qp = QueryProcessor(InMemoryStorage(), index)
    metas = random_metadata(rng, 200)
    dtos = [VectorDTO(values=rng.standard_normal(6).astype(np.float32).tolist(), metadata=m) for m in metas]
    qp.upsert_many(dtos, "ns")
    qs = rng.standard_normal((3, 6)).astype(np.float32)
    hits = index.search_scored(qs, 7, "ns", "cosine", RECIPES["bonus"])
    many = qp.find_similar_scored_many(qs, 7, RECIPES["bonus"], "ns", "cosine")
    for q in range(3):
        assert [h["score"] for h in many[q]] == hits.scores[q].tolist()
        assert [h["id"] for h in many[q]] == [h.vector_id for h in hits[q]]
        assert all(set(h) == {"id", "values", "metadata", "score"} for h in many[q])
    one = qp.find_similar_scored(VectorDTO(values=qs[1].tolist(), metadata={}), 7, RECIPES["bonus"], "ns", "cosine")
    assert [(h["id"], h["score"]) for h in one] == [(h["id"], h["score"]) for h in many[1]]


# ---------------------------------------------------------------- the ABI's shape
def test_the_symbol_is_exported_and_the_prototype_matches_the_header():
    lib = _native.load()
    assert hasattr(lib, "mlvdb_search_batch_scored")
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_score.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == sorted(_native.SCORE_SIGNATURES)
    proto = re.search(r"int\s+mlvdb_search_batch_scored\s*\(([^)]*)\)", text).group(1)
    kinds = {"mlvdb_index*": _native._P, "const float*": _native._P, "int64_t": C.c_int64, "int32_t": C.c_int32,
             "const mlvdb_score*": C.POINTER(_native.Score), "const mlvdb_where*": C.POINTER(_native.Where),
             "int64_t*": _native._P, "double*": _native._P, "int32_t*": _native._P}
    params = [" ".join(p.split()[:-1]) for p in proto.split(",")]
    restype, argtypes = _native.SCORE_SIGNATURES["mlvdb_search_batch_scored"]
    assert restype is C.c_int and argtypes == [kinds[p] for p in params]
    consts = dict(re.findall(r"#define\s+(MLVDB_SCORE_[A-Z0-9_]+)\s+(-?\d+)", text))
    for name in ("MAX_OPS", "MAX_DEPTH", "MAX_CONDS", "CONST", "DIST", "ATTR", "MATCH", "ADD", "SUB", "MUL", "DIV", "MIN", "MAX",
                 "NEG", "ABS"):
        assert int(consts[f"MLVDB_SCORE_{name}"]) == getattr(_native, f"SCORE_{name}")
    assert (S.MAX_OPS, S.MAX_DEPTH, S.MAX_CONDS) == (_native.SCORE_MAX_OPS, _native.SCORE_MAX_DEPTH, _native.SCORE_MAX_CONDS)
    assert [S.CONST, S.DIST, S.ATTR, S.MATCH, S.ADD, S.SUB, S.MUL, S.DIV, S.MIN, S.MAX, S.NEG, S.ABS] == list(range(12))
    assert S.OP_DTYPE.itemsize == 16 and C.sizeof(_native.Score) == 32  # mlvdb_score_op, mlvdb_score
