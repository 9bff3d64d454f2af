"""Scored kNN on the MI355X (include/mlvdb_score.h).
1. Replay: the model of tests/scored_helpers.py run on the device's own bits -- ``pair_distances(queries, all labels)`` for
   DIST, the columns read back with ``get_attr``, the cond masks from ``where_labels`` -- must reproduce ``search_scored``
   bit for bit (labels, scores, counts, dist64).  No tolerance: it holds for any input, ties, NaN and infinities included.
2. Against the NumPy oracle (``exact_scan.exact_distances`` for DIST): equal labels and scores within SCORE_ATOL, under the
   precondition -- asserted on the CPU for every query -- that the oracle's consecutive scores through rank k + 1 differ by
   more than GAP_MIN.
3. Structure: identical bytes from two calls, a split batch, mutations, an empty index, no query, the C-level refusals.
4. The Index / QueryProcessor surface on the three recipes.
Rows are Gaussian."""
import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO
from mlvectordb_amd import score as S
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.conftest import dump_mismatch
from tests.helpers import SCORE_ATOL
from tests.scored_helpers import GAP_MIN, ScoredOracleEngine, random_score, score_eval, scored_topk
from tests.where_helpers import SCHEMA, random_filter, random_metadata

pytestmark = pytest.mark.gpu

NAN = float("nan")
fb = W.float_bits
TRUE = W.Program(np.array([(W.TRUE, 0, 0, 0)], dtype=W.OP_DTYPE), np.zeros(0, np.int64))
INT, FLT, LIST, GEO, BIG = 0, 1, 2, 3, 4  # the columns of the engine-level corpus
NUMERIC = {INT: np.int64, FLT: np.float64, BIG: np.int64}


def P(ops, conds=()):
    return S.ScoreProgram(np.array(ops, dtype=S.OP_DTYPE), list(conds))


def c(x):
    return (S.CONST, 0, fb(x))


def W1(op, attr, a=0, b=0, table=()):
    return W.Program(np.array([(op, attr, a, b)], dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _corpus(space, n, d, seed, tomb=0.0):
    """An engine of n Gaussian rows with an int column (duplicates, zeros, absents), a float column (duplicates, signed
    zeros, an infinity, NaN = absent), a list column, a geo column and an int column of values beyond 2^53."""
    rng = np.random.default_rng(seed)
    eng = HipScanEngine(d, space, device=0)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    eng.append(rows)
    for a, kind in ((INT, "int64"), (FLT, "float64"), (LIST, "int64_list"), (GEO, "geo"), (BIG, "int64")):
        eng.define_attr(a, kind)
    ints = rng.integers(-2, 6, n).astype(np.int64)
    ints[rng.random(n) < 0.15] = W.INT64_ABSENT
    flts = rng.choice(np.array([0.0, -0.0, 1.5, -2.25, 3.0, 0.5, np.inf, 1e-300]), n)
    flts[rng.random(n) < 0.15] = NAN
    big = rng.choice(np.array([2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53) - 1, 2 ** 63 - 1, 5, 0, W.INT64_ABSENT], dtype=np.int64), n)
    lists = [None if rng.random() < 0.1 else sorted(set(rng.integers(0, 10, rng.integers(0, 5)).tolist())) for _ in range(n)]
    geo = np.array([W.geo_pack((float(rng.uniform(-60, 60)), float(rng.uniform(-170, 170)))) for _ in range(n)], dtype=np.int64)
    geo[rng.random(n) < 0.1] = W.INT64_ABSENT
    eng.set_attr(INT, 0, ints)
    eng.set_attr(FLT, 0, flts)
    eng.set_attr(BIG, 0, big)
    eng.set_attr(GEO, 0, geo)
    eng.set_attr_list(LIST, 0, W.encode_list_column("tags", "int[]", lists, {}))
    if tomb:
        eng.tombstone(np.flatnonzero(rng.random(n) < tomb))
    return eng, rng


def _mask(labels, n):
    m = np.zeros(n, bool)
    m[labels] = True
    return m


class Bits:
    """What the model reads, from the device: the distances of every (query, row) pair, the numeric columns, the live rows."""

    def __init__(self, eng, qs, columns=NUMERIC):
        self.eng, self.qs = eng, qs
        self.n = eng.counts()[0]
        self.D = np.zeros((qs.shape[0], self.n))
        if self.n and qs.shape[0]:
            self.D = eng.pair_distances(qs, np.broadcast_to(np.arange(self.n), (qs.shape[0], self.n)))[0]
        self.cols = {a: eng.get_attr(a, 0, self.n, dt) for a, dt in columns.items()}
        self.live = _mask(eng.where_labels(TRUE), self.n) if self.n else np.zeros(0, bool)

    def want(self, prog, k, where=None, nq=None):
        masks = [_mask(self.eng.where_labels(cond), self.n) for cond in prog.conds]
        live = self.live if where is None else _mask(self.eng.where_labels(where), self.n)
        D = self.D if nq is None else self.D[:nq]
        return scored_topk(score_eval(prog, D, self.cols, masks), k, live, D)


NAMES = ("labels", "scores", "counts", "dist64")


def _replay(b, prog, k, tag, where=None, nq=None):
    """``search_scored`` against the model on the device's own bits: every output, bit for bit."""
    qs = b.qs if nq is None else b.qs[:nq]
    got = b.eng.search_scored(qs, k, prog, where=where, want64=True)
    want = b.want(prog, k, where, nq)
    for name, g, w in zip(NAMES, got, want):
        if g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
            dump_mismatch(f"scored_{tag}", **{f"got_{n}": a for n, a in zip(NAMES, got)},
                          **{f"want_{n}": a for n, a in zip(NAMES, want)})
            bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))
            raise AssertionError(f"{tag}: {name} differs in {bad.size} queries, first {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")
    without = b.eng.search_scored(qs, k, prog, where=where)
    assert len(without) == 3 and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(without, got[:3]))
    return got


# ---------------------------------------------------------------- 1. replay of the device's own bits
def attr(a, default=NAN):
    return (S.ATTR, a, fb(default))


def op(o):
    return (o, 0, 0)


EIGHT_CONDS = [W1(W.GE, INT, 2), W1(W.HAS_ANY, LIST, 0, 3, (1, 4, 7)),
               W1(W.GEO_BOX, GEO, W.geo_pack((-30.0, -90.0)), W.geo_pack((45.0, 120.0))), W1(W.LT, FLT, fb(1.0)),
               W1(W.EXISTS, BIG), W1(W.HAS, LIST, 3), W1(W.IN, INT, 0, 2, (0, 3)), W1(W.LEN, LIST, 2, 4)]
# ((m0 * 2 + m1) * 2 + ...) * 2 + m7, then + DIST: every cond bit has its own weight
HORNER = [(S.MATCH, 0, 0)] + [t for i in range(1, 8) for t in (c(2.0), op(S.MUL), (S.MATCH, 0, i), op(S.ADD))]
FIXED = {
    "dist": P([op(S.DIST)]),
    "const": P([c(3.25)]),
    "int": P([attr(INT)]),
    "float": P([attr(FLT)]),
    "big": P([attr(BIG)]),
    "big_plus_dist": P([attr(BIG, 0.0), op(S.DIST), op(S.ADD)]),
    # eight values on the stack at once, then seven binary ops
    "depth8": P([attr(INT, 0.0), attr(FLT, 1.0), op(S.DIST), c(2.0), attr(BIG, 4.0), c(0.5), op(S.DIST), c(3.0),
                 op(S.ADD), op(S.MUL), op(S.MIN), op(S.SUB), op(S.MAX), op(S.ADD), op(S.DIV)]),
    # 16 pushes, 15 binary ops and a NEG
    "ops32": P([op(S.DIST)] + [t for i in range(15) for t in
                               ((c(0.1 * (i + 1)), attr(INT, 1.0), attr(FLT, 2.0), op(S.DIST))[i % 4],
                                op((S.ADD, S.MUL, S.SUB, S.MAX, S.MIN)[i % 5]))] + [op(S.NEG)]),
    "conds8": P(HORNER + [op(S.DIST), op(S.ADD)], EIGHT_CONDS),
    "absent_dropped": P([op(S.DIST), attr(INT), op(S.ADD)]),
    "absent_default": P([op(S.DIST), attr(INT, 100.0), op(S.ADD)]),
    "nan_default_twice": P([attr(INT), attr(INT, 7.0), op(S.MIN)]),
    # FLT / INT: 0/0 = NaN (dropped), x/0 = +-inf, -0.0 / 5 = -0.0, inf / 0 = inf
    "div": P([attr(FLT, 0.0), attr(INT, 0.0), op(S.DIV)]),
    "abs_neg": P([op(S.DIST), attr(FLT), op(S.SUB), op(S.ABS), op(S.NEG)]),
}

SHAPES = ((1, 3), (15, 16), (16, 3), (17, 100), (1000, 16), (5000, 100), (300, 768))
BATCHES = ((1, 1), (9, 10), (70, 64))  # (nq, k): past one query tile and into a second grid row; one, some, all lanes of a list


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_search_scored_equals_the_model_replayed_on_the_devices_own_bits(space, n, d):
    assert len(FIXED["ops32"].ops) == 32 and len(FIXED["conds8"].conds) == 8
    eng, rng = _corpus(space, n, d, 7 * n + d + len(space), tomb=1 / 3 if n == 5000 else 0.0)
    try:
        qs = rng.standard_normal((70, d), dtype=np.float32)
        b = Bits(eng, qs)
        for nq, k in BATCHES:
            for name, prog in FIXED.items():
                got = _replay(b, prog, k, f"{space}_{n}x{d}_{nq}_{k}_{name}", nq=nq)
                if name == "dist" and k <= b.live.sum():  # the plain search's labels and distances, bit for bit
                    lab, _, cnt, d64 = eng.search64(qs[:nq], k)
                    assert np.array_equal(lab, got[0]) and np.array_equal(cnt, got[2])
                    assert np.array_equal(_bits(d64), _bits(got[1])) and np.array_equal(_bits(d64), _bits(got[3]))
                if name == "const":  # all rows tie: the first k live labels
                    first = np.flatnonzero(b.live)[:k]
                    assert (got[0][:, :first.size] == first).all() and (got[2] == first.size).all()
        # a filter in front: tombstones and the mask act as in search_batch_where; few candidates leave padding behind them
        where = W1(W.EQ, INT, 3)
        got = _replay(b, FIXED["depth8"], 64, f"{space}_{n}x{d}_where", where=where)
        assert (got[2] <= eng.where_count(where)).all()
    finally:
        eng.close()


def _schema_index(n, d, seed, space="l2"):
    rng = np.random.default_rng(seed)
    index = Index(space=space, attributes=SCHEMA)
    metas = random_metadata(rng, n)
    index.add([Vector(values=rng.standard_normal(d).astype(np.float32), metadata=m) for m in metas], "ns")
    return rng, index, index._ns["ns"], metas


SCHEMA_COLS = {0: np.int64, 1: np.int64, 2: np.float64, 3: np.int64}  # genre codes, year, price, in_stock


def test_forty_random_programs_over_random_metadata():
    rng, index, ns, _ = _schema_index(2000, 16, 11)
    qs = rng.standard_normal((9, 16), dtype=np.float32)
    b = Bits(ns.engine, qs, SCHEMA_COLS)
    for i in range(40):
        expr, prog = random_score(rng, SCHEMA, ns.strings)
        where = W.compile_where(random_filter(rng), SCHEMA, ns.strings) if i % 2 else None
        _replay(b, prog, (1, 10, 64)[i % 3], f"random_{i}", where=where)


# ---------------------------------------------------------------- 2. against the NumPy oracle
ORACLE_RECIPES = {
    "bonus": {"$sub": ["$distance", {"$mul": [0.2, {"$match": {"genre": "jazz"}}]}]},
    "popularity": {"$div": ["$distance", {"$add": [1, {"$attr": "price", "$default": 0}]}]},
    "age": {"$add": ["$distance", {"$mul": [0.3, {"$min": [1, {"$div": [{"$abs": {"$sub": [{"$attr": "year"}, 2024]}}, 10]}]}]}]},
}


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_search_scored_equals_the_numpy_oracle_where_its_scores_are_apart(space):
    n, d, k = 3000, 48, 10
    rng = np.random.default_rng(21)
    metas = random_metadata(rng, n)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((16, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    oracle = Index(space=space, attributes=SCHEMA, engine_factory=ScoredOracleEngine)
    device = Index(space=space, attributes=SCHEMA)
    oracle.add(vecs, "ns")
    device.add(vecs, "ns")
    for name, expr in ORACLE_RECIPES.items():
        want = oracle.search_scored(qs, k + 1, "ns", space, expr)
        gaps = np.diff(want.scores, axis=1)
        assert (want.counts == k + 1).all() and (gaps > GAP_MIN).all(), \
            f"{name}: precondition: oracle scores closer than {GAP_MIN} ({gaps.min()}): choose another seed"
        got = device.search_scored(qs, k, "ns", space, expr)
        print(f"{space} {name}: max |score - oracle| {np.abs(got.scores - want.scores[:, :k]).max():.3e}, "
              f"max |dist - oracle| {np.abs(got.distances - want.distances[:, :k]).max():.3e}, min gap {gaps.min():.3e}")
        assert np.array_equal(got.labels, want.labels[:, :k]) and (got.counts == k).all()
        assert np.abs(got.scores - want.scores[:, :k]).max() <= SCORE_ATOL
        assert np.abs(got.distances - want.distances[:, :k]).max() <= SCORE_ATOL


# ---------------------------------------------------------------- 3. structure
def test_two_calls_return_identical_bytes_and_a_split_batch_the_same_answer():
    eng, rng = _corpus("cosine", 5000, 100, 3, tomb=0.2)
    try:
        qs = rng.standard_normal((70, 100), dtype=np.float32)
        for prog in (FIXED["conds8"], FIXED["ops32"], FIXED["div"]):
            one = eng.search_scored(qs, 10, prog, want64=True)
            two = eng.search_scored(qs, 10, prog, want64=True)
            head = eng.search_scored(qs[:1], 10, prog, want64=True)
            tail = eng.search_scored(qs[1:], 10, prog, want64=True)
            for a, b2, h, t in zip(one, two, head, tail):
                assert a.tobytes() == b2.tobytes()
                assert a.tobytes() == np.concatenate([h, t]).tobytes()
    finally:
        eng.close()


def test_mutations_are_followed():
    rng, index, ns, metas = _schema_index(1500, 24, 5)
    qs = rng.standard_normal((9, 24), dtype=np.float32)
    exprs = [ORACLE_RECIPES["age"], ORACLE_RECIPES["bonus"], {"$attr": "price"}]

    def check(tag):
        b = Bits(ns.engine, qs, SCHEMA_COLS)
        for j, e in enumerate(exprs):
            _replay(b, S.compile_score(e, SCHEMA, ns.strings), 10, f"mutate_{tag}_{j}",
                    where=W.compile_where({"in_stock": True}, SCHEMA, ns.strings) if j == 1 else None)
        return b

    check("fresh")
    uuids = ns.ids.uuids_at(np.arange(0, 1500, 7)).tolist()
    assert index.update_attributes(uuids[:100], {"year": 2024, "genre": "jazz", "price": None}, "ns") > 0
    check("updated")
    index.remove(uuids[100:160], "ns")
    check("removed")
    assert index.remove_where("ns", {"year": {"$lt": 1960}}) > 0
    b = check("removed_where")
    assert not b.live.all()
    index.compact("ns")
    b = check("compacted")
    assert b.live.all() and b.n < 1500


def test_an_empty_index_and_no_query():
    eng = HipScanEngine(8, "l2", device=0)
    try:
        eng.define_attr(INT, "int64")
        qs = np.ones((3, 8), np.float32)
        lab, sc, cnt, d64 = eng.search_scored(qs, 5, FIXED["absent_default"], want64=True)
        assert (lab == -1).all() and np.isposinf(sc).all() and (cnt == 0).all() and np.isposinf(d64).all()
        eng.append(np.ones((4, 8), np.float32))
        lab, sc, cnt = eng.search_scored(qs[:0], 5, FIXED["dist"])
        assert lab.shape == (0, 5) and sc.shape == (0, 5) and cnt.shape == (0,)
        lab, sc, cnt, d64 = eng.search_scored(qs, 5, FIXED["absent_default"], where=W1(W.EXISTS, INT), want64=True)
        assert (lab == -1).all() and (cnt == 0).all()  # no row matches the filter
        eng.tombstone(np.arange(4))
        lab, sc, cnt = eng.search_scored(qs, 5, FIXED["dist"])
        assert (lab == -1).all() and np.isposinf(sc).all() and (cnt == 0).all()
    finally:
        eng.close()


def test_the_c_level_refusals_launch_nothing():
    eng, rng = _corpus("l2", 100, 8, 1)
    try:
        eng.define_attr(5, "sparse")
        eng.define_attr(6, "bits")
        qs = rng.standard_normal((2, 8), dtype=np.float32)
        eng.last_stats()
        ok = W1(W.EXISTS, INT)
        invalid = {
            "stack underflow (binary)": P([op(S.DIST), op(S.ADD)]),
            "stack underflow (unary)": P([op(S.NEG)]),
            "final depth 2": P([op(S.DIST), c(1.0)]),
            "depth 9": P([c(1.0)] * 9 + [op(S.ADD)] * 8),
            "33 ops": P([c(1.0)] + [c(1.0), op(S.ADD)] * 16),
            "no op": P(np.zeros(0, dtype=S.OP_DTYPE).tolist()),
            "unknown op": P([(12, 0, 0)]),
            "undefined attr": P([attr(9)]),
            "attr out of range": P([attr(16)]),
            "list attr": P([attr(LIST)]),
            "geo attr": P([attr(GEO)]),
            "sparse attr": P([attr(5)]),
            "bits attr": P([attr(6)]),
            "match without conds": P([(S.MATCH, 0, 0)]),
            "match past conds": P([(S.MATCH, 0, 1)], [ok]),
            "match below conds": P([(S.MATCH, 0, -1)], [ok]),
            "a cond that leaves two values": P([(S.MATCH, 0, 0)], [W.Program(np.array([(W.TRUE, 0, 0, 0)] * 2, dtype=W.OP_DTYPE),
                                                                              np.zeros(0, np.int64))]),
            "a cond on an undefined attr": P([(S.MATCH, 0, 0)], [W1(W.EQ, 9, 1)]),
            "a cond whose set range leaves its table": P([(S.MATCH, 0, 0)], [W1(W.IN, INT, 0, 3, (1, 2))]),
            "nine conds": P([(S.MATCH, 0, 0)], [ok] * 9),
            "conds of 65 ops": P([(S.MATCH, 0, 0)], [W.Program(np.array([(W.TRUE, 0, 0, 0)] + [(W.NOT, 0, 0, 0)] * 32,
                                                                        dtype=W.OP_DTYPE), np.zeros(0, np.int64))] * 2),
        }
        for what, prog in invalid.items():
            with pytest.raises(RuntimeError, match=r"search_batch_scored failed \(1\)"):
                eng.search_scored(qs, 5, prog)
        with pytest.raises(RuntimeError, match=r"search_batch_scored failed \(1\)"):  # a bad outer filter
            eng.search_scored(qs, 5, FIXED["dist"], where=W1(W.EQ, 9, 1))
        with pytest.raises(RuntimeError, match=r"search_batch_scored failed \(1\)"):
            eng.search_scored(qs, 0, FIXED["dist"])
        with pytest.raises(RuntimeError, match=r"search_batch_scored failed \(6\).*MLVDB_MAX_TOPK"):
            eng.search_scored(qs, 65, FIXED["dist"])
        st = eng.last_stats()
        assert st["scan_launches"] == 0 and st["rows_scanned"] == 0
        _replay(Bits(eng, qs), FIXED["conds8"], 64, "after_refusals")  # the handle is as good as before
        assert eng.last_stats()["scan_launches"] >= 1
    finally:
        eng.close()


# ---------------------------------------------------------------- 4. the surface
TIERS = {"tier": "str", "likes": "int", "year": "int"}
RECIPES = {
    "bonus": {"$sub": ["$distance", {"$mul": [0.2, {"$match": {"tier": "gold"}}]}]},
    "popularity": {"$div": ["$distance", {"$add": [1, {"$attr": "likes", "$default": 0}]}]},
    "age": {"$add": ["$distance", {"$mul": [0.3, {"$min": [1, {"$div": [{"$abs": {"$sub": [{"$attr": "year"}, 2024]}}, 10]}]}]}]},
}


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_index_and_query_processor_return_the_models_answer_for_the_recipes(metric):
    rng = np.random.default_rng(31)
    index = Index(space=metric, attributes=TIERS)
    qp = QueryProcessor(InMemoryStorage(), index)
    dtos = []
    for i in range(500):
        m = {"tier": ("gold", "silver", "bronze")[int(rng.integers(3))]}
        if rng.random() < 0.8:
            m["likes"] = int(rng.integers(0, 50))
        if rng.random() < 0.8:
            m["year"] = int(rng.integers(1990, 2025))
        dtos.append(VectorDTO(values=rng.standard_normal(12).astype(np.float32).tolist(), metadata=m))
    qp.upsert_many(dtos, "ns")
    ns = index._ns["ns"]
    qs = rng.standard_normal((5, 12), dtype=np.float32)
    b = Bits(ns.engine, qs, {0: np.int64, 1: np.int64, 2: np.int64})
    for name, expr in RECIPES.items():
        lab, sc, cnt, d64 = b.want(S.compile_score(expr, TIERS, ns.strings), 10)
        hits = index.search_scored(qs, 10, "ns", metric, expr)
        assert np.array_equal(hits.labels, lab) and np.array_equal(hits.counts, cnt)
        assert np.array_equal(_bits(hits.scores), _bits(sc)) and np.array_equal(_bits(hits.distances), _bits(d64))
        many = qp.find_similar_scored_many(qs, 10, expr, "ns", metric)
        for q in range(5):
            m = int(cnt[q])
            assert [h["id"] for h in many[q]] == ns.ids.uuids_at(lab[q, :m]).tolist()
            assert [h["score"] for h in many[q]] == sc[q, :m].tolist()
            assert [h.vector_id for h in hits[q]] == ns.ids.uuids_at(lab[q, :m]).tolist()
        one = qp.find_similar_scored(VectorDTO(values=qs[2].tolist(), metadata={}), 10, expr, "ns", metric)
        assert [(h["id"], h["score"]) for h in one] == [(h["id"], h["score"]) for h in many[2]]
        assert cnt.min() == 10 or name == "age"  # (age drops the rows without a year; 400 remain)
