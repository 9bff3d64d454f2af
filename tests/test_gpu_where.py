"""Metadata filters on the MI355X: the device-evaluated row mask against the NumPy oracle and against the host-mask path,
through the engine, the Index lifecycle and the QueryProcessor."""
import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, VectorDTO
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from mlvectordb_amd.vector import Vector
from oracle import exact_scan
from tests.conftest import dump_mismatch
from tests.where_helpers import SCHEMA, py_match, random_metadata

pytestmark = pytest.mark.gpu

BUCKET = {"bucket": "int", "score": "float"}
# selectivity from no row to every row: bucket = label % 1000, score = NaN on every 7th row
FILTERS = [
    {"bucket": {"$lt": 0}},                                   # none
    {"bucket": {"$in": [3, 500, 999]}},                       # 0.3 %
    {"bucket": {"$lt": 100}, "score": {"$exists": True}},    # ~8.6 %
    {"$or": [{"score": {"$lt": 0.0}}, {"bucket": {"$gte": 900}}]},  # ~50 %
    {"$not": {"bucket": {"$lt": 0}}},                          # all
]


def _make(space, d, n, strategy, seed, capacity_hint=0):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    eng = HipScanEngine(d, space, device=0, strategy=strategy, capacity_hint=capacity_hint)
    eng.append(rows)
    eng.define_attr(0, "int64")
    eng.define_attr(1, "float64")
    bucket = np.arange(n, dtype=np.int64) % 1000
    score = rng.standard_normal(n)
    score[::7] = np.nan
    eng.set_attr(0, 0, bucket)
    eng.set_attr(1, 0, score)
    tomb = np.zeros(n, bool)
    tomb[rng.choice(n, n // 10, replace=False)] = True
    eng.tombstone(np.flatnonzero(tomb))
    return eng, rows, {0: bucket, 1: score}, tomb, rng


def _match(f, cols, n):
    from tests.where_helpers import eval_program
    return eval_program(W.compile_where(f, BUCKET), cols, n)


@pytest.mark.parametrize("d", [3, 100, 768])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_knn_and_range_where_equal_the_oracle(space, d):
    n = 40_000
    for strategy in ("auto", "exact", "filter"):
        eng, rows, cols, tomb, rng = _make(space, d, n, strategy, seed=d + len(space))
        qs = rng.standard_normal((12, d), dtype=np.float32)
        try:
            for fi, f in enumerate(FILTERS):
                prog = W.compile_where(f, BUCKET)
                match = _match(f, cols, n)
                live_match = match & ~tomb
                assert eng.where_count(prog) == int(live_match.sum())
                assert np.array_equal(eng.where_labels(prog), np.flatnonzero(live_match))
                for k in (1, 10, 64, 100, 300):
                    lab, dist, cnt, d64 = eng.search64(qs, k, where=prog)
                    ol, od, oc = exact_scan.knn(qs, rows, k, space, deleted=tomb | ~match)
                    tag = f"{space}_{d}_{strategy}_{fi}_{k}"
                    if not (np.array_equal(lab, ol) and np.array_equal(cnt, oc)):
                        dump_mismatch(f"where_{tag}", lab=lab, ol=ol, cnt=cnt, oc=oc)
                    assert (cnt == min(k, int(live_match.sum()))).all(), tag
                    assert np.array_equal(lab, ol) and np.array_equal(cnt, oc), tag
                    assert np.allclose(dist, od, atol=1e-5, rtol=0), tag
                    hl, hd, hc, h64 = eng.search64(qs, k, mask=live_match.astype(np.uint8))
                    assert np.array_equal(lab, hl) and np.array_equal(cnt, hc), tag
                    assert np.array_equal(d64.view(np.int64), h64.view(np.int64)), tag  # bit for bit
                if strategy == "exact":
                    continue
                dd = exact_scan.exact_distances(qs[:4], rows, space)
                radius = float(np.sort(dd, axis=1)[:, 300].mean())
                got = eng.range(qs[:4], radius, 4096, where=prog)
                want = exact_scan.range_query(qs[:4], rows, radius, space, deleted=tomb | ~match)
                for qi, (g, w) in enumerate(zip(got, want)):
                    assert np.array_equal(g[0], w[0]), f"range {space}_{d}_{strategy}_{fi} q{qi}"
                    assert np.allclose(g[1], w[1], atol=1e-5, rtol=0)
        finally:
            eng.close()


def test_refused_programs_are_status_codes_not_faults():
    eng, rows, cols, tomb, rng = _make("cosine", 64, 2000, "auto", seed=1)
    try:
        def prog(ops, table=()):
            return W.Program(np.array(ops, dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))
        bad = [
            prog([(W.AND, 0, 0, 0)]),                                   # stack underflow
            prog([(W.TRUE, 0, 0, 0), (W.TRUE, 0, 0, 0)]),                # ends at depth 2
            prog([(W.EQ, 5, 1, 0)]),                                    # undefined attribute
            prog([(W.EQ, 99, 1, 0)]),                                   # attribute out of range
            prog([(W.IN, 1, 0, 1)], [1]),                               # IN on a float64 column
            prog([(W.IN, 0, 0, 3)], [1, 2]),                            # set range outside the table
            prog([(W.IN, 0, 0, 2)], [2, 1]),                            # unsorted range
            prog([(42, 0, 0, 0)]),                                      # unknown op
            prog([(W.TRUE, 0, 0, 0)] * 65 + [(W.AND, 0, 0, 0)] * 64),   # too long
        ]
        for p in bad:
            with pytest.raises(RuntimeError, match=r"\(1\)"):
                eng.where_count(p)
            with pytest.raises(RuntimeError, match=r"\(1\)"):
                eng.search(rows[:2], 3, where=p)
        assert eng.where_count(W.compile_where({}, BUCKET)) == int((~tomb).sum())  # the handle still works
    finally:
        eng.close()


def _check_index(index, live, q, tag):
    for f in ({"genre": "jazz"}, {"year": {"$gte": 1990, "$lt": 2010}}, {"$or": [{"price": {"$lt": 20}},
              {"in_stock": False}]}, {"genre": {"$nin": ["rock", "pop"]}}, {}):
        want = [v.id for v in live if py_match(f, v.metadata)]
        assert index.query_by_metadata("ns", f) == want, (tag, f)
        assert index.count("ns", f) == len(want), (tag, f)
        got = index.search_many(q, 10, "ns", "cosine", where=f)
        if want:
            ref = index.search_many(q, 10, "ns", "cosine", allowed_ids=want)
            assert [[(h.vector_id, h.score) for h in r] for r in got] == \
                [[(h.vector_id, h.score) for h in r] for r in ref], (tag, f)
            rows = np.stack([v.values for v in live])
            ids = [v.id for v in live]
            deleted = np.array([not py_match(f, v.metadata) for v in live])
            ol, _, oc = exact_scan.knn(q, rows, min(10, len(want)), "cosine", deleted=deleted)
            assert [[h.vector_id for h in r] for r in got] == [[ids[j] for j in ol[i, :oc[i]]] for i in range(len(q))], (tag, f)
        else:
            assert all(len(r) == 0 for r in got)


def test_index_lifecycle_keeps_filters_exact(tmp_path):
    rng = np.random.default_rng(11)
    d = 256
    index = Index(space="cosine", capacity_hint=3000, attributes=SCHEMA)
    mk = lambda m: Vector(values=rng.standard_normal(d).astype(np.float32), metadata=m)  # noqa: E731
    first = [mk(m) for m in random_metadata(rng, 2500)]
    index.add(first, "ns")
    q = rng.standard_normal((8, d)).astype(np.float32)
    live = list(first)
    _check_index(index, live, q, "add")
    # append after a search, the attributes of the new rows set later (add_arrays: rows first, then values)
    more = [mk(m) for m in random_metadata(rng, 1500)]  # regrowth past capacity_hint
    index.add(more, "ns")
    live += more
    _check_index(index, live, q, "append+regrowth")
    extra_meta = random_metadata(rng, 300)
    rows = rng.standard_normal((300, d)).astype(np.float32)
    ids = index.add_arrays(rows, "ns", attributes=index.extract_attributes(extra_meta))
    from uuid import UUID
    for r, m, raw in zip(rows, extra_meta, ids):
        v = Vector(values=r, metadata=m)
        v._id = UUID(bytes=bytes(raw))
        live.append(v)
    _check_index(index, live, q, "add_arrays")
    gone = {v.id for v in live[::4]}
    index.remove(list(gone), "ns")
    live = [v for v in live if v.id not in gone]
    _check_index(index, live, q, "tombstones")
    assert index.compact("ns")
    _check_index(index, live, q, "compact")
    index.save_index(str(tmp_path))
    back = Index(space="cosine", attributes=SCHEMA)
    assert back.load_index(str(tmp_path))
    _check_index(back, live, q, "load")
    back.close()
    index.rebuild({"ns": live}, "cosine")  # closes the engines, re-ingests: reset + fresh dictionaries
    _check_index(index, live, q, "rebuild")
    eng = index._ns["ns"].engine
    eng.reset()  # values dropped, definitions kept
    assert eng.counts() == (0, 0)
    eng.append(rng.standard_normal((10, d)).astype(np.float32))
    assert eng.where_count(W.compile_where({"year": {"$exists": True}}, SCHEMA)) == 0
    assert eng.where_count(W.compile_where({}, SCHEMA)) == 10
    index.close()


def test_query_processor_dict_where_equals_the_callable():
    rng = np.random.default_rng(12)
    d = 128
    qp = QueryProcessor(InMemoryStorage(), Index(space="cosine", attributes=SCHEMA))
    qp.upsert_many([VectorDTO(values=rng.standard_normal(d).tolist(), metadata=m) for m in random_metadata(rng, 3000)], "ns")
    q = rng.standard_normal((16, d)).astype(np.float32)
    for f in ({"genre": {"$in": ["jazz", "blues"]}, "year": {"$gte": 1980}}, {"price": {"$lt": 10}}, {"genre": "zydeco"}):
        pred = lambda m, f=f: py_match(f, m)  # noqa: E731
        a = qp.find_similar_many(q, 10, "ns", where=f)
        b = qp.find_similar_many(q, 10, "ns", where=pred)
        assert [[(h["id"], h["score"], h["metadata"]) for h in r] for r in a] == \
            [[(h["id"], h["score"], h["metadata"]) for h in r] for r in b], f
        one = VectorDTO(values=q[0].tolist(), metadata={})
        ra = qp.find_in_radius(one, 0.95, "ns", where=f)
        rb = qp.find_in_radius(one, 0.95, "ns", where=pred)
        assert [(h["id"], h["score"]) for h in ra] == [(h["id"], h["score"]) for h in rb], f
        assert qp.count_where(f, "ns") == qp.count_where(pred, "ns")
