"""Per-query metadata filters on the MI355X (include/mlvdb_where_each.h): every route against the NumPy oracle under each
query's own mask and, bit for bit, against one single-program call per query; many tenants (the chunking); the index
lifecycle; the Index / QueryProcessor surface."""
import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, VectorDTO, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.conftest import dump_mismatch

pytestmark = pytest.mark.gpu

SCHEMA = {"v": "int"}
ALWAYS = 1 << 30  # WHERE_GATHER that gathers every program when k <= 64


def _filters(n):
    # v is a permutation of 0..n-1: none, one row, ~0.3 %, ~9 %, ~50 %, every row (before the tombstones)
    return [{"v": -5}, {"v": 123}, {"v": {"$lt": n * 3 // 1000}}, {"v": {"$gte": 1000, "$lt": 1000 + n * 9 // 100}},
            {"v": {"$lt": n // 2}}, {}]


def _engine(space, d, n, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    eng = HipScanEngine(d, space, device=0)
    eng.append(rows)
    eng.define_attr(0, "int64")
    v = rng.permutation(n).astype(np.int64)
    eng.set_attr(0, 0, v)
    tomb = np.zeros(n, bool)
    tomb[rng.choice(n, n // 10, replace=False)] = True
    eng.tombstone(np.flatnonzero(tomb))
    return eng, rows, v, tomb, rng


def _check_against_singles(eng, qs, k, programs, of, tag):
    """search_each == one search64(where=program) (or unfiltered) per program's queries, labels and fp64 bit for bit."""
    lab, dist, cnt, d64, routes = eng.search_each(qs, k, programs, of, want64=True, return_routes=True)
    for p in range(-1, len(programs)):
        sel = np.flatnonzero(of == p)
        if not sel.size:
            continue
        sl, sd, sc, s64 = eng.search64(qs[sel], k, where=None if p < 0 else programs[p])
        ok = np.array_equal(lab[sel], sl) and np.array_equal(cnt[sel], sc) and \
            np.array_equal(d64[sel].view(np.int64), s64.view(np.int64)) and np.array_equal(dist[sel], sd)
        if not ok:
            dump_mismatch(f"where_each_{tag}_p{p}", lab=lab[sel], sl=sl, cnt=cnt[sel], sc=sc, d64=d64[sel], s64=s64)
        assert ok, f"{tag} program {p} (route {routes[p] if p >= 0 else '-'})"
    return lab, cnt, routes


@pytest.mark.parametrize("d", [3, 100, 768])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_every_route_equals_the_oracle_and_the_single_calls(space, d):
    n = 40_000
    eng, rows, v, tomb, rng = _engine(space, d, n, seed=d + 7 * len(space))
    try:
        fs = _filters(n)
        programs, _ = W.compile_each(fs, SCHEMA)
        assert len(programs) == len(fs)
        nq = 36
        of = np.array([(i % (len(fs) + 1)) - 1 for i in range(nq)], np.int32)  # cycles through None and every filter
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        masks = [W_match(f, v) & ~tomb for f in fs]
        assert [int(m.sum()) for m in masks[:2]] == [0, int(not tomb[np.flatnonzero(v == 123)[0]])]
        oracle = {}  # k -> (labels, counts) of every query under its own mask
        for k in (1, 10, 64, 100):
            ol, oc = np.empty((nq, k), np.int64), np.empty(nq, np.int32)
            for p in range(-1, len(fs)):
                sel = np.flatnonzero(of == p)
                ol[sel], _, oc[sel] = exact_scan.knn(qs[sel], rows, k, space, deleted=tomb if p < 0 else ~masks[p])
            oracle[k] = ol, oc
        for gather in (0, None, ALWAYS):
            if gather is not None:
                eng.set_tuning(WHERE_GATHER=gather)
            else:
                eng.set_tuning(WHERE_GATHER=_default_gather())
            for k in (1, 10, 64, 100):
                tag = f"{space}_{d}_{gather}_{k}"
                lab, cnt, routes = _check_against_singles(eng, qs, k, programs, of, tag)
                ol, oc = oracle[k]
                assert np.array_equal(lab, ol) and np.array_equal(cnt, oc), tag
                for p, m in enumerate(masks):
                    want = _native.ROUTE_NONE if not m.any() else \
                        _native.ROUTE_SCAN if (k > 64 or gather == 0) else \
                        _native.ROUTE_GATHER if gather == ALWAYS else None
                    if want is not None:
                        assert routes[p] == want, f"{tag} program {p}: route {routes[p]}, expected {want}"
                    else:
                        assert routes[p] in (_native.ROUTE_SCAN, _native.ROUTE_GATHER)
        # the counts of every program in one pass
        assert eng.count_each(programs).tolist() == [int(m.sum()) for m in masks]
    finally:
        eng.close()


def W_match(f, v):
    from tests.where_helpers import eval_program
    return eval_program(W.compile_where(f, SCHEMA), {0: v}, v.size)


def _default_gather():
    eng = HipScanEngine(4, "l2", device=0)
    try:
        return eng.get_tuning("WHERE_GATHER")
    finally:
        eng.close()


def test_many_tenants_take_the_gathered_route_and_equal_the_oracle():
    n, d, nq, k, T = 300_000, 768, 256, 10, 997
    rng = np.random.default_rng(997)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    eng = HipScanEngine(d, "cosine", device=0)
    try:
        eng.append(rows)
        eng.define_attr(0, "int64")
        tenant = np.arange(n, dtype=np.int64) % T
        eng.set_attr(0, 0, tenant)
        tenants = rng.choice(T, nq, replace=False)
        programs, of = W.compile_each([{"v": int(t)} for t in tenants], SCHEMA)
        assert len(programs) == nq > W.EACH_MAX_PROGRAMS  # four native calls
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        lab, dist, cnt, d64, routes = eng.search_each(qs, k, programs, of, want64=True, return_routes=True)
        assert (routes == _native.ROUTE_GATHER).all(), np.unique(routes, return_counts=True)
        assert (cnt == k).all()
        for i, t in enumerate(tenants):
            idx = np.flatnonzero(tenant == t)
            ol, od, _ = exact_scan.knn(qs[i:i + 1], rows[idx], k, "cosine")
            assert np.array_equal(lab[i], idx[ol[0]]), f"query {i} tenant {t}"
            assert np.allclose(dist[i], od[0], atol=1e-5, rtol=0)
        # ... and bit for bit what the single-program calls return (a sample of them)
        for i in range(0, nq, 37):
            sl, _, sc, s64 = eng.search64(qs[i:i + 1], k, where=programs[of[i]])
            assert np.array_equal(lab[i:i + 1], sl) and np.array_equal(d64[i:i + 1].view(np.int64), s64.view(np.int64))
    finally:
        eng.close()


def test_results_follow_appends_tombstones_and_compaction():
    n, d = 20_000, 64
    eng, rows, v, tomb, rng = _engine("l2", d, n, seed=3)
    try:
        fs = _filters(n)
        programs, _ = W.compile_each(fs, SCHEMA)
        qs = rng.standard_normal((14, d), dtype=np.float32)
        of = np.array([(i % (len(fs) + 1)) - 1 for i in range(14)], np.int32)

        def check(tag):
            for gather in (0, ALWAYS):
                eng.set_tuning(WHERE_GATHER=gather)
                lab, cnt, _ = _check_against_singles(eng, qs, 10, programs, of, f"{tag}_{gather}")
                for p in range(-1, len(fs)):
                    sel = np.flatnonzero(of == p)
                    m = ~tomb if p < 0 else (W_match(fs[p], v) & ~tomb)
                    ol, _, oc = exact_scan.knn(qs[sel], rows, 10, "l2", deleted=~m)
                    assert np.array_equal(lab[sel], ol) and np.array_equal(cnt[sel], oc), f"{tag} program {p}"

        check("start")
        more = rng.standard_normal((5000, d), dtype=np.float32)
        first = eng.append(more)
        extra = np.arange(n, n + 5000, dtype=np.int64)
        eng.set_attr(0, first, extra)
        rows, v, tomb = np.vstack([rows, more]), np.concatenate([v, extra]), np.concatenate([tomb, np.zeros(5000, bool)])
        check("appended")
        gone = rng.choice(rows.shape[0], 3000, replace=False)
        eng.tombstone(gone)
        tomb[gone] = True
        check("tombstoned")
        old = eng.compact()
        rows, v, tomb = rows[old], v[old], np.zeros(old.size, bool)
        check("compacted")
    finally:
        eng.close()


def test_index_and_query_processor_surface():
    rng = np.random.default_rng(21)
    d, n = 96, 3000
    idx = Index(space="cosine", attributes={"tenant": "str", "year": "int"})
    qp = QueryProcessor(InMemoryStorage(), idx)
    metas = [{"tenant": f"t{i % 13}", "year": int(1990 + i % 30)} for i in range(n)]
    qp.upsert_many([VectorDTO(values=rng.standard_normal(d).tolist(), metadata=m) for m in metas], "ns")
    qs = rng.standard_normal((20, d)).astype(np.float32)
    wheres = [None if i % 6 == 0 else {"tenant": f"t{i % 13}", "year": {"$gte": 1990 + i}} for i in range(20)]
    got = qp.find_similar_many(qs, 7, "ns", where=wheres)
    bh = idx.search_many(qs, 7, "ns", "cosine", where=wheres)
    for i, w in enumerate(wheres):
        one = VectorDTO(values=qs[i].tolist(), metadata={})
        single = qp.find_similar(one, 7, "ns") if w is None else qp.find_similar_where(one, 7, w, "ns")
        assert got[i] == single, i
        assert [h.vector_id for h in bh[i]] == [h["id"] for h in single], i
    fs = [w for w in wheres if w is not None] + [{"tenant": "nobody"}]
    assert idx.count_many("ns", fs) == [idx.count("ns", f) for f in fs]
    with pytest.raises(ValueError):
        qp.find_similar_many(qs, 7, "ns", where=[lambda m: True] * 20)
