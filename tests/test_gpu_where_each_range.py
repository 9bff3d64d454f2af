"""Per-query metadata filters in batched range search on the MI355X (include/mlvdb_where_each_range.h): every route against
the NumPy oracle under each query's own mask and, bit for bit, against one single-program range call per program's queries;
the capacity rules; the GATHER route's list overflow; ties; many tenants (the chunking); the index lifecycle; the
Index / QueryProcessor surface.  Every comparison is exact: integer labels and the bit patterns of the distances."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.conftest import dump_mismatch

pytestmark = pytest.mark.gpu

SCHEMA = {"v": "int"}
ALWAYS = 1 << 30  # WHERE_GATHER that gathers every program
H = _native.WHERE_EACH_RANGE_LIST  # hits per query the GATHER route lists


def _filters(n):
    # v is a permutation of 0..n-1: none, one row, ~0.3 %, ~9 %, ~50 %, every row (before the tombstones)
    return [{"v": -5}, {"v": 123}, {"v": {"$lt": n * 3 // 1000}}, {"v": {"$gte": 1000, "$lt": 1000 + n * 9 // 100}},
            {"v": {"$lt": n // 2}}, {}]


def _match(f, v):
    from tests.where_helpers import eval_program
    return eval_program(W.compile_where(f, SCHEMA), {0: v}, v.size)


def _engine(space, d, n, seed, rows=None):
    rng = np.random.default_rng(seed)
    if rows is None:
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


def _default_gather():
    eng = HipScanEngine(4, "l2", device=0)
    try:
        return eng.get_tuning("WHERE_GATHER")
    finally:
        eng.close()


def _native_each(eng, qs, radius, capacity, total, programs, of):
    """The native batched call -> (status, labels, dist, offsets, counts, routes); labels / dist prefilled with a sentinel."""
    qs = np.ascontiguousarray(qs, np.float32)
    of = np.ascontiguousarray(of, np.int32)
    nq = qs.shape[0]
    labels, dist = np.full(max(total, 1), -7, np.int64), np.full(max(total, 1), -7.0, np.float32)
    offsets, counts = np.full(nq + 1, -7, np.int64), np.full(nq, -7, np.int64)
    routes = np.full(max(len(programs), 1), -7, np.int32)
    arr, keep = eng._where_array(programs)
    rc = eng._lib.mlvdb_range_batch_packed_where_each(eng._h, qs.ctypes.data, nq, float(radius), capacity, total, arr,
                                                      len(programs), of.ctypes.data, labels.ctypes.data, dist.ctypes.data,
                                                      offsets.ctypes.data, counts.ctypes.data, routes.ctypes.data)
    return rc, labels, dist, offsets, counts, routes[:len(programs)]


def _native_single(eng, qs, radius, capacity, total, program):
    """The native single-filter call (unfiltered when ``program`` is None) -> (status, labels, dist, offsets, counts)."""
    qs = np.ascontiguousarray(qs, np.float32)
    nq = qs.shape[0]
    labels, dist = np.full(max(total, 1), -7, np.int64), np.full(max(total, 1), -7.0, np.float32)
    offsets, counts = np.full(nq + 1, -7, np.int64), np.full(nq, -7, np.int64)
    if program is None:
        rc = eng._lib.mlvdb_range_batch_packed(eng._h, qs.ctypes.data, nq, float(radius), capacity, total, labels.ctypes.data,
                                               dist.ctypes.data, offsets.ctypes.data, counts.ctypes.data)
    else:
        w, keep = eng._where(program)
        rc = eng._lib.mlvdb_range_batch_packed_where(eng._h, qs.ctypes.data, nq, float(radius), capacity, total, C.byref(w),
                                                     labels.ctypes.data, dist.ctypes.data, offsets.ctypes.data,
                                                     counts.ctypes.data)
    return rc, labels, dist, offsets, counts


def _check_against_singles(eng, qs, radius, capacity, programs, of, tag, total=None):
    """The batched native call == one single-filter native call per program's queries (same radius and capacity): status
    class, counts, and every query's labels and fp32 distances bit for bit.  -> (per-query label arrays, counts, routes)."""
    nq = qs.shape[0]
    total = nq * min(capacity, _native.MAX_TOPK_PAGED) if total is None else total
    rc, lab, dist, off, cnt, routes = _native_each(eng, qs, radius, capacity, total, programs, of)
    assert rc in (_native.OK, _native.ERR_OVERFLOW), (tag, rc)
    assert off[0] == 0 and np.all(np.diff(off) == np.minimum(cnt, capacity)), tag
    want_rc = _native.OK
    for p in range(-1, len(programs)):
        sel = np.flatnonzero(of == p)
        if not sel.size:
            continue
        src, sl, sd, so, sc = _native_single(eng, qs[sel], radius, capacity, total, None if p < 0 else programs[p])
        assert src in (_native.OK, _native.ERR_OVERFLOW), (tag, p, src)
        want_rc = max(want_rc, src)
        ok = np.array_equal(cnt[sel], sc)
        for j, i in enumerate(sel):
            a, b = lab[off[i]:off[i + 1]], sl[so[j]:so[j + 1]]
            ok = ok and np.array_equal(a, b) and \
                np.array_equal(dist[off[i]:off[i + 1]].view(np.int32), sd[so[j]:so[j + 1]].view(np.int32))
        if not ok:
            dump_mismatch(f"where_each_range_{tag}_p{p}", lab=lab, off=off, cnt=cnt[sel], sl=sl, so=so, sc=sc, dist=dist, sd=sd)
        assert ok, f"{tag} program {p} (route {routes[p] if p >= 0 else '-'})"
    assert rc == want_rc, (tag, rc, want_rc)  # OVERFLOW exactly when some single call overflows its capacity
    return [lab[off[i]:off[i + 1]] for i in range(nq)], cnt, routes


def _oracle_radii(qs, rows, tomb, space):
    """Two radii from the oracle's distances of the queries to the live rows: one that makes ~0.5 % of the live rows hits, and
    the median of the queries' nearest distances (about half the queries have no hit at all, even unfiltered)."""
    dist = exact_scan.exact_distances(qs, rows[~tomb], space)
    wide = np.float32(np.quantile(dist, 0.005))
    narrow = np.float32(np.median(dist.min(axis=1)))
    zero = int((dist.min(axis=1) > float(narrow)).sum())
    assert 0 < zero < qs.shape[0], "the narrow radius leaves some queries, not all, without a hit"
    assert 0.002 < (dist <= float(wide)).mean() < 0.01
    return float(wide), float(narrow)


@pytest.mark.parametrize("d", [3, 100, 768])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_every_route_equals_the_oracle_and_the_single_calls(space, d):
    n = 40_000 if d < 768 else 16_000
    eng, rows, v, tomb, rng = _engine(space, d, n, seed=d + 7 * len(space))
    try:
        fs = _filters(n)
        programs, _ = W.compile_each(fs, SCHEMA)
        assert len(programs) == len(fs)
        nq = 35
        of = np.array([(i % (len(fs) + 1)) - 1 for i in range(nq)], np.int32)  # cycles through None and every filter
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        masks = [_match(f, v) & ~tomb for f in fs]
        default = _default_gather()
        for radius in _oracle_radii(qs, rows, tomb, space):
            want = [None] * nq  # the oracle's labels of every query under its own mask
            for p in range(-1, len(fs)):
                sel = np.flatnonzero(of == p)
                res = exact_scan.range_query(qs[sel], rows, radius, space, deleted=tomb if p < 0 else ~masks[p])
                for j, i in enumerate(sel):
                    want[i] = res[j][0]
            assert max(w.size for w in want) < H
            for gather in (0, default, ALWAYS):
                eng.set_tuning(WHERE_GATHER=gather)
                tag = f"{space}_{d}_{gather}_{radius:.4g}"
                lab, cnt, routes = _check_against_singles(eng, qs, radius, _native.MAX_TOPK_PAGED, programs, of, tag)
                for i in range(nq):
                    assert np.array_equal(lab[i], want[i]) and cnt[i] == want[i].size, f"{tag} query {i} (program {of[i]})"
                for p, m in enumerate(masks):
                    forced = _native.ROUTE_NONE if not m.any() else \
                        _native.ROUTE_SCAN if gather == 0 else _native.ROUTE_GATHER if gather == ALWAYS else None
                    if forced is not None:
                        assert routes[p] == forced, f"{tag} program {p}: route {routes[p]}, expected {forced}"
                    else:
                        assert routes[p] in (_native.ROUTE_SCAN, _native.ROUTE_GATHER)
                # ... and the same through the engine's own protocol
                hits = eng.range_each(qs, radius, 64, programs, of)
                for p in range(-1, len(fs)):
                    sel = np.flatnonzero(of == p)
                    single = eng.range(qs[sel], radius, 64, where=None if p < 0 else programs[p])
                    for j, i in enumerate(sel):
                        assert np.array_equal(hits[i][0], single[j][0]) and np.array_equal(hits[i][0], want[i]), (tag, i)
                        assert np.array_equal(hits[i][1].view(np.int32), single[j][1].view(np.int32)), (tag, i)
    finally:
        eng.close()


def test_capacity_semantics():
    n, d, space = 30_000, 32, "l2"
    eng, rows, v, tomb, rng = _engine(space, d, n, seed=41)
    try:
        fs = _filters(n)[2:]
        programs, _ = W.compile_each(fs, SCHEMA)
        nq = 20
        of = np.array([(i % (len(fs) + 1)) - 1 for i in range(nq)], np.int32)
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        radius, _ = _oracle_radii(qs, rows, tomb, space)
        masks = [_match(f, v) & ~tomb for f in fs]
        exact = np.array([exact_scan.range_query(qs[i:i + 1], rows, radius, space,
                                                 deleted=tomb if of[i] < 0 else ~masks[of[i]])[0][0].size for i in range(nq)])
        cap = 5
        assert (exact > cap).any() and (exact < cap).any()
        for gather in (0, ALWAYS):
            eng.set_tuning(WHERE_GATHER=gather)
            # a capacity below some counts: the nearest `capacity`, exact counts, the single call's status
            lab, cnt, _ = _check_against_singles(eng, qs, radius, cap, programs, of, f"cap_{gather}")
            assert np.array_equal(cnt, exact)
            rc = _native_each(eng, qs, radius, cap, nq * cap, programs, of)[0]
            assert rc == _native.ERR_OVERFLOW
            for i in range(nq):
                full = exact_scan.range_query(qs[i:i + 1], rows, radius, space, deleted=tomb if of[i] < 0 else ~masks[of[i]])
                assert np.array_equal(lab[i], full[0][0][:cap]), i
            # the engine: truncate=True keeps the nearest `capacity`, truncate=False brings every hit back
            cut, full = eng.range_each(qs, radius, cap, programs, of, truncate=True), eng.range_each(qs, radius, cap, programs, of)
            for p in range(-1, len(fs)):
                sel = np.flatnonzero(of == p)
                scut = eng.range(qs[sel], radius, cap, truncate=True, where=None if p < 0 else programs[p])
                for j, i in enumerate(sel):
                    assert np.array_equal(cut[i][0], scut[j][0]) and np.array_equal(cut[i][0], lab[i])
                    assert np.array_equal(cut[i][1].view(np.int32), scut[j][1].view(np.int32))
                    assert full[i][0].size == exact[i] and np.array_equal(full[i][0][:cap], lab[i])
            # total_capacity too small: offsets and counts are right, nothing is written
            need = int(exact.sum())
            rc, lab2, dist2, off2, cnt2, _ = _native_each(eng, qs, radius, _native.MAX_TOPK_PAGED, need - 1, programs, of)
            assert rc == _native.ERR_OVERFLOW
            assert np.array_equal(cnt2, exact) and np.array_equal(np.diff(off2), exact) and off2[0] == 0
            assert (lab2 == -7).all() and (dist2 == -7.0).all()
            rc, lab3, _, off3, cnt3, _ = _native_each(eng, qs, radius, _native.MAX_TOPK_PAGED, need, programs, of)
            assert rc == _native.OK and np.array_equal(off3, off2) and np.array_equal(cnt3, exact)
        # validation: a status, nothing launched
        bad = of.copy()
        bad[3] = len(programs)
        assert _native_each(eng, qs, radius, 4, 64, programs, bad)[0] == 1
        bad[3] = -2
        assert _native_each(eng, qs, radius, 4, 64, programs, bad)[0] == 1
        assert _native_each(eng, qs, radius, 0, 64, programs, of)[0] == 1
        assert _native_each(eng, qs, radius, 4, -1, programs, of)[0] == 1
        assert _native_each(eng, qs, radius, 4, 64, programs * 17, of)[0] == 1  # 68 programs
    finally:
        eng.close()


def test_list_overflow_on_the_gather_route_is_served_by_the_scan_route():
    n, d, space = 40_000, 3, "l2"
    eng, rows, v, tomb, rng = _engine(space, d, n, seed=17)
    try:
        f = {"v": {"$lt": n * 6 // 10}}
        programs, _ = W.compile_each([f], SCHEMA)
        mask = _match(f, v) & ~tomb
        assert mask.sum() > 2 * H
        qs = np.array([[0.0, 0.0, 0.0], [4.5, 0.0, 0.0]], np.float32)  # the middle of the cloud, and its edge
        dist = exact_scan.exact_distances(qs, rows[mask], space)
        radius = float(np.float32(np.sort(dist[0])[H + 3000]))
        want = exact_scan.range_query(qs, rows, radius, space, deleted=~mask)
        assert want[0][0].size > H and 0 < want[1][0].size < H // 4
        of = np.zeros(2, np.int32)
        eng.set_tuning(WHERE_GATHER=ALWAYS)
        eng.last_stats()
        single = eng.range(qs[:1], radius, _native.MAX_TOPK_PAGED, where=programs[0])  # (room for every hit: one native call)
        alone = eng.last_stats()["fallback_queries"]
        hits, routes = eng.range_each(qs, radius, _native.MAX_TOPK_PAGED, programs, of, return_routes=True)
        both = eng.last_stats()["fallback_queries"]
        assert routes.tolist() == [_native.ROUTE_GATHER]
        for i in range(2):
            assert np.array_equal(hits[i][0], want[i][0]), i
        assert np.array_equal(hits[0][0], single[0][0]) and np.array_equal(hits[0][1].view(np.int32), single[0][1].view(np.int32))
        # one query left the GATHER route (on top of what the masked pass of that query counts for itself); the other stayed
        assert both == alone + 1, (both, alone)
        hits1 = eng.range_each(qs[1:], radius, _native.MAX_TOPK_PAGED, programs, of[:1])
        assert eng.last_stats()["fallback_queries"] == 0
        assert np.array_equal(hits1[0][0], want[1][0])
        _check_against_singles(eng, qs, radius, _native.MAX_TOPK_PAGED, programs, of, "list_overflow")
    finally:
        eng.close()


def test_more_than_256_gathered_queries_in_one_native_call():
    """300 gathered queries: two 256-query groups of the GATHER route.  Sorted by program the second program's queries begin at
    position 254, so its first tile is cut at 256 (no tile straddles two groups) and the group loop runs twice."""
    n, d, space = 2000, 16, "l2"
    eng, rows, v, tomb, rng = _engine(space, d, n, seed=256)
    try:
        fs = [{"v": {"$lt": 40}}, {"v": {"$gte": 100, "$lt": 150}}, {"v": {"$gte": 500, "$lt": 530}}]
        programs, _ = W.compile_each(fs, SCHEMA)
        masks = [_match(f, v) & ~tomb for f in fs]
        assert all(24 <= m.sum() <= 50 for m in masks)  # a few dozen rows each
        of = rng.permutation(np.repeat(np.arange(3, dtype=np.int32), [254, 6, 40]))
        nq = of.size
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        # the radius from the oracle's distances of every query to its own program's rows: a tenth of the queries have no hit
        nearest = np.empty(nq)
        for p, m in enumerate(masks):
            sel = np.flatnonzero(of == p)
            nearest[sel] = exact_scan.exact_distances(qs[sel], rows[m], space).min(axis=1)
        radius = float(np.float32(np.quantile(nearest, 0.9)))
        want = np.empty(nq, np.int64)
        for p, m in enumerate(masks):
            sel = np.flatnonzero(of == p)
            want[sel] = [r[0].size for r in exact_scan.range_query(qs[sel], rows, radius, space, deleted=~m)]
        assert (want == 0).any() and ((want >= 1) & (want <= 50)).mean() > 0.5 and want.max() <= 50
        eng.set_tuning(WHERE_GATHER=ALWAYS)
        lab, cnt, routes = _check_against_singles(eng, qs, radius, 64, programs, of, "two_groups")
        assert routes.tolist() == [_native.ROUTE_GATHER] * 3
        assert np.array_equal(cnt, want)
    finally:
        eng.close()


def test_ties_come_out_in_ascending_label_order_on_both_routes():
    n, d, space = 12_000, 24, "cosine"
    rng = np.random.default_rng(77)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows[rng.choice(n, 3000, replace=False)] = rows[5]  # 3000 copies of one row, spread over the tenants
    eng, rows, v, tomb, rng = _engine(space, d, n, seed=78, rows=rows)
    try:
        fs = [{"v": {"$lt": n // 3}}, {"v": {"$gte": n // 3}}]
        programs, _ = W.compile_each(fs, SCHEMA)
        qs = np.stack([rows[5] + 0.01 * rng.standard_normal(d, dtype=np.float32) for _ in range(4)]).astype(np.float32)
        of = np.array([0, 1, 0, 1], np.int32)
        radius = 0.01
        for gather in (0, ALWAYS):
            eng.set_tuning(WHERE_GATHER=gather)
            lab, cnt, routes = _check_against_singles(eng, qs, radius, _native.MAX_TOPK_PAGED, programs, of, f"ties_{gather}")
            assert (routes == (_native.ROUTE_SCAN if gather == 0 else _native.ROUTE_GATHER)).all()
            for i in range(4):
                want = exact_scan.range_query(qs[i:i + 1], rows, radius, space, deleted=~(_match(fs[of[i]], v) & ~tomb))[0][0]
                assert want.size > 500 and np.array_equal(lab[i], want), i
                assert np.all(np.diff(lab[i]) > 0)  # the copies tie exactly: the label alone orders them
    finally:
        eng.close()


def test_many_tenants_in_one_call_equal_the_loop_of_single_filter_calls():
    n, d, T = 30_000, 64, 200
    rng = np.random.default_rng(200)
    idx = Index(space="l2", attributes={"tenant": "int"})
    rows = rng.standard_normal((n, d), dtype=np.float32)
    tenant = rng.integers(0, T, n)
    idx.add([Vector(values=r, metadata={"tenant": int(t)}) for r, t in zip(rows, tenant)], "ns")
    qs = rows[rng.choice(n, T, replace=False)] + 0.3 * rng.standard_normal((T, d), dtype=np.float32)
    wheres = [{"tenant": int(t)} for t in rng.permutation(T)]
    programs, _ = W.compile_each(wheres, {"tenant": "int"})
    assert len(W.chunk_programs(programs, np.arange(T, dtype=np.int32))) == 4  # four native calls
    radius = float(np.float32(np.quantile(exact_scan.exact_distances(qs[:20], rows, "l2"), 0.02)))
    got = idx.range_search_many(qs, radius, "ns", "l2", where=wheres)
    assert sum(len(g) for g in got) > T
    for i, w in enumerate(wheres):
        one = idx.range_search_many(qs[i:i + 1], radius, "ns", "l2", where=w)[0]
        assert [(h.vector_id, h.score) for h in got[i]] == [(h.vector_id, h.score) for h in one], i


def test_results_follow_appends_tombstones_and_compaction():
    n, d = 20_000, 64
    eng, rows, v, tomb, rng = _engine("l2", d, n, seed=3)
    try:
        fs = _filters(n)
        programs, _ = W.compile_each(fs, SCHEMA)
        qs = rng.standard_normal((14, d), dtype=np.float32)
        of = np.array([(i % (len(fs) + 1)) - 1 for i in range(14)], np.int32)
        radius, _ = _oracle_radii(qs, rows, tomb, "l2")

        def check(tag):
            for gather in (0, ALWAYS):
                eng.set_tuning(WHERE_GATHER=gather)
                lab, cnt, _ = _check_against_singles(eng, qs, radius, _native.MAX_TOPK_PAGED, programs, of, f"{tag}_{gather}")
                for p in range(-1, len(fs)):
                    sel = np.flatnonzero(of == p)
                    m = ~tomb if p < 0 else (_match(fs[p], v) & ~tomb)
                    res = exact_scan.range_query(qs[sel], rows, radius, "l2", deleted=~m)
                    for j, i in enumerate(sel):
                        assert np.array_equal(lab[i], res[j][0]), f"{tag} query {i} program {p}"

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
    radius = 0.85
    got = qp.find_in_radius_many(qs, radius, "ns", where=wheres)
    per = idx.range_search_many(qs, radius, "ns", "cosine", where=wheres)
    assert sum(len(g) for g in got) > 20
    for i, w in enumerate(wheres):
        single = qp.find_in_radius(VectorDTO(values=qs[i].tolist(), metadata={}), radius, "ns", where=w)
        assert [(h["id"], h["score"], h["metadata"]) for h in got[i]] == [(h["id"], h["score"], h["metadata"]) for h in single], i
        assert all(np.array_equal(a["values"], b["values"]) for a, b in zip(got[i], single))
        one = idx.range_search_many(qs[i:i + 1], radius, "ns", "cosine", where=w)[0]
        assert [(h.vector_id, h.score) for h in per[i]] == [(h.vector_id, h.score) for h in one], i
    with pytest.raises(ValueError):
        qp.find_in_radius_many(qs, radius, "ns", where=[lambda m: True] * 20)
    with pytest.raises(ValueError):
        idx.range_search_many(qs, radius, "ns", "cosine", where=wheres[:5])
