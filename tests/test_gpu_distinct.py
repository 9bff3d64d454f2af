"""Distinct-by-attribute kNN on the MI355X (include/mlvdb_distinct.h): both routes -- the pick over the plain search's ranked
list and the grouped exact scan -- against the NumPy oracle (tests/distinct_helpers.py).  Ids, counts and groups equal the
oracle exactly; distances are within SCORE_ATOL of it and bit-equal to ``pair_distances`` of the returned pairs.
Rows are Gaussian (no fp64 near-ties between different rows); exact duplicates are copies of rows."""
import functools
from uuid import UUID

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, VectorDTO
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.conftest import dump_mismatch
from tests.distinct_helpers import ABSENT, distinct_knn, group_spans_blocks_and_waves, scan_geometry
from tests.helpers import SCORE_ATOL
from tests.where_helpers import SCHEMA, py_match, random_filter, random_metadata

pytestmark = pytest.mark.gpu

ROUTES = [0, None]  # DISTINCT_OVERSAMPLE: 0 = every query takes the grouped scan, None = the default (list pass first)
INT64_MAX = np.iinfo(np.int64).max


def _engine(space, rows, groups, tomb=None):
    eng = HipScanEngine(rows.shape[1], space, device=0)
    eng.append(rows)
    eng.define_attr(0, "int64")
    eng.set_attr(0, 0, np.ascontiguousarray(groups, dtype=np.int64))
    if tomb is not None and tomb.any():
        eng.tombstone(np.flatnonzero(tomb))
    return eng


def _route(eng, oversample):
    if oversample is not None:
        eng.set_tuning(DISTINCT_OVERSAMPLE=oversample)
    else:
        assert eng.get_tuning("DISTINCT_OVERSAMPLE") == 4
    return eng


def _check(eng, qs, k, want, tag, **kw):
    """One call against the oracle's (labels, d64, counts, groups) for this k."""
    lab, dist, cnt, d64, grp = eng.search_distinct(qs, k, 0, want64=True, **kw)
    wl, wd, wc, wg = want
    ok = np.array_equal(lab, wl) and np.array_equal(cnt, wc) and np.array_equal(grp, wg)
    if not ok:
        dump_mismatch(f"distinct_{tag}", lab=lab, wl=wl, cnt=cnt, wc=wc, grp=grp, wg=wg, d64=d64, wd=wd)
        bad = np.flatnonzero((lab != wl).any(axis=1) | (cnt != wc) | (grp != wg).any(axis=1))
        raise AssertionError(f"{tag}: {bad.size} queries differ, first {bad[0]}: got {lab[bad[0]]} ({cnt[bad[0]]}) "
                             f"want {wl[bad[0]]} ({wc[bad[0]]})")
    fin = np.isfinite(wd)
    assert np.array_equal(np.isfinite(d64), fin) and np.array_equal(np.isfinite(dist), fin), f"{tag}: padding differs"
    if fin.any():
        err = float(np.abs(d64[fin] - wd[fin]).max())
        print(f"{tag}: max |d64 - oracle| = {err:.3e}")
        assert err <= SCORE_ATOL, f"{tag}: distance error {err}"
    # the fp32 output is the fp64 distance rounded once: an absolute 1e-5 cannot be asked of fp32 itself beyond 128, where
    # half an ulp is 7.6e-6 and more (l2 at d = 200 gives ~330), so it is held to the exact rounding instead
    assert np.array_equal(dist.view(np.int32), d64.astype(np.float32).view(np.int32)), f"{tag}: fp32 is not the rounded fp64"
    p64, p32 = eng.pair_distances(qs, lab)
    assert np.array_equal(p64.view(np.int64), d64.view(np.int64)), f"{tag}: fp64 differs from pair_distances"
    assert np.array_equal(p32.view(np.int32), dist.view(np.int32)), f"{tag}: fp32 differs from pair_distances"
    return lab, cnt


def _cut(full, k):
    """The oracle's answer for k out of its answer for 64."""
    lab, d64, cnt, grp = full
    return lab[:, :k], d64[:, :k], np.minimum(cnt, k).astype(np.int32), grp[:, :k]


# ---------------------------------------------------------------- a. both routes, every size
SIZES = (1, 15, 16, 17, 63, 64, 65, 1000, 40_000)
NQS = (1, 9, 70)
KS = (1, 2, 63, 64)


@functools.lru_cache(maxsize=None)
def _case_a(space, d):
    """Per size n: (rows, groups, tombstones, the oracle for k = 64 over 70 queries) -- computed once, shared by the routes."""
    rng = np.random.default_rng(1000 * d + len(space))
    qs = rng.standard_normal((max(NQS), d), dtype=np.float32)
    out = {}
    for n in SIZES:
        rows = rng.standard_normal((n, d), dtype=np.float32)
        groups = rng.integers(0, max(1, n // 20), n).astype(np.int64)  # ~20 rows per value
        groups[rng.random(n) < 0.15] = ABSENT
        tomb = rng.random(n) < 0.10
        full = distinct_knn(exact_scan.exact_distances(qs, rows, space), groups, ~tomb, 64)
        for a in full:
            a.setflags(write=False)
        out[n] = rows, groups, tomb, full
    # 40,000 rows span many blocks of the grouped scan: some group has live rows in two blocks, and in two waves of a block
    rows, groups, tomb, _ = out[40_000]
    for nq in NQS:
        assert group_spans_blocks_and_waves(groups, ~tomb, scan_geometry(40_000, d, nq)), (d, nq)
    return qs, out


@pytest.mark.parametrize("oversample", ROUTES)
@pytest.mark.parametrize("d", [3, 64, 200])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_both_routes_equal_the_oracle_at_every_size(space, d, oversample):
    qs, cases = _case_a(space, d)
    for n in SIZES:
        rows, groups, tomb, full = cases[n]
        eng = _route(_engine(space, rows, groups, tomb), oversample)
        try:
            for nq in NQS:
                want = tuple(a[:nq] for a in full)
                for k in KS:
                    _check(eng, qs[:nq], k, _cut(want, k), f"a_{space}_{d}_{oversample}_n{n}_q{nq}_k{k}")
        finally:
            eng.close()


# ---------------------------------------------------------------- a2. the tail of the grouped scan's walk
# distinct_scan_kernel walks the rows as the exact scan does (plan_exact's tiles): totals at and around one wave step and one
# block step of every tile (16 x PW x NW = 512 rows for 1, 2 and 4 queries, 256 for 8), as tests/test_gpu_knn_limits.py has them.
TAIL_COUNTS = [1, 15, 17, 255, 257, 511, 513]


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
@pytest.mark.parametrize("n", TAIL_COUNTS)
def test_grouped_scan_tail_with_the_last_row_tombstoned(n, space):
    """The list pass off: every query takes the grouped scan.  The last row is a copy of query 0 in a group of its own and
    tombstoned (where there is more than one row); batches of 1, 2, 3, 4 and 8 queries.  No two live fp64 distances of a
    query lie within 1e-9 (relative) of each other."""
    d, k = 20, 3
    rng = np.random.default_rng(9900 + n)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((8, d), dtype=np.float32)
    groups = (np.arange(n) % 7).astype(np.int64)
    tomb = np.zeros(n, dtype=bool)
    if n > 1:
        rows[n - 1], groups[n - 1], tomb[n - 1] = qs[0], 1000, True
    dm = exact_scan.exact_distances(qs, rows, space)
    srt = np.sort(dm[:, ~tomb], axis=1)
    assert (np.diff(srt, axis=1) > 1e-9 * np.abs(srt[:, 1:])).all(), "precondition: an accidental near-tie -- choose another seed"
    assert n == 1 or (dm[0, n - 1] < srt[0, 0]), "precondition: the tombstoned row would lead query 0"
    full = distinct_knn(dm, groups, ~tomb, k)
    assert n == 1 or not (full[3] == 1000).any(), "precondition: the oracle leaves the tombstoned row's group out"
    eng = _route(_engine(space, rows, groups, tomb), 0)
    try:
        for nq in (1, 2, 3, 4, 8):
            _check(eng, qs[:nq], k, tuple(a[:nq] for a in full), f"tail_{space}_n{n}_q{nq}")
    finally:
        eng.close()


# ---------------------------------------------------------------- b. shapes of the group column
@pytest.mark.parametrize("oversample", ROUTES)
@pytest.mark.parametrize("n", [3000, 40_000])
def test_every_row_its_own_value_is_the_plain_search_bit_for_bit(n, oversample):
    rng = np.random.default_rng(n)
    d = 64
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows[n // 2] = rows[7]  # an exact duplicate: two groups, one distance
    tomb = rng.random(n) < 0.1
    qs = rng.standard_normal((20, d), dtype=np.float32)
    for space in ("l2", "cosine", "ip"):
        eng = _route(_engine(space, rows, rng.permutation(n) - n // 2, tomb), oversample)
        try:
            for k in (1, 10, 64):
                lab, dist, cnt, d64, grp = eng.search_distinct(qs, k, 0, want64=True)
                sl, sd, sc, s64 = eng.search64(qs, k)
                assert np.array_equal(lab, sl) and np.array_equal(cnt, sc), f"{space} k={k}"
                assert np.array_equal(d64.view(np.int64), s64.view(np.int64)) and np.array_equal(dist.view(np.int32), sd.view(np.int32))
        finally:
            eng.close()


def _column_shapes(rng, n):
    sizes = rng.integers(1, 501, 64)
    drawn = np.repeat(np.arange(sizes.size), sizes)[:n]
    drawn = np.concatenate([drawn, np.full(n - drawn.size, 999)])
    return {
        "one_value": np.full(n, 42, np.int64),
        "all_absent": np.full(n, ABSENT, np.int64),
        "five_groups": rng.integers(0, 5, n).astype(np.int64),
        "extreme_values": rng.choice(np.array([ABSENT + 1, INT64_MAX, -1, 0, ABSENT], np.int64), n),
        "sizes_1_to_500": rng.permutation(drawn).astype(np.int64),
    }


@pytest.mark.parametrize("oversample", ROUTES)
@pytest.mark.parametrize("shape", ["one_value", "all_absent", "five_groups", "extreme_values", "sizes_1_to_500"])
def test_shapes_of_the_group_column(shape, oversample):
    rng = np.random.default_rng(17)
    n, d, nq = 5000, 24, 9
    rows = rng.standard_normal((n, d), dtype=np.float32)
    tomb = rng.random(n) < 0.1
    groups = _column_shapes(rng, n)[shape]
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    eng = _route(_engine("cosine", rows, groups, tomb), oversample)
    try:
        dist = exact_scan.exact_distances(qs, rows, "cosine")
        for k in (1, 10, 64):
            want = distinct_knn(dist, groups, ~tomb, k)
            _, cnt = _check(eng, qs, k, want, f"b_{shape}_{oversample}_k{k}")
            expect = {"one_value": 1, "all_absent": 0, "five_groups": min(k, 5), "extreme_values": min(k, 4)}.get(shape)
            if expect is not None:
                assert cnt.tolist() == [expect] * nq
    finally:
        eng.close()


# ---------------------------------------------------------------- c. replacement inside the list
@pytest.mark.parametrize("oversample", ROUTES)
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_later_rows_of_a_group_replace_the_listed_one_in_place(space, oversample):
    # unit rows at a decreasing angle to query 0, row i in group i mod G: within each group every later row is nearer to
    # query 0 (in all three spaces) and must take the place of the listed one
    rng = np.random.default_rng(5)
    d, G, R = 16, 100, 12
    n = G * R
    q0 = rng.standard_normal(d)
    q0 /= np.linalg.norm(q0)
    perp = rng.standard_normal((n, d))
    perp -= (perp @ q0)[:, None] * q0
    perp /= np.linalg.norm(perp, axis=1)[:, None]
    theta = np.linspace(1.5, 0.05, n)
    rows = (np.cos(theta)[:, None] * q0 + np.sin(theta)[:, None] * perp).astype(np.float32)
    groups = (np.arange(n) % G).astype(np.int64)
    # exact duplicates: the best row of group G-2 is a copy of group G-1's, the nearest of all (different groups, the tie
    # goes to the lower label), and every group's best row is appended once more to its own group (same group, the lower
    # label represents it)
    rows[n - 2] = rows[n - 1]
    rows = np.vstack([rows, rows[n - G:]])
    groups = np.concatenate([groups, groups[n - G:]])
    qs = np.vstack([q0[None, :].astype(np.float32), rng.standard_normal((8, d), dtype=np.float32)])
    dist = exact_scan.exact_distances(qs, rows, space)
    assert (np.diff(dist[0, :n - 1]) < 0).all() and dist[0, n - 2] == dist[0, n - 1]
    eng = _route(_engine(space, rows, groups), oversample)
    try:
        for k in (1, 5, 64):
            want = distinct_knn(dist, groups, np.ones(rows.shape[0], bool), k)
            lab, _ = _check(eng, qs, k, want, f"c_{space}_{oversample}_k{k}")
            assert lab[0, :2].tolist() == [n - 2, n - 1][:k]  # between groups: the lower label first
            assert (lab[0, :k] < n).all()                         # within a group: never the appended copy
    finally:
        eng.close()


# ---------------------------------------------------------------- d. the list pass cannot finish
@pytest.mark.parametrize("space", ["l2", "cosine"])
def test_queries_the_list_cannot_finish_take_the_grouped_scan_and_are_counted(space):
    rng = np.random.default_rng(11)
    d, k = 16, 10
    a = np.zeros(d, np.float32)
    a[0] = 20.0
    cluster = a + 0.01 * rng.standard_normal((2000, d), dtype=np.float32)  # the 2,000 nearest rows of a query near `a`
    others = rng.standard_normal((4000, d), dtype=np.float32)
    others[:, 0] = -np.abs(others[:, 0])                                    # ... the rest lie on the other side
    rows = np.vstack([cluster, others])
    groups = np.concatenate([np.full(2000, 7), 100 + rng.integers(0, 200, 4000)]).astype(np.int64)
    near = a + 0.01 * rng.standard_normal((5, d), dtype=np.float32)
    far = rng.standard_normal((4, d), dtype=np.float32)
    far[:, 0] = -np.abs(far[:, 0])
    qs = np.vstack([near[:2], far[:2], near[2:], far[2:]])
    is_near = np.array([1, 1, 0, 0, 1, 1, 1, 0, 0], bool)
    dist = exact_scan.exact_distances(qs, rows, space)
    order = np.argsort(dist, axis=1)
    assert (order[is_near, :2000] < 2000).all()  # L <= 1024 sees one group
    assert all(np.unique(groups[order[i, :64]]).size >= k for i in np.flatnonzero(~is_near))
    eng = _engine(space, rows, groups)
    try:
        assert eng.get_tuning("DISTINCT_OVERSAMPLE") == 4
        eng.last_stats()
        want = distinct_knn(dist, groups, np.ones(6000, bool), k)
        _check(eng, qs, k, want, f"d_{space}")
        eng.last_stats()
        eng.search_distinct(qs, k, 0)
        assert eng.last_stats()["fallback_queries"] == int(is_near.sum())
    finally:
        eng.close()


def test_a_list_longer_than_the_live_rows_completes_without_fallback():
    rng = np.random.default_rng(12)
    n, d = 40, 8
    rows = rng.standard_normal((n, d), dtype=np.float32)
    groups = rng.integers(0, 4, n).astype(np.int64)
    qs = rng.standard_normal((6, d), dtype=np.float32)
    eng = _engine("l2", rows, groups)
    try:
        eng.last_stats()
        want = distinct_knn(exact_scan.exact_distances(qs, rows, "l2"), groups, np.ones(n, bool), 10)
        lab, dist, cnt, grp = eng.search_distinct(qs, 10, 0)
        assert eng.last_stats()["fallback_queries"] == 0
        assert np.array_equal(lab, want[0]) and cnt.tolist() == [4] * 6 and np.array_equal(grp, want[3])
    finally:
        eng.close()


# ---------------------------------------------------------------- e. max_groups
def test_a_str_column_bounds_the_groups_by_its_dictionary():
    rng = np.random.default_rng(13)
    n, d, nq = 1200, 32, 7
    genres = ["jazz", "blues", "rock", "pop", "folk", "metal"]
    rows = rng.standard_normal((n, d), dtype=np.float32)
    genre = rng.integers(0, 6, n)
    idx = Index(space="l2", attributes={"genre": "str"})
    try:
        ids = idx.add_arrays(rows, "ns", attributes={"genre": [genres[g] for g in genre]})
        eng = idx._ns["ns"].engine
        codes = eng.get_attr(0, 0, n)
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        dist = exact_scan.exact_distances(qs, rows, "l2")
        eng.last_stats()
        got = idx.search_many(qs, 10, "ns", "l2", distinct="genre")
        assert eng.last_stats()["fallback_queries"] == 0
        want = distinct_knn(dist, codes, np.ones(n, bool), 10)
        assert got.counts.tolist() == [6] * nq and np.array_equal(got.labels, want[0])
        # every row of one value gone: five groups, still the oracle's (the queries may take the grouped scan)
        gone = np.flatnonzero(genre == 2)
        idx.remove([UUID(bytes=ids[i].tobytes()) for i in gone], "ns")
        got = idx.search_many(qs, 10, "ns", "l2", distinct="genre")
        want = distinct_knn(dist, codes, genre != 2, 10)
        assert got.counts.tolist() == [5] * nq and np.array_equal(got.labels, want[0])
    finally:
        idx.close()


# ---------------------------------------------------------------- f. with where
def test_distinct_under_random_filters_equals_the_oracle_over_the_matching_rows():
    rng = np.random.default_rng(14)
    n, d, nq, k = 2000, 16, 9, 10
    schema = dict(SCHEMA, doc="int")
    metas = random_metadata(rng, n)
    doc = rng.integers(0, 150, n).astype(np.int64)
    for m, v in zip(metas, doc.tolist()):
        if rng.random() < 0.85:
            m["doc"] = v
    docs = np.array([m.get("doc", ABSENT) if m.get("doc") is not None else ABSENT for m in metas], np.int64)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    idx = Index(space="cosine", attributes=schema)
    try:
        idx.add_arrays(rows, "ns", attributes=idx.extract_attributes(metas))
        gone = rng.choice(n, n // 10, replace=False)
        idx._ns["ns"].engine.tombstone(gone)
        live = np.ones(n, bool)
        live[gone] = False
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        dist = exact_scan.exact_distances(qs, rows, "cosine")
        filters = [random_filter(rng) for _ in range(10)] + [{"genre": "zydeco"}, {}]
        for oversample in (0, 4):
            idx._ns["ns"].engine.set_tuning(DISTINCT_OVERSAMPLE=oversample)
            for f in filters:
                allowed = live & np.array([py_match(f, m) for m in metas])
                want = distinct_knn(dist, docs, allowed, k)
                got = idx.search_many(qs, k, "ns", "cosine", distinct="doc", where=f)
                assert np.array_equal(got.labels, want[0]) and np.array_equal(got.counts, want[2]), (oversample, f)
                if f == {"genre": "zydeco"}:  # matches nothing
                    assert got.counts.tolist() == [0] * nq and (got.labels == -1).all()
    finally:
        idx.close()


# ---------------------------------------------------------------- g. columns follow the rows
@pytest.mark.parametrize("oversample", ROUTES)
def test_groups_follow_appends_tombstones_and_compaction(oversample):
    rng = np.random.default_rng(15)
    d, k = 48, 12
    rows = rng.standard_normal((3000, d), dtype=np.float32)
    groups = rng.integers(0, 300, 3000).astype(np.int64)
    groups[rng.random(3000) < 0.15] = ABSENT
    qs = rng.standard_normal((9, d), dtype=np.float32)
    eng = _route(_engine("l2", rows, groups), oversample)
    try:
        gone = rng.choice(3000, 700, replace=False)
        eng.tombstone(gone)
        old = eng.compact()
        rows, groups = rows[old], groups[old]
        assert np.array_equal(eng.get_attr(0, 0, old.size), groups)
        more = rng.standard_normal((500, d), dtype=np.float32)
        more_g = rng.integers(250, 400, 500).astype(np.int64)
        first = eng.append(more)
        eng.set_attr(0, first, more_g)
        rows, groups = np.vstack([rows, more]), np.concatenate([groups, more_g])
        want = distinct_knn(exact_scan.exact_distances(qs, rows, "l2"), groups, np.ones(rows.shape[0], bool), k)
        _check(eng, qs, k, want, f"g_{oversample}")
    finally:
        eng.close()


# ---------------------------------------------------------------- h. protocol level
def test_query_processor_returns_one_dict_per_group():
    rng = np.random.default_rng(16)
    d, n = 32, 900
    idx = Index(space="cosine", attributes={"doc": "int"})
    qp = QueryProcessor(InMemoryStorage(), idx)
    try:
        qp.upsert_many([VectorDTO(values=rng.standard_normal(d).tolist(), metadata={"doc": int(i % 31), "chunk": i})
                        for i in range(n)], "ns")
        qs = rng.standard_normal((5, d)).astype(np.float32)
        out = qp.find_similar_many(qs, 8, "ns", distinct="doc")
        bh = idx.search_many(qs, 8, "ns", "cosine", distinct="doc")
        assert len(out) == 5
        for i, hits in enumerate(out):
            docs = [h["metadata"]["doc"] for h in hits]
            assert len(hits) == 8 == len(set(docs))
            assert [h["id"] for h in hits] == [r.vector_id for r in bh[i]]
    finally:
        idx.close()


# ---------------------------------------------------------------- the C ABI's refusals
def test_the_entry_refuses_a_float_column_and_k_above_64():
    eng = HipScanEngine(8, "l2", device=0)
    try:
        eng.append(np.zeros((4, 8), np.float32))
        eng.define_attr(0, "int64")
        eng.define_attr(1, "float64")
        qs = np.zeros((1, 8), np.float32)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*int64 column"):
            eng.search_distinct(qs, 3, 1)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*not defined"):
            eng.search_distinct(qs, 3, 2)
        with pytest.raises(RuntimeError, match=r"MLVDB_MAX_TOPK"):
            eng.search_distinct(qs, 65, 0)
        lab, _, cnt, _ = eng.search_distinct(qs, 3, 0)  # every value absent
        assert cnt.tolist() == [0] and (lab == -1).all()
    finally:
        eng.close()
