"""Grouped kNN on the MI355X (include/mlvdb_grouped.h) through the C ABI: the distinct stage on both of its routes and the
member stage behind it against the NumPy oracle (tests/grouped_helpers.py).  Labels, counts, group counts and groups equal
the oracle exactly; fp64 distances are within SCORE_ATOL of it, fp32 is the rounded fp64, and both are bit-equal to
``pair_distances`` of the returned pairs.  Rows are Gaussian (no fp64 near-ties between different rows); exact duplicates
are copies of rows."""
import functools

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, VectorDTO
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.distinct_helpers import ABSENT
from tests.facet_helpers import colliding_keys, facet_hash
from tests.grouped_helpers import check_grouped, grouped_knn, oracle_index, table_slots, tile_plan
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


def _check(eng, qs, k, g, want, tag, **kw):
    """One call against the oracle's (labels, d64, counts, group counts, groups) for this k and g."""
    return check_grouped(eng, qs, k, g, eng.search_grouped(qs, k, g, 0, want64=True, **kw), want, tag)


def _cut(full, nq, k, g):
    """The oracle's answer for nq queries, k and g out of its answer for 64 x 64."""
    lab, d64, cnt, gcnt, grp = full
    return (lab[:nq, :k, :g], d64[:nq, :k, :g], np.minimum(cnt[:nq], k).astype(np.int32),
            np.minimum(gcnt[:nq, :k], g).astype(np.int32), grp[:nq, :k])


def _oracle(space, qs, rows, groups, allowed, k=64, g=64):
    return grouped_knn(exact_scan.exact_distances(qs, rows, space), groups, allowed, k, g)


# ---------------------------------------------------------------- a. both routes, every size
SIZES = (1, 15, 16, 17, 63, 64, 65, 1000, 40_000)
NQS = (1, 9, 70)
KS = (1, 2, 64)
GS = (1, 2, 63, 64)


@functools.lru_cache(maxsize=None)
def _case_a(space, d):
    """Per size n: (rows, groups, tombstones, the oracle for k = g = 64 over 70 queries) -- computed once, shared by the routes."""
    rng = np.random.default_rng(2000 * d + len(space))
    qs = rng.standard_normal((max(NQS), d), dtype=np.float32)
    out = {}
    for n in SIZES:
        rows = rng.standard_normal((n, d), dtype=np.float32)
        groups = rng.integers(0, max(1, n // 20), n).astype(np.int64)  # ~20 rows per value
        groups[rng.random(n) < 0.15] = ABSENT
        tomb = rng.random(n) < 0.10
        full = _oracle(space, qs, rows, groups, ~tomb)
        for a in full:
            a.setflags(write=False)
        out[n] = rows, groups, tomb, full
    return qs, out


@pytest.mark.parametrize("oversample", ROUTES)
@pytest.mark.parametrize("d", [16, 200])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_both_routes_equal_the_oracle_at_every_size(space, d, oversample):
    qs, cases = _case_a(space, d)
    for n in SIZES:
        rows, groups, tomb, full = cases[n]
        eng = _route(_engine(space, rows, groups, tomb), oversample)
        try:
            for nq in NQS:
                for k in KS:
                    for g in GS:
                        _check(eng, qs[:nq], k, g, _cut(full, nq, k, g), f"a_{space}_{d}_{oversample}_n{n}_q{nq}_k{k}_g{g}")
        finally:
            eng.close()


# ---------------------------------------------------------------- b. group sizes around g, tombstones inside groups
@pytest.mark.parametrize("oversample", ROUTES)
@pytest.mark.parametrize("g", [2, 5, 64])
def test_groups_of_g_minus_one_g_and_g_plus_one_live_rows(g, oversample):
    rng = np.random.default_rng(100 + g)
    d, nq = 24, 9
    sizes = [g - 1, g, g + 1] * 4 + [g + 6, 3]       # live rows per group; the last two lose rows to tombstones below
    groups = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int64)
    n = groups.size
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    dist = exact_scan.exact_distances(qs, rows, "l2")
    tomb = np.zeros(n, bool)
    a = np.flatnonzero(groups == len(sizes) - 2)
    tomb[a[np.argsort(dist[0, a])[:5]]] = True          # the five rows of this group nearest to query 0 are gone
    tomb[groups == len(sizes) - 1] = True               # every row of this group is gone: the group vanishes
    eng = _route(_engine("l2", rows, groups, tomb), oversample)
    try:
        want = grouped_knn(dist, groups, ~tomb, 64, g)
        _, cnt, gcnt, grp = _check(eng, qs, 64, g, want, f"b_{g}_{oversample}")
        assert cnt.tolist() == [len(sizes) - 1] * nq
        assert not (grp == len(sizes) - 1).any()
        for i in range(nq):
            by_group = dict(zip(grp[i, :cnt[i]].tolist(), gcnt[i, :cnt[i]].tolist()))
            assert [by_group[j] for j in range(len(sizes) - 1)] == [min(g, s) for s in sizes[:-2]] + [g]
    finally:
        eng.close()


# ---------------------------------------------------------------- c. lists longer than one chunk
@pytest.mark.parametrize("oversample", ROUTES)
def test_two_values_at_40000_rows_are_split_into_chunks_and_merged(oversample):
    rng = np.random.default_rng(21)
    n, d, nq = 40_000, 32, 9
    rows = rng.standard_normal((n, d), dtype=np.float32)
    groups = rng.integers(0, 2, n).astype(np.int64)
    tomb = rng.random(n) < 0.1
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    dist = exact_scan.exact_distances(qs, rows, "cosine")
    eng = _route(_engine("cosine", rows, groups, tomb), oversample)
    try:
        for k, g in ((2, 64), (1, 7), (2, 1)):
            want = grouped_knn(dist, groups, ~tomb, k, g)
            _, cnt, _, grp = _check(eng, qs, k, g, want, f"c_{oversample}_k{k}_g{g}")
            members = {c: int((~tomb & (groups == c)).sum()) for c in (0, 1)}
            chunk, tiles = tile_plan(grp, cnt, members)
            assert chunk < min(members.values()) and all(nch >= 2 for _, _, nch in tiles), (chunk, tiles)
    finally:
        eng.close()


# ---------------------------------------------------------------- d. exact duplicates
@pytest.mark.parametrize("oversample", ROUTES)
def test_exact_duplicates_resolve_by_label_and_the_fill_order_does_not_leak(oversample):
    rng = np.random.default_rng(22)
    n, d, nq = 3000, 16, 9
    rows = rng.standard_normal((n, d), dtype=np.float32)
    groups = rng.integers(0, 12, n).astype(np.int64)
    src = rng.choice(1000, 40, replace=False)
    rows[1000:1040] = rows[src]                       # copies across groups (their own random group) ...
    rows[2000:2040] = rows[src]
    groups[2000:2040] = groups[src]                   # ... and inside one group
    qs = np.vstack([rows[src[:4]], rng.standard_normal((nq - 4, d), dtype=np.float32)])
    dist = exact_scan.exact_distances(qs, rows, "l2")
    eng = _route(_engine("l2", rows, groups), oversample)
    try:
        want = grouped_knn(dist, groups, np.ones(n, bool), 12, 64)
        lab, _, _, grp = _check(eng, qs, 12, 64, want, f"d_{oversample}")
        for i in range(4):  # the query is a copied row: three rows at one distance, the lowest label first, across and inside groups
            zero = [int(src[i]), 1000 + i, 2000 + i]
            assert lab[i, 0, 0] == min(zero)
            j = grp[i].tolist().index(int(groups[src[i]]))
            same = [r for r in sorted(zero) if groups[r] == groups[src[i]]]
            assert len(same) >= 2 and lab[i, j, :len(same)].tolist() == same
        first = eng.search_grouped(qs, 12, 64, 0, want64=True)
        again = eng.search_grouped(qs, 12, 64, 0, want64=True)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, again))
    finally:
        eng.close()


# ---------------------------------------------------------------- e. equivalences
@pytest.mark.parametrize("oversample", ROUTES)
def test_group_size_one_and_slot_zero_are_search_distinct_bit_for_bit(oversample):
    rng = np.random.default_rng(23)
    n, d, nq = 5000, 48, 20
    rows = rng.standard_normal((n, d), dtype=np.float32)
    groups = rng.integers(0, 300, n).astype(np.int64)
    groups[rng.random(n) < 0.15] = ABSENT
    tomb = rng.random(n) < 0.1
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    for space in ("l2", "cosine", "ip"):
        eng = _route(_engine(space, rows, groups, tomb), oversample)
        try:
            for k in (1, 10, 64):
                dl, dd, dc, d64, dg = eng.search_distinct(qs, k, 0, want64=True)
                for g in (1, 3, 64):
                    lab, dist, cnt, gcnt, g64, grp = eng.search_grouped(qs, k, g, 0, want64=True)
                    assert np.array_equal(lab[:, :, 0], dl) and np.array_equal(cnt, dc) and np.array_equal(grp, dg), (space, k, g)
                    assert np.array_equal(g64[:, :, 0].view(np.int64), d64.view(np.int64))
                    assert np.array_equal(dist[:, :, 0].view(np.int32), dd.view(np.int32))
                    assert np.array_equal(gcnt > 0, dl >= 0)
        finally:
            eng.close()


@pytest.mark.parametrize("oversample", ROUTES)
def test_every_row_its_own_value_is_the_plain_search_in_slot_zero(oversample):
    rng = np.random.default_rng(24)
    n, d = 3000, 64
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows[n // 2] = rows[7]  # an exact duplicate: two groups, one distance
    tomb = rng.random(n) < 0.1
    qs = rng.standard_normal((20, d), dtype=np.float32)
    for space in ("l2", "cosine", "ip"):
        eng = _route(_engine(space, rows, rng.permutation(n) - n // 2, tomb), oversample)
        try:
            for k, g in ((1, 1), (10, 3), (64, 64)):
                lab, dist, cnt, gcnt, d64, _ = eng.search_grouped(qs, k, g, 0, want64=True)
                sl, sd, sc, s64 = eng.search64(qs, k)
                assert np.array_equal(lab[:, :, 0], sl) and np.array_equal(cnt, sc), f"{space} k={k}"
                assert np.array_equal(d64[:, :, 0].view(np.int64), s64.view(np.int64))
                assert np.array_equal(dist[:, :, 0].view(np.int32), sd.view(np.int32))
                assert (gcnt == 1).all() and (lab[:, :, 1:] == -1).all()
        finally:
            eng.close()


# ---------------------------------------------------------------- f. with where
def _flat(lab, gcnt):
    return [[int(x) for j in range(lab.shape[1]) for x in lab[i, j, :gcnt[i, j]]] for i in range(lab.shape[0])]


def test_grouped_under_random_filters_equals_the_oracle_over_the_matching_rows():
    rng = np.random.default_rng(25)
    n, d, nq, k, g = 2000, 16, 9, 10, 4
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
        # {"doc": {"$lt": 75}} keeps whole groups; a filter on another column empties some picked groups' tails
        filters = [random_filter(rng) for _ in range(8)] + [{"genre": "zydeco"}, {}, {"doc": {"$lt": 75}}]
        tails_cut = False
        for oversample in (0, 4):
            idx._ns["ns"].engine.set_tuning(DISTINCT_OVERSAMPLE=oversample)
            for f in filters:
                allowed = live & np.array([py_match(f, m, schema) for m in metas])
                lab, _, cnt, gcnt, grp = grouped_knn(dist, docs, allowed, k, g)
                got = idx.search_many(qs, k, "ns", "cosine", distinct="doc", where=f, group_size=g)
                assert np.array_equal(got.group_sizes, gcnt) and np.array_equal(got.counts, gcnt.sum(axis=1)), (oversample, f)
                for i, flat in enumerate(_flat(lab, gcnt)):
                    assert got.labels[i, :len(flat)].tolist() == flat, (oversample, f, i)
                    assert got.group_values[i, :cnt[i]].tolist() == grp[i, :cnt[i]].tolist()
                full = grouped_knn(dist, docs, live, k, g)[3]
                tails_cut = tails_cut or bool(((gcnt > 0) & (gcnt < g) & (gcnt < full.max())).any())
                if f == {"genre": "zydeco"}:  # matches nothing
                    assert got.counts.tolist() == [0] * nq and (got.labels == -1).all()
        assert tails_cut
    finally:
        idx.close()


# ---------------------------------------------------------------- g. shared and disjoint groups
@pytest.mark.parametrize("oversample", ROUTES)
def test_queries_sharing_groups_fill_tiles_of_every_size_and_disjoint_groups_take_one_each(oversample):
    rng = np.random.default_rng(26)
    d, per = 16, 30
    centres = 8.0 * rng.standard_normal((40, d)).astype(np.float32)
    rows = (centres[:, None, :] + 0.1 * rng.standard_normal((40, per, d)).astype(np.float32)).reshape(-1, d)
    groups = np.repeat(np.arange(40), per).astype(np.int64)
    n = rows.shape[0]
    # 11 queries at centre 0 (tiles of 4, 4, 3), 2 at centre 1, 1 at centre 2, 6 at centre 3 (4, 2), then one per centre 4..39
    at = [0] * 11 + [1] * 2 + [2] + [3] * 6 + list(range(4, 40))
    qs = (centres[at] + 0.05 * rng.standard_normal((len(at), d)).astype(np.float32)).astype(np.float32)
    dist = exact_scan.exact_distances(qs, rows, "l2")
    eng = _route(_engine("l2", rows, groups), oversample)
    try:
        want = grouped_knn(dist, groups, np.ones(n, bool), 1, 5)
        _, cnt, _, grp = _check(eng, qs, 1, 5, want, f"g_{oversample}_k1")
        assert grp[:, 0].tolist() == at
        _, tiles = tile_plan(grp, cnt, {c: per for c in range(40)})
        assert sorted(t[1] for t in tiles if t[0] < 4) == [1, 2, 2, 3, 4, 4, 4] and all(t[1] == 1 for t in tiles if t[0] >= 4)
        want = grouped_knn(dist, groups, np.ones(n, bool), 3, 64)
        _check(eng, qs, 3, 64, want, f"g_{oversample}_k3")
    finally:
        eng.close()


# ---------------------------------------------------------------- h. code values
@pytest.mark.parametrize("oversample", ROUTES)
def test_extreme_negative_and_colliding_codes(oversample):
    rng = np.random.default_rng(27)
    n, d, nq, k = 4000, 16, 9, 8
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    dist = exact_scan.exact_distances(qs, rows, "ip")
    tomb = rng.random(n) < 0.1
    columns = {"extreme": rng.choice(np.array([ABSENT + 1, INT64_MAX, -1, 0, -(1 << 40), ABSENT], np.int64), n)}
    # the column's 8 codes, all negative, are picked by every query and share one probe chain of the table a chunk with 8
    # distinct codes builds (16 slots): every lookup but the first one's walks the chain
    slots = table_slots(k)
    chain = colliding_keys(slots, k, slot=5, start=-10_000)
    assert slots == 16 and (facet_hash(chain) & np.uint64(slots - 1) == np.uint64(5)).all() and (chain < 0).all()
    columns["one_chain"] = chain[rng.integers(0, k, n)]
    for name, groups in columns.items():
        eng = _route(_engine("ip", rows, groups, tomb), oversample)
        try:
            want = grouped_knn(dist, groups, ~tomb, k, 6)
            _, cnt, _, grp = _check(eng, qs, k, 6, want, f"h_{name}_{oversample}")
            if name == "one_chain":
                assert cnt.tolist() == [k] * nq and table_slots(np.unique(grp).size) == slots
        finally:
            eng.close()


# ---------------------------------------------------------------- i. the chunk boundary
def test_1025_queries_cross_the_chunk_boundary():
    rng = np.random.default_rng(28)
    n, d, nq = 1000, 8, 1025
    rows = rng.standard_normal((n, d), dtype=np.float32)
    groups = rng.integers(0, 50, n).astype(np.int64)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    eng = _engine("l2", rows, groups)
    try:
        want = _oracle("l2", qs, rows, groups, np.ones(n, bool), 3, 4)
        _check(eng, qs, 3, 4, want, "i_1025")
    finally:
        eng.close()


# ---------------------------------------------------------------- j. state left behind
def test_other_calls_are_unchanged_after_a_grouped_call_and_the_index_may_grow():
    rng = np.random.default_rng(29)
    n, d, nq = 3000, 32, 9
    rows = rng.standard_normal((n, d), dtype=np.float32)
    groups = rng.integers(0, 100, n).astype(np.int64)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    idx = Index(space="l2", attributes={"doc": "int"})
    try:
        idx.add_arrays(rows, "ns", attributes={"doc": groups.tolist()})
        eng = idx._ns["ns"].engine
        where = {"doc": {"$lt": 40}}

        def others():
            return (eng.search64(qs, 10), eng.search_distinct(qs, 10, 0, want64=True),
                    (idx.search_many(qs, 10, "ns", "l2", where=where).labels,))

        before = others()
        want = _oracle("l2", qs, rows, groups, np.ones(n, bool), 10, 3)
        _check(eng, qs, 10, 3, want, "j_first")
        got = idx.search_many(qs, 10, "ns", "l2", distinct="doc", where=where, group_size=3)
        assert (got.counts > 0).all()
        after = others()
        for a, b in zip(before, after):
            assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
        # grow (the columns and the workspaces follow), tombstone, call again
        more = rng.standard_normal((5000, d), dtype=np.float32)
        more_g = rng.integers(50, 160, 5000).astype(np.int64)
        first = eng.append(more)
        eng.set_attr(0, first, more_g)
        rows2, groups2 = np.vstack([rows, more]), np.concatenate([groups, more_g])
        tomb = rng.random(rows2.shape[0]) < 0.2
        eng.tombstone(np.flatnonzero(tomb))
        want = _oracle("l2", qs, rows2, groups2, ~tomb, 10, 3)
        _check(eng, qs, 10, 3, want, "j_grown")
    finally:
        idx.close()


# ---------------------------------------------------------------- k. the C ABI's refusals
def test_the_entry_validates_before_anything_is_launched():
    eng = HipScanEngine(8, "l2", device=0)
    try:
        eng.append(np.ones((4, 8), np.float32))
        eng.define_attr(0, "int64")
        eng.define_attr(1, "float64")
        eng.set_attr(0, 0, np.arange(4, dtype=np.int64))
        qs = np.zeros((1, 8), np.float32)
        eng.last_stats()
        with pytest.raises(RuntimeError, match=r"failed \(6\).*MLVDB_MAX_TOPK"):
            eng.search_grouped(qs, 65, 2, 0)
        with pytest.raises(RuntimeError, match=r"failed \(6\).*MLVDB_GROUPED_MAX_SIZE"):
            eng.search_grouped(qs, 3, 65, 0)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*group_size"):
            eng.search_grouped(qs, 3, 0, 0)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*int64 column"):
            eng.search_grouped(qs, 3, 2, 1)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*not defined"):
            eng.search_grouped(qs, 3, 2, 2)
        buf = np.zeros(64, np.int64)
        for null in range(4):  # labels, dist, counts, group counts
            outs = [buf.ctypes.data] * 4
            outs[null] = None
            rc = eng._lib.mlvdb_search_batch_grouped(eng._h, qs.ctypes.data, 1, 2, 2, 0, 0, None, *outs, None, None)
            assert rc == 1 and b"null buffer" in eng._lib.mlvdb_last_error(eng._h)
        assert eng._lib.mlvdb_search_batch_grouped(eng._h, None, 1, 2, 2, 0, 0, None, *[buf.ctypes.data] * 4, None, None) == 1
        assert eng._lib.mlvdb_search_batch_grouped(eng._h, qs.ctypes.data, -1, 2, 2, 0, 0, None, *[buf.ctypes.data] * 4, None, None) == 1
        stats = eng.last_stats()
        assert stats["scan_launches"] == 0 and stats["rows_scanned"] == 0 and stats["fallback_queries"] == 0
        lab, _, cnt, gcnt, grp = eng.search_grouped(qs, 3, 2, 0)
        assert cnt.tolist() == [3] and gcnt.tolist() == [[1, 1, 1]] and lab[0, :, 0].tolist() == [0, 1, 2]
        # a fully tombstoned index answers padding
        eng.tombstone(np.arange(4))
        eng.last_stats()
        lab, dist, cnt, gcnt, grp = eng.search_grouped(qs, 3, 2, 0)
        assert cnt.tolist() == [0] and (lab == -1).all() and np.isinf(dist).all() and (gcnt == 0).all() and (grp == ABSENT).all()
        assert eng.last_stats()["scan_launches"] == 0
    finally:
        eng.close()


def test_an_empty_index_answers_padding():
    eng = HipScanEngine(8, "cosine", device=0)
    try:
        eng.define_attr(0, "int64")
        lab, dist, cnt, gcnt, d64, grp = eng.search_grouped(np.ones((2, 8), np.float32), 4, 3, 0, want64=True)
        assert lab.shape == (2, 4, 3) and (lab == -1).all() and np.isinf(dist).all() and np.isinf(d64).all()
        assert cnt.tolist() == [0, 0] and (gcnt == 0).all() and (grp == ABSENT).all()
    finally:
        eng.close()


# ---------------------------------------------------------------- l. through Index and QueryProcessor
def test_index_and_query_processor_on_the_gpu_equal_the_oracle_engine_index():
    rng = np.random.default_rng(30)
    d, n = 32, 900
    vecs = [VectorDTO(values=rng.standard_normal(d).tolist(), metadata={"doc": int(i % 31), "chunk": i}) for i in range(n)]
    qs = rng.standard_normal((5, d)).astype(np.float32)
    gpu, ref = Index(space="cosine", attributes={"doc": "int"}), oracle_index({"doc": "int"}, space="cosine")
    qp, qp_ref = QueryProcessor(InMemoryStorage(), gpu), QueryProcessor(InMemoryStorage(), ref)
    try:
        qp.upsert_many(vecs, "ns")
        qp_ref.upsert_many(vecs, "ns")
        a = gpu.search_many(qs, 8, "ns", "cosine", distinct="doc", group_size=3)
        b = ref.search_many(qs, 8, "ns", "cosine", distinct="doc", group_size=3)
        assert np.array_equal(a.labels, b.labels) and np.array_equal(a.counts, b.counts)
        assert np.array_equal(a.group_sizes, b.group_sizes) and a.group_values.tolist() == b.group_values.tolist()
        assert a.counts.tolist() == [24] * 5 and np.abs(a.scores[a.valid()] - b.scores[b.valid()]).max() <= SCORE_ATOL
        out, out_ref = (p.find_similar_many(qs, 8, "ns", distinct="doc", group_size=3) for p in (qp, qp_ref))
        for hits, want, row in zip(out, out_ref, a):
            assert [h["metadata"]["chunk"] for h in hits] == [h["metadata"]["chunk"] for h in want]
            assert [h["id"] for h in hits] == [r.vector_id for r in row] and len(hits) == 24
            docs = [h["metadata"]["doc"] for h in hits]
            assert docs[::3] == docs[1::3] == docs[2::3] and len(set(docs)) == 8
    finally:
        gpu.close()
