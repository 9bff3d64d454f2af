"""Clustering on the MI355X (include/mlvdb_cluster.h), at the engine level through the C ABI.
1. Assignment replay: the rule of tests/cluster_helpers.py run on the device's own bits -- ``pair_distances(centroid, every
   label)`` for every d_j(x) -- must reproduce the column, the sizes, the candidates and, bit for bit, the costs.  No tolerance.
2. Means replay: one k-means iteration against the blocked order in NumPy on the fetched rows, bit for bit.
3. Whole runs: the model's loop driven by the device's own distances.
4. Against the NumPy fp64 oracle: blobs, and Gaussian rows under an asserted gap precondition.
5. Structure: filters, no column, more centroids than candidates, empty cases, mutations, the C-level refusals."""
import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.cluster_helpers import (NO_CANDIDATE, centroid_vectors, model_assign, model_kmeans, model_means,
                                   model_sizes_costs)
from tests.scored_helpers import GAP_MIN

pytestmark = pytest.mark.gpu

TRUE = W.Program(np.array([(W.TRUE, 0, 0, 0)], dtype=W.OP_DTYPE), np.zeros(0, np.int64))
COL, TAG = 0, 1  # the cluster column, a second int64 column the filters read
ABSENT = W.INT64_ABSENT
KEPT = 77  # what the cluster column holds before a call: a row the call must not touch still holds it afterwards


def W1(op, attr, a=0, b=0, table=()):
    return W.Program(np.array([(op, attr, a, b)], dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(got.shape[0], -1).any(axis=1)) if got.size else []
    assert len(bad) == 0, f"{what}: differs in {len(bad)} entries, first {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def _mask(labels, n):
    m = np.zeros(n, bool)
    m[labels] = True
    return m


def _corpus(space, n, d, seed, tomb=0.0, rows=None):
    rng = np.random.default_rng(seed)
    eng = HipScanEngine(d, space, device=0)
    rows = rng.standard_normal((n, d), dtype=np.float32) if rows is None else rows
    eng.append(rows)
    if tomb:
        eng.tombstone(np.flatnonzero(rng.random(n) < tomb))
    eng.define_attr(COL, "int64")
    eng.define_attr(TAG, "int64")
    eng.set_attr(COL, 0, np.full(n, KEPT, np.int64))
    eng.set_attr(TAG, 0, np.arange(n, dtype=np.int64) % 5)
    return eng, rows, rng


def _live(eng, where=TRUE):
    return _mask(eng.where_labels(where), eng.counts()[0])


def _distances(eng, c):
    n = eng.counts()[0]
    return eng.pair_distances(c, np.broadcast_to(np.arange(n), (c.shape[0], n)))[0]


def _random_centroids(rng, m, n, d, dead):
    """Stored and raw centroids mixed, labels repeated (duplicate centroids), the last one a tombstoned label."""
    lab = rng.choice(n, m).astype(np.int64)
    for j in range(1, m):
        if rng.random() < 0.2:
            lab[j] = lab[int(rng.integers(j))]
    lab[rng.random(m) < 0.3] = -1
    if m >= 4:  # whatever the draw: a stored centroid, a raw one, a duplicate of the stored one
        lab[0], lab[1] = int(rng.integers(n)), -1
        lab[2] = lab[0]
    if m >= 2 and dead.any():
        lab[-1] = np.flatnonzero(dead)[0]
    return lab, rng.standard_normal((m, d)).astype(np.float32)


def _column_want(assign, before):
    return np.where(assign == NO_CANDIDATE, before, np.where(assign >= 0, assign, ABSENT))


def _replay_assign(eng, rows, lab, vec, tag, where=None, attr=COL):
    """One ``assign_nearest`` against the model on the device's own distances; returns the model's assignment."""
    n = eng.counts()[0]
    c = centroid_vectors(rows, lab, vec)
    live = _live(eng, TRUE if where is None else where)
    assign, best = model_assign(_distances(eng, c), live)
    before = eng.get_attr(COL, 0, n)
    sizes, costs, matched = eng.assign_nearest(lab, vec, where=where, assign_attr=attr)
    want_sizes, want_costs = model_sizes_costs(assign, best, c.shape[0])
    assert matched == int(live.sum()), tag
    assert np.array_equal(sizes, want_sizes), f"{tag}: sizes {sizes} want {want_sizes}"
    assert int(sizes.sum()) + int((assign == -1).sum()) == matched, tag
    _same_bits(costs, want_costs, f"{tag}: costs")
    want_col = _column_want(assign, before) if attr >= 0 else before
    col = eng.get_attr(COL, 0, n)
    bad = np.flatnonzero(col != want_col)
    assert bad.size == 0, f"{tag}: column differs in {bad.size} rows, first {bad[0]}: got {col[bad[0]]} want {want_col[bad[0]]}"
    return assign


# ---------------------------------------------------------------- 1. assignment replay
SHAPES = ((1, 16), (15, 16), (16, 16), (17, 16), (5000, 16), (300, 768), (700, 300), (40, 4112))
MS = (1, 8, 9, 16, 17, 64, 65)


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_assign_nearest_equals_the_rule_replayed_on_the_devices_own_bits(space, n, d):
    eng, rows, rng = _corpus(space, n, d, 13 * n + d + len(space), tomb=1 / 3 if n >= 15 else 0.0)
    try:
        dead = ~_live(eng)
        assert n < 15 or (dead.any() and not dead.all())
        for m in MS:
            lab, vec = _random_centroids(rng, m, n, d, dead)
            if m >= 8:
                assert (lab == -1).any() and (lab >= 0).any(), "stored and raw centroids are not mixed"
                assert n < 15 or dead[lab[-1]], "no tombstoned centroid"
            assign = _replay_assign(eng, rows, lab, vec, f"{space} {n}x{d} m={m}")
            stored = lab[lab >= 0]
            if m >= 8:
                assert np.unique(stored).size < stored.size, "no duplicate centroid"
            for j in range(m):  # a duplicate of an earlier centroid never wins a row
                if lab[j] >= 0 and (lab[:j] == lab[j]).any():
                    assert not (assign == j).any()
            eng.set_attr(COL, 0, np.full(n, KEPT, np.int64))
    finally:
        eng.close()


def test_assign_nearest_with_the_most_centroids():
    n, d, m = 2000, 16, _native.CLUSTER_MAX
    eng, rows, rng = _corpus("cosine", n, d, 5, tomb=1 / 3)
    try:
        lab, vec = _random_centroids(rng, m, n, d, ~_live(eng))
        _replay_assign(eng, rows, lab, vec, "m=1024")
    finally:
        eng.close()


# ---------------------------------------------------------------- 2. means replay
def _replay_one_iteration(eng, rows, lab, vec, space, tag):
    n = eng.counts()[0]
    c0 = centroid_vectors(rows, lab, vec)
    assign, best = model_assign(_distances(eng, c0), _live(eng))
    fetched = eng.get_rows(0, n)
    assert np.array_equal(fetched.view(np.int32), rows.view(np.int32))
    want = model_means(fetched, assign, c0.shape[0], space, c0)
    want_sizes, want_costs = model_sizes_costs(assign, best, c0.shape[0])
    cent, sizes, costs, iterations, converged, matched = eng.kmeans(lab, vec, max_iterations=1, assign_attr=COL)
    assert iterations == 1 and not converged and matched == int(_live(eng).sum()), tag
    assert np.array_equal(sizes, want_sizes), tag
    _same_bits(cent, want, f"{tag}: centroids")
    _same_bits(costs, want_costs, f"{tag}: costs")
    for j in np.flatnonzero(sizes == 0):  # an empty cluster keeps its centroid
        _same_bits(cent[j], c0[j], f"{tag}: empty cluster {j}")
    return sizes


@pytest.mark.parametrize("space", ["l2", "cosine"])
@pytest.mark.parametrize("live", [255, 256, 257, 513])
def test_one_cluster_at_the_segment_edges(space, live):
    n, d = live + 40, 16
    eng, rows, rng = _corpus(space, n, d, live)
    try:
        eng.tombstone(rng.choice(n, 40, replace=False))
        assert int(_live(eng).sum()) == live
        sizes = _replay_one_iteration(eng, rows, np.array([-1]), rng.standard_normal((1, d)).astype(np.float32), space,
                                      f"{space} {live} live rows")
        assert sizes.tolist() == [live]
    finally:
        eng.close()


@pytest.mark.parametrize("space", ["l2", "cosine"])
@pytest.mark.parametrize("n,d", [(5000, 16), (300, 768)])
def test_the_means_of_seven_clusters(space, n, d):
    eng, rows, rng = _corpus(space, n, d, n + d, tomb=1 / 3)
    try:
        lab = rng.choice(_live(eng).nonzero()[0], 7).astype(np.int64)
        lab[2] = -1
        lab[5] = lab[1]  # a duplicate: cluster 5 stays empty and keeps its centroid
        sizes = _replay_one_iteration(eng, rows, lab, rng.standard_normal((7, d)).astype(np.float32), space, f"{space} {n}x{d}")
        assert sizes[5] == 0 and (sizes > kernel_segment()).any() == (n >= 5000)
    finally:
        eng.close()


def kernel_segment():
    return _native.CLUSTER_SEGMENT


# ---------------------------------------------------------------- 3. whole runs
def _loose_blobs(rng, n, d, k, spread):
    centres = rng.standard_normal((k, d)) * spread
    return (centres[rng.integers(k, size=n)] + rng.standard_normal((n, d))).astype(np.float32)


@pytest.mark.parametrize("space", ["l2", "cosine"])
def test_whole_runs_equal_the_models_loop_on_the_devices_own_distances(space):
    rng = np.random.default_rng(3)
    n, d, m = 700, 24, 5
    eng, rows, rng = _corpus(space, n, d, 17, tomb=0.2, rows=_loose_blobs(rng, n, d, 4, 1.5))
    try:
        live = _live(eng)
        lab = rng.choice(np.flatnonzero(live), m, replace=False).astype(np.int64)
        seen = set()
        for max_iterations in (1, 2, 25):
            want = model_kmeans(lambda c: _distances(eng, c), rows, live, rows[lab], space, max_iterations)
            eng.set_attr(COL, 0, np.full(n, KEPT, np.int64))
            got = eng.kmeans(lab, max_iterations=max_iterations, assign_attr=COL)
            again = eng.kmeans(lab, max_iterations=max_iterations, assign_attr=COL)
            for g, a in zip(got[:3], again[:3]):
                assert g.tobytes() == a.tobytes(), "two calls differ"
            assert got[3:] == again[3:]
            cent, sizes, costs, iterations, converged, matched = got
            assert (iterations, converged) == (want[3], bool(want[4])), f"max_iterations={max_iterations}"
            assert matched == int(live.sum()) and iterations <= max_iterations
            _same_bits(cent, want[0], "centroids")
            assert np.array_equal(sizes, want[1])
            _same_bits(costs, want[2], "costs")
            col = eng.get_attr(COL, 0, n)
            assert np.array_equal(col, _column_want(want[5], np.full(n, KEPT)))
            if converged:  # the column is the assignment against the returned centroids
                sizes2, costs2, _ = eng.assign_nearest(None, cent, assign_attr=COL)
                assert np.array_equal(eng.get_attr(COL, 0, n), col) and np.array_equal(sizes2, sizes)
                _same_bits(costs2, costs, "costs against the returned centroids")
            seen.add(converged)
        assert seen == {False, True}, "the runs never converged (or always did)"
    finally:
        eng.close()


# ---------------------------------------------------------------- 4. against the NumPy oracle
@pytest.mark.parametrize("space", ["l2", "cosine"])
def test_separated_blobs_are_recovered(space):
    rng = np.random.default_rng(8)
    n, d, k = 1200, 32, 6
    centres = rng.standard_normal((k, d)) * 20.0
    blob = rng.integers(k, size=n)
    rows = (centres[blob] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    eng, rows, rng = _corpus(space, n, d, 1, rows=rows)
    try:
        seeds = np.array([np.flatnonzero(blob == j)[0] for j in range(k)])
        cent, sizes, costs, iterations, converged, matched = eng.kmeans(seeds, max_iterations=10, assign_attr=COL)
        assert converged and iterations == 2 and matched == n
        assert np.array_equal(eng.get_attr(COL, 0, n), blob)
        assert np.array_equal(sizes, np.bincount(blob, minlength=k))
        x = rows.astype(np.float64)
        if space == "cosine":
            x = x / np.sqrt((x * x).sum(axis=1))[:, None]
        for j in range(k):
            want = x[blob == j].mean(axis=0).astype(np.float32)
            assert (np.abs(cent[j] - want) <= np.spacing(np.abs(want))).all(), f"centroid {j}"
    finally:
        eng.close()


ORACLE_CASES = (("l2", 3000, 48, 21), ("cosine", 3000, 48, 22), ("ip", 3000, 48, 23))


def oracle_case(space, n, d, seed):
    """Gaussian rows and 12 Gaussian centroids; (rows, centroids, the oracle's argmin, the rows whose two best oracle
    distances are more than GAP_MIN apart)."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    cent = rng.standard_normal((12, d)).astype(np.float32)
    D = exact_scan.exact_distances(cent, rows, space)
    two = np.sort(D, axis=0)[:2]
    return rows, cent, D.argmin(axis=0), (two[1] - two[0]) > GAP_MIN


@pytest.mark.parametrize("space,n,d,seed", ORACLE_CASES)
def test_gaussian_rows_get_the_oracles_nearest_centroid(space, n, d, seed):
    rows, cent, want, asked = oracle_case(space, n, d, seed)
    assert asked.all(), "the seed leaves rows out (tests/test_cluster_host.py checks this without a device)"
    eng, rows, rng = _corpus(space, n, d, 1, rows=rows)
    try:
        sizes, costs, matched = eng.assign_nearest(None, cent, assign_attr=COL)
        col = eng.get_attr(COL, 0, n)
        assert matched == n and np.array_equal(col[asked], want[asked])
        assert np.array_equal(sizes, np.bincount(col, minlength=12))
    finally:
        eng.close()


# ---------------------------------------------------------------- 5. structure
def test_filters_restrict_the_candidates_and_may_read_the_column_itself():
    n, d = 900, 16
    eng, rows, rng = _corpus("l2", n, d, 4, tomb=0.25)
    try:
        dead = ~_live(eng)
        lab, vec = _random_centroids(rng, 9, n, d, dead)
        _replay_assign(eng, rows, lab, vec, "tag == 2", where=W1(W.EQ, TAG, 2))
        _replay_assign(eng, rows, lab, vec, "tag in (0, 4)", where=W1(W.IN, TAG, 0, 2, (0, 4)))
        # every live row into the column, then only the members of cluster 1 against other centroids: the mask is the
        # column from BEFORE the call, although the call overwrites exactly those rows
        _replay_assign(eng, rows, lab, vec, "all")
        members = _live(eng, W1(W.EQ, COL, 1))
        assert members.any()
        lab2, vec2 = _random_centroids(rng, 4, n, d, dead)
        assign = _replay_assign(eng, rows, lab2, vec2, "column == 1", where=W1(W.EQ, COL, 1))
        assert np.array_equal(assign != NO_CANDIDATE, members)
        # no column at all
        before = eng.get_attr(COL, 0, n)
        _replay_assign(eng, rows, lab, vec, "no column", attr=-1)
        assert np.array_equal(eng.get_attr(COL, 0, n), before)
        # k-means under a filter
        want = model_kmeans(lambda c: _distances(eng, c), rows, _live(eng, W1(W.EQ, TAG, 3)), centroid_vectors(rows, lab2, vec2),
                            "l2", 3)
        cent, sizes, costs, iterations, converged, matched = eng.kmeans(lab2, vec2, max_iterations=3, where=W1(W.EQ, TAG, 3),
                                                                        assign_attr=COL)
        _same_bits(cent, want[0], "filtered k-means")
        assert np.array_equal(eng.get_attr(COL, 0, n), _column_want(want[5], before))
    finally:
        eng.close()


def test_more_centroids_than_candidates_no_candidate_and_an_empty_index():
    d = 8
    eng = HipScanEngine(d, "l2", device=0)
    try:
        raw = np.arange(3 * d, dtype=np.float32).reshape(3, d)
        sizes, costs, matched = eng.assign_nearest(None, raw)
        assert sizes.tolist() == [0, 0, 0] and costs.tolist() == [0.0, 0.0, 0.0] and matched == 0
        cent, sizes, costs, iterations, converged, matched = eng.kmeans(None, raw, max_iterations=7)
        _same_bits(cent, raw, "an empty index keeps C_0")
        assert sizes.tolist() == [0, 0, 0] and costs.tolist() == [0.0, 0.0, 0.0] and matched == 0
        assert (iterations, converged) == (2, True)
        assert eng.kmeans(None, raw, max_iterations=1)[3:5] == (1, False)
    finally:
        eng.close()
    eng, rows, rng = _corpus("l2", 5, d, 2)
    try:
        lab, vec = np.array([0, -1, 3, -1, 4, -1, 2, 1, -1]), rng.standard_normal((9, d)).astype(np.float32)
        assign = _replay_assign(eng, rows, lab, vec, "9 centroids, 5 rows")
        assert assign.tolist() == [0, 7, 6, 2, 4]  # every row is its own centroid
        # no candidate: a filter nothing matches, then every row tombstoned
        c0 = centroid_vectors(rows, lab, vec)
        for step in ("filter", "tombstoned"):
            where = W1(W.EQ, TAG, 99) if step == "filter" else None
            if step == "tombstoned":
                eng.tombstone(np.arange(5))
            before = eng.get_attr(COL, 0, 5)
            cent, sizes, costs, iterations, converged, matched = eng.kmeans(lab, vec, max_iterations=9, where=where, assign_attr=COL)
            _same_bits(cent, c0, f"{step}: C_0 kept")
            assert not sizes.any() and not costs.any() and matched == 0 and (iterations, converged) == (2, True), step
            sizes, costs, matched = eng.assign_nearest(lab, vec, where=where, assign_attr=COL)
            assert not sizes.any() and not costs.any() and matched == 0
            assert np.array_equal(eng.get_attr(COL, 0, 5), before), step
    finally:
        eng.close()


def test_reruns_after_append_tombstone_and_compact():
    n, d = 600, 16
    eng, rows, rng = _corpus("cosine", n, d, 6)
    try:
        lab, vec = _random_centroids(rng, 6, n, d, np.zeros(n, bool))

        def check(tag, rows):
            _replay_assign(eng, rows, lab, vec, tag)
            _replay_one_iteration(eng, rows, lab, vec, "cosine", tag)

        check("fresh", rows)
        more = rng.standard_normal((300, d)).astype(np.float32)
        eng.append(more)
        rows = np.concatenate([rows, more])
        check("appended", rows)  # (the new rows' column is absent before the call)
        eng.tombstone(rng.choice(900, 250, replace=False))
        check("tombstoned", rows)
        old = eng.compact()
        rows = rows[old]  # (the stored centroids' labels now name other rows: still inside the index)
        check("compacted", rows)
    finally:
        eng.close()


def test_the_c_level_refusals_launch_nothing_and_write_nothing():
    n, d = 100, 8
    eng, rows, rng = _corpus("l2", n, d, 1)
    ip = HipScanEngine(d, "ip", device=0)
    try:
        ip.append(rows)
        lib = _native.load()
        eng.define_attr(2, "float64")
        eng.last_stats()
        good = dict(eng=eng, labels=[1, -1, 2], vectors=np.ones((3, d), np.float32), m=3, max_iterations=5, where=None, attr=COL,
                    null=None)

        def call(entry, **kw):
            a = {**good, **kw}
            labels = None if a["labels"] is None else np.asarray(a["labels"], np.int64)
            m = a["m"]
            outs = [np.full((max(m, 1), d), -7, np.float32), np.full(max(m, 1), -7, np.int64), np.full(max(m, 1), -7.0)]
            it, conv, matched = (np.full(1, -7, np.int32), np.full(1, -7, np.int32), np.full(1, -7, np.int64))
            ptr = lambda i, o: None if a["null"] == i else o.ctypes.data  # noqa: E731
            w, keep = a["eng"]._where_arg(a["where"])
            h, vec = a["eng"].handle, a["vectors"]
            lab_p, vec_p = None if labels is None else labels.ctypes.data, None if vec is None else vec.ctypes.data
            if entry == "assign":
                rc = lib.mlvdb_assign_nearest(h, lab_p, vec_p, m, w, a["attr"], ptr(1, outs[1]), ptr(2, outs[2]),
                                              None if a["null"] == 5 else matched.ctypes.data_as(_native.C.POINTER(_native.C.c_int64)))
            else:
                P32 = _native.C.POINTER(_native.C.c_int32)
                rc = lib.mlvdb_kmeans(h, lab_p, vec_p, m, a["max_iterations"], w, a["attr"], ptr(0, outs[0]), ptr(1, outs[1]),
                                      ptr(2, outs[2]), None if a["null"] == 3 else it.ctypes.data_as(P32),
                                      None if a["null"] == 4 else conv.ctypes.data_as(P32),
                                      None if a["null"] == 5 else matched.ctypes.data_as(_native.C.POINTER(_native.C.c_int64)))
            assert all((o == -7).all() for o in outs + [it, conv, matched]), "a refused call wrote to its outputs"
            return rc

        INVALID, UNSUPPORTED = 1, 6
        bad_vec = np.ones((3, d), np.float32)
        bad_vec[1, 3] = np.inf
        both = {
            "m = 0": (dict(m=0), INVALID),
            "m = 1025": (dict(m=1025, labels=[1] * 1025, vectors=None), INVALID),
            "label = total": (dict(labels=[1, -1, n]), INVALID),
            "label = -2": (dict(labels=[1, -1, -2]), INVALID),
            "a raw centroid without vectors": (dict(vectors=None), INVALID),
            "neither labels nor vectors": (dict(labels=None, vectors=None), INVALID),
            "a non-finite raw vector": (dict(vectors=bad_vec), INVALID),
            "an undefined column": (dict(attr=7), INVALID),
            "a float64 column": (dict(attr=2), INVALID),
            "a column outside the table": (dict(attr=16), INVALID),
            "column -2": (dict(attr=-2), INVALID),
            "a bad program": (dict(where=W1(W.EQ, 9, 1)), INVALID),
            "null sizes": (dict(null=1), INVALID),
            "null costs": (dict(null=2), INVALID),
            "null matched": (dict(null=5), INVALID),
        }
        kmeans_only = {
            "max_iterations = 0": (dict(max_iterations=0), INVALID),
            "max_iterations above the bound": (dict(max_iterations=_native.CLUSTER_MAX_ITERATIONS + 1), UNSUPPORTED),
            "an ip index": (dict(eng=ip, attr=-1), UNSUPPORTED),
            "null centroids": (dict(null=0), INVALID),
            "null iterations": (dict(null=3), INVALID),
            "null converged": (dict(null=4), INVALID),
        }
        for what, (kw, code) in both.items():
            assert call("assign", **kw) == code, f"assign_nearest: {what}"
        for what, (kw, code) in {**both, **kmeans_only}.items():
            assert call("kmeans", **kw) == code, f"kmeans: {what}"
        st = eng.last_stats()
        assert st["scan_launches"] == 0 and st["rows_scanned"] == 0
        assert (eng.get_attr(COL, 0, n) == KEPT).all(), "a refused call wrote to the column"
        with pytest.raises(RuntimeError, match=r"kmeans failed \(6\).*l2 or cosine"):
            ip.kmeans([1, 2])
        with pytest.raises(RuntimeError, match=r"assign_nearest failed \(1\).*int64 column"):
            eng.assign_nearest([1, 2], assign_attr=2)
        sizes, costs, matched = ip.assign_nearest([1, 2])  # ip is served by the assignment
        assert matched == n and sizes.sum() <= n
        _replay_assign(eng, rows, np.array([3, -1, 9]), np.ones((3, d), np.float32), "after the refusals")
        assert eng.last_stats()["scan_launches"] >= 1
    finally:
        eng.close()
        ip.close()
