"""k-means++ seeding on the MI355X (include/mlvdb_seed.h), at the engine level through the C ABI: the header's steps of
tests/seed_helpers.py run on the device's own bits -- ``pair_distances(stored row s, every label)`` for every d(s, x) -- must
reproduce the picks and, bit for bit, the potentials.  No tolerance."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.seed_helpers import model_seed, seed_u

pytestmark = pytest.mark.gpu

TAG = 0


def W1(op, attr, a=0, b=0, table=()):
    return W.Program(np.array([(op, attr, a, b)], dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


def _engine(space, rows, batches=1, tomb=0.0):
    eng = HipScanEngine(rows.shape[1], space, device=0)
    for part in np.array_split(rows, batches):
        eng.append(part)
    if tomb:
        eng.tombstone(np.flatnonzero(np.random.default_rng(1).random(rows.shape[0]) < tomb))
    eng.define_attr(TAG, "int64")
    eng.set_attr(TAG, 0, np.arange(rows.shape[0], dtype=np.int64) % 25)
    return eng


def _gauss(n, d):
    return np.random.default_rng(11 * n + d).standard_normal((n, d), dtype=np.float32)


THIRD = W1(W.IN, TAG, 0, 8, tuple(range(8)))  # 8 of 25 tag values
FORTY = W1(W.EQ, TAG, 3)                      # rows 3, 28, .. 978 of 1,003

# (space, rows, dim, m, trials, where, tombstoned share, append batches)
CASES = {
    "l2 ragged last block": ("l2", 1003, 20, 5, 8, None, 0.0, 1),
    "cosine ragged last block": ("cosine", 1003, 20, 5, 8, None, 0.0, 1),
    "a block holding one row": ("l2", 257, 16, 3, 1, None, 0.0, 1),
    "tile width 4, two launches per step": ("l2", 300, 1040, 4, 8, None, 0.0, 1),
    "tombstones, a filter, three batches": ("cosine", 1003, 20, 5, 3, THIRD, 0.1, 3),
    "five distinct vectors": ("l2", 640, 16, 8, 2, None, 0.0, 1),
    "m = 1": ("l2", 1003, 20, 1, 8, None, 0.0, 1),
    "m = the candidates": ("l2", 1003, 20, 40, 2, FORTY, 0.0, 1),
    "upper tree in one launch": ("l2", 65536, 16, 2, 2, None, 0.0, 1),
    "upper tree in two launches": ("l2", 65537, 16, 2, 2, None, 0.0, 1),
}


@pytest.mark.parametrize("case", CASES)
def test_the_seeding_equals_the_headers_steps_replayed_on_the_devices_own_bits(case):
    space, n, d, m, trials, where, tomb, batches = CASES[case]
    rows = _gauss(n, d)
    if case == "five distinct vectors":
        rows = rows[:5][np.random.default_rng(2).integers(5, size=n)]
    eng = _engine(space, rows, batches, tomb)
    try:
        live = np.zeros(n, bool)
        live[eng.where_labels(where if where is not None else W1(W.TRUE, 0))] = True
        every = np.arange(n)[None, :]
        u = seed_u(len(case), m, trials)
        want_labels, want_pot, candidates = model_seed(lambda s: eng.pair_distances(rows[s:s + 1], every)[0][0], live, m, u)
        labels, pot, matched = eng.kmeans_seed(m, u, where=where)
        again = eng.kmeans_seed(m, u, where=where)
        assert matched == candidates == int(live.sum()) and (where is None and not tomb) == (candidates == n)
        assert labels.tolist() == want_labels.tolist(), f"potentials {pot.tolist()} want {want_pot.tolist()}"
        assert pot.tobytes() == want_pot.tobytes(), f"{pot.tolist()} want {want_pot.tolist()}"
        assert again[0].tobytes() == labels.tobytes() and again[1].tobytes() == pot.tobytes(), "two calls differ"
        assert live[labels].all() and (np.diff(pot) <= 0).all()
        if case == "five distinct vectors":  # zero weights from the fifth pick on, the fallback draw, duplicate picks
            assert (pot[4:] == 0).all() and pot[3] > 0 and np.unique(rows[labels[:5]], axis=0).shape[0] == 5
        if case == "m = the candidates":
            assert candidates == 40 == m
    finally:
        eng.close()


def test_the_c_level_refusals_write_nothing_and_the_handle_still_answers():
    n, d = 100, 8
    rows = _gauss(n, d)
    eng, ip, empty = _engine("l2", rows), HipScanEngine(d, "ip", device=0), HipScanEngine(d, "l2", device=0)
    try:
        ip.append(rows)
        lib = _native.load()
        eng.last_stats()

        def call(eng=eng, m=3, trials=2, u=None, where=None, null=None, matched_written=-7):
            u = np.full((max(m, 1), max(trials, 1)), 0.5) if u is None else np.asarray(u, np.float64)
            labels, pot, matched = np.full(max(m, 1), -7, np.int64), np.full(max(m, 1), -7.0), np.full(1, -7, np.int64)
            w, keep = eng._where_arg(where)
            ptr = lambda i, o: None if null == i else o.ctypes.data  # noqa: E731
            rc = lib.mlvdb_kmeans_seed(eng.handle, m, trials, ptr(0, u), w, ptr(1, labels), ptr(2, pot),
                                       None if null == 3 else matched.ctypes.data_as(C.POINTER(C.c_int64)))
            assert (labels == -7).all() and (pot == -7).all() and matched[0] == matched_written, "a refused call wrote"
            return rc

        INVALID, UNSUPPORTED = 1, 6
        half = [[0.5, 0.5]] * 2
        refusals = {
            "m = 0": (dict(m=0), INVALID), "m = 1025": (dict(m=1025), INVALID),
            "trials = 0": (dict(trials=0), INVALID), "trials = 9": (dict(trials=9), INVALID),
            "u = 1": (dict(u=half + [[0.5, 1.0]]), INVALID), "u < 0": (dict(u=half + [[-1e-300, 0.5]]), INVALID),
            "u a NaN": (dict(u=half + [[0.5, np.nan]]), INVALID), "u = inf": (dict(u=[[np.inf, 0.5]] + half), INVALID),
            "null u": (dict(null=0), INVALID), "null labels": (dict(null=1), INVALID),
            "null potentials": (dict(null=2), INVALID), "null matched": (dict(null=3), INVALID),
            "a bad program": (dict(where=W1(W.EQ, 9, 1)), INVALID), "an ip index": (dict(eng=ip), UNSUPPORTED),
            # fewer candidates than m: known after the one count, which is written
            "a filter's 4 rows": (dict(m=5, where=W1(W.EQ, TAG, 3), matched_written=4), INVALID),
            "m = total + 1": (dict(m=101, matched_written=100), INVALID),
            "an empty index": (dict(eng=empty, m=1, matched_written=0), INVALID),
        }
        for what, (kw, code) in refusals.items():
            assert call(**kw) == code, what
        st = eng.last_stats()
        assert st["scan_launches"] == 0 and st["rows_scanned"] == 0
        with pytest.raises(RuntimeError, match=r"kmeans_seed failed \(1\).*fewer candidates"):
            eng.kmeans_seed(101, np.zeros((101, 1)))
        labels, dist, counts = eng.search(rows[:2], 3)
        assert labels[:, 0].tolist() == [0, 1] and counts.tolist() == [3, 3]
        assert eng.kmeans_seed(100, np.full((100, 1), 0.5))[2] == 100
    finally:
        eng.close()
        ip.close()
        empty.close()


def test_index_cluster_from_kmeanspp_equals_kmeans_from_the_seeds_ids():
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((400, 24)) + 5.0 * rng.integers(0, 2, (400, 24))).astype(np.float32)
    index = Index(space="l2", attributes={"tag": "int"})
    try:
        index.add([Vector(values=r, metadata={"tag": i % 3}) for i, r in enumerate(rows)], "ns")
        ids, pot = index.cluster_seeds("ns", "l2", 7, where={"tag": 1}, seed=4)
        assert len(set(ids)) == 7 and (np.diff(pot) <= 0).all()
        got = index.cluster("ns", "l2", 7, where={"tag": 1}, init="k-means++", seed=4, max_iterations=4)
        want = index.cluster("ns", "l2", 7, where={"tag": 1}, init=ids, max_iterations=4)
        assert got.centroids.tobytes() == want.centroids.tobytes() and got.costs.tobytes() == want.costs.tobytes()
        assert np.array_equal(got.sizes, want.sizes) and got.iterations == want.iterations
    finally:
        index.close()
