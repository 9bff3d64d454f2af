"""The helpers of tests/test_gpu_knn_limits.py, checked without a device: the launch-plan mirrors against figures worked out
by hand from kernels_exact.hip / api.hip, the planted-row builders and the gap assertion against the oracle."""
import importlib

import numpy as np
import pytest

from oracle import exact_scan
from tests import knn_limits_helpers as H

SPACES = ["l2", "cosine", "ip"]


def test_the_gpu_file_imports_without_a_device():
    mod = importlib.import_module("tests.test_gpu_knn_limits")
    assert mod.pytestmark.name == "gpu"


# ---------------------------------------------------------------- launch plans
@pytest.mark.parametrize("nq,ld,qt,nw,pw", [
    (1, 112, 1, 16, 2), (2, 112, 2, 16, 2), (3, 112, 2, 16, 2), (4, 112, 4, 8, 4), (7, 112, 4, 8, 4), (8, 112, 8, 8, 2),
    (17, 112, 8, 8, 2),
    (9, 1024, 8, 8, 2), (9, 1040, 4, 8, 4), (9, 2048, 4, 8, 4), (9, 2064, 2, 16, 2), (9, 4096, 2, 16, 2), (9, 4112, 1, 16, 2),
    (9, 8192, 1, 16, 2), (3, 4096, 2, 16, 2), (3, 4112, 1, 16, 2),
])
def test_plan_exact_query_tiles(nq, ld, qt, nw, pw):
    p = H.plan_exact(1000, ld, nq)
    assert (p.qt, p.nw, p.pw) == (qt, nw, pw)
    assert p.nqtiles == -(-nq // qt)
    assert p.qt * ld * 8 <= 64 * 1024 and p.lds_bytes <= 64 * 1024
    assert p.qt == 1 or p.qt == min(8, 1 << (nq.bit_length() - 1)) or 2 * p.qt * ld * 8 > 64 * 1024  # halved only when it must be


def test_plan_exact_blocks_and_row_owners():
    # 1,100 rows = 69 panels; QT 8: 35 tasks / 8 waves = 5 blocks; QT 4: 18 tasks / 8 = 3; QT 2: 35 tasks / 16 = 3
    assert [H.plan_exact(1100, 32, nq).nblk for nq in (9, 4, 2)] == [5, 3, 3]
    assert H.plan_exact(512, 32, 2).nblk == 1 and H.plan_exact(513, 32, 2).nblk == 2    # 16 x 2 x 16 rows per block
    assert H.plan_exact(512, 32, 4).nblk == 1 and H.plan_exact(513, 32, 4).nblk == 2    # 16 x 4 x 8
    assert H.plan_exact(256, 32, 9).nblk == 1 and H.plan_exact(257, 32, 9).nblk == 2    # 16 x 2 x 8
    assert H.plan_exact(10 ** 7, 768, 8).nblk == 256 and H.plan_exact(10 ** 7, 768, 4096).nblk == 8  # the caps
    big = H.plan_exact(64, 16, 8 * 65_535 + 16)
    assert (big.qt, big.nqtiles, big.nblk) == (8, 65_537, 1)
    p = H.plan_exact(1100, 32, 9)
    assert H.exact_owner(0, p) == (0, 0) and H.exact_owner(31, p) == (0, 0) and H.exact_owner(32, p) == (0, 1)
    assert H.exact_owner(255, p) == (0, 7) and H.exact_owner(256, p) == (1, 0) and H.exact_owner(1099, p) == (4, 2)


def test_filter_rounds_formula():
    # the defaults: seed 3,840, rounds end at 65,280 and 1,572,864 rows
    assert H.filter_rounds(10_000_000, 5, 85, 2048) == [(3840, 65280), (65280, 1572864), (1572864, 10_000_000)]
    assert H.filter_rounds(65280, 5, 85, 2048) == [(3840, 65280)] and H.filter_rounds(65281, 5, 85, 2048)[-1] == (65280, 65281)
    assert H.filter_rounds(3840, 5, 85, 2048) == [] and H.filter_rounds(3841, 5, 85, 2048) == [(3840, 3841)]
    # SEED_ROWS=1 ROUND1=6 ROUND2=7
    assert H.filter_rounds(6200, 1, 6, 7) == [(768, 4608), (4608, 5376), (5376, 6200)]
    assert [len(H.filter_rounds(t, 1, 6, 7)) for t in (767, 768, 769, 4607, 4608, 4609, 5375, 5376, 5377)] == [0, 0, 1, 1, 1, 2, 2, 2, 3]
    assert H.filter_rounds(6200, 1, 6, 7, prefix_seed=True) == [(0, 4608), (4608, 5376), (5376, 6200)]
    # a call of 257 queries: a full pass, then one query that seeds from the exact prefix on the int8 shadow
    assert H.filter_call_rounds(6200, 257, 1, 6, 7, int8=True) == [H.filter_rounds(6200, 1, 6, 7), H.filter_rounds(6200, 1, 6, 7, True)]
    assert H.filter_call_rounds(6200, 257, 1, 6, 7, int8=False) == [H.filter_rounds(6200, 1, 6, 7)] * 2
    assert H.filter_call_rounds(6200, 256, 1, 6, 7, int8=True) == [H.filter_rounds(6200, 1, 6, 7)]
    assert len(H.filter_call_rounds(6200, 513, 1, 6, 7, int8=True)) == 3
    # ROUND1 is at least 6 units, ROUND2 at least ROUND1, the seed at most 3,840 rows
    assert H.filter_rounds(6200, 9, 1, 1) == [(3840, 4608), (4608, 6200)] == H.filter_rounds(6200, 5, 6, 6)


def test_bigk_rounds_formula():
    assert H.bigk_seed_rows(30_000, 20, 65) == 3840 and H.bigk_seed_rows(30_000, 20, 300) == 3840
    assert H.bigk_seed_rows(40_000, 4, 1024) == 4608 and H.bigk_seed_rows(150_001, 40, 1000) == 10752
    assert H.bigk_seed_rows(10 ** 6, 256, 1000) == 65280 and H.bigk_seed_rows(3000, 20, 100) == 3072
    assert H.bigk_growth(20, 300, 1) == 1.5 and H.bigk_growth(20, 65, 10 ** 8) == 24.0
    assert H.bigk_growth(20, 300, 10 ** 8) == 1.0 + 4096.0 / 300
    chain = H.bigk_rounds(30_000, 20, 65, 1)
    assert chain[:3] == [(3840, 5376), (5376, 7680), (7680, 11520)] and chain[-1][1] == 30_000
    assert all(a[1] == b[0] for a, b in zip(chain, chain[1:]))
    assert chain[3:] == [(11520, 16896), (16896, 30_000)]  # 16,896 x 1.5 = 25,344, x 1.25 > 30,000: no sliver of a last round
    assert H.bigk_rounds(30_000, 20, 65, 10 ** 8) == [(3840, 30_000)]
    assert H.bigk_rounds(3000, 20, 100, 1) == []


def test_routes():
    assert [H.knn_route(k, 10 ** 5) for k in (64, 65, 1024, 1025)] == ["filter", "bigk", "bigk", "paged"]
    assert [H.knn_route(k, 200) for k in (199, 200, 201)] == ["bigk", "paged", "paged"]
    assert H.knn_route(10, 100, filter_path=False) == "exact" and H.knn_route(100, 10 ** 5, filter_path=False) == "paged"


# ---------------------------------------------------------------- the gap assertion
def test_gap_assertion():
    assert H.gap_ok(1.0, 1.0) and H.gap_ok(0.0, 0.0) and H.gap_ok(1.0, 1.0 + 1e-8) and H.gap_ok(-767.0, -766.0)
    assert not H.gap_ok(1.0, 1.0 + 1e-10) and not H.gap_ok(-767.0, np.nextafter(-767.0, 0.0))
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((50, 8), dtype=np.float32)
    qs = rng.standard_normal((3, 8), dtype=np.float32)
    srt, lab = H.assert_cuts(qs, rows, "l2", [5, 10, 60])
    d = exact_scan.exact_distances(qs, rows, "l2")
    assert np.array_equal(srt, np.sort(d, axis=1)) and np.array_equal(np.take_along_axis(d, lab, axis=1), srt)
    # a row one fp32 ulp away from another, in one component of 8: relative distance gap below 1e-9 for a query far from both
    rows[7] = rows[3]
    rows[7, 0] = np.nextafter(rows[3, 0], np.float32(np.inf))
    far = (rows[3] + 100.0).astype(np.float32)[None, :]
    srt, lab = H.sorted_live_distances(far, rows, "l2")
    cut = int(np.nonzero(np.isin(lab[0], [3, 7]))[0].max())
    assert not H.gap_ok(srt[0, cut - 1], srt[0, cut])
    with pytest.raises(AssertionError, match="near-tie"):
        H.assert_cuts(far, rows, "l2", [cut])
    rows[7] = rows[3]  # bit-identical: an intended tie
    H.assert_cuts(far, rows, "l2", [cut])


# ---------------------------------------------------------------- planted rows
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("d", [24, 64, 256])
def test_planted_rows_are_the_oracles_nearest(d, space):
    rng = np.random.default_rng(2 + d)
    rows = rng.standard_normal((3000, d), dtype=np.float32)
    qs = rng.standard_normal((6, d), dtype=np.float32)
    deleted = np.zeros(3000, dtype=bool)
    deleted[::9] = True
    placements = [(0, 1), (1, 767), (2, 2999)]
    H.plant(rows, qs, space, placements, rng)
    H.plant_pair(rows, qs, space, 3, 100, 2000, rng)
    deleted[[1, 767, 2999, 100, 2000]] = False
    H.assert_rank0(qs, rows, space, placements + [(3, 100)], deleted)
    labels, dist, _ = exact_scan.knn(qs, rows, 2, space, deleted=deleted)
    assert labels[3].tolist() == [100, 2000] and dist[3, 0] == dist[3, 1]
    with pytest.raises(AssertionError, match="planted"):
        H.assert_rank0(qs, rows, space, [(4, 5)], deleted)
    deleted[767] = True  # a tombstoned planted row is no longer the nearest
    with pytest.raises(AssertionError, match="planted"):
        H.assert_rank0(qs, rows, space, placements, deleted)


@pytest.mark.parametrize("space", SPACES)
def test_tie_group_sits_at_its_ranks(space):
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((300, 16), dtype=np.float32)
    qs = rng.standard_normal((2, 16), dtype=np.float32)
    deleted = np.zeros(300, dtype=bool)
    deleted[::7] = True
    group = H.plant_tie_group(rows, qs, space, 1, 62, 5, deleted)
    labels, dist, _ = exact_scan.knn(qs, rows, 70, space, deleted=deleted)
    assert labels[1, 62:67].tolist() == group.tolist() and not deleted[group].any()
    srt, lab = H.sorted_live_distances(qs, rows, space, deleted)
    assert np.array_equal(lab[:, :70], labels)
    assert srt[1, 62] == srt[1, 66] and srt[1, 61] < srt[1, 62] < srt[1, 67]


def test_slabbed_oracles_equal_the_oracle():
    rng = np.random.default_rng(6)
    rows = rng.standard_normal((64, 8), dtype=np.float32)
    rows[40] = rows[9]
    qs = rng.standard_normal((500, 8), dtype=np.float32)
    deleted = np.zeros(64, dtype=bool)
    deleted[5] = True
    for space in SPACES:
        want = exact_scan.knn(qs, rows, 3, space, deleted=deleted)
        got = H.oracle_knn(qs, rows, 3, space, deleted, slab=7)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        wl, wd, _ = exact_scan.knn(qs, rows, 2, space)
        gl, gd, g64 = H.oracle_topk_dense(qs, rows, 2, space, slab=128)
        assert np.array_equal(gl, wl) and np.array_equal(gd, wd) and g64.shape == (500, 3)
