"""Preconditions of tests/test_gpu_magnitudes.py, on the oracle alone (no GPU): every case that file sends to the device is
finite, and the oracle's own answer for it does not depend on the order of summation (tests/magnitude_helpers.py:
oracle_is_stable), so a device answer that differs is the device's fault.  No case is skipped or redrawn at run time: a seed
that fails a precondition is replaced in magnitude_helpers.py."""
import numpy as np
import pytest

from oracle import exact_scan
from tests import magnitude_helpers as mh
from tests.helpers import SCORE_ATOL


# ---------------------------------------------------------------- the helpers themselves
def test_pow2_and_uniform_scaling_are_exact_in_the_normal_range():
    assert float(mh.pow2(-149)) == 2.0 ** -149 and float(mh.pow2(127)) == 2.0 ** 127
    base, bq = mh.make_case(mh.UNIFORM_SEED, 50, 8, 3, dup=True)
    for e in (-100, 40, 124):
        rows, qs = mh.uniform_case(mh.UNIFORM_SEED, 50, 8, 3, e)
        assert np.array_equal(rows.astype(np.float64), base.astype(np.float64) * 2.0 ** e)
        assert np.array_equal(qs.astype(np.float64), bq.astype(np.float64) * 2.0 ** e)
    rows, _ = mh.uniform_case(mh.UNIFORM_SEED, 50, 8, 3, -140)
    assert np.array_equal(rows, np.rint(base.astype(np.float64) * 2.0 ** 9).astype(np.float32) * mh.pow2(-149))
    with pytest.raises(AssertionError):
        mh.uniform_case(mh.UNIFORM_SEED, 50, 8, 3, 127)


def test_assert_knn_matches_rel_bars():
    lab = np.array([[3, 5, -1]], dtype=np.int64)
    cnt = np.array([2], dtype=np.int32)
    inf = np.float32(np.inf)
    want = (lab, np.array([[1e30, inf, inf]], dtype=np.float32), cnt)
    mh.assert_knn_matches_rel((lab, np.array([[1e30 * (1 + 5e-6), inf, inf]], dtype=np.float32), cnt), want, "ok")
    for bad in ([1e30 * (1 + 3e-5), inf, inf],   # beyond 1e-5 relative
                [1e30, 3.0e38, inf],             # finite against infinite
                [1e30, -inf, inf],               # the other infinity
                [1e30, inf, 3.4e38],             # padding that is not +inf
                [np.nan, inf, inf]):
        with pytest.raises(AssertionError):
            mh.assert_knn_matches_rel((lab, np.array([bad], dtype=np.float32), cnt), want, "bad")
    with pytest.raises(AssertionError):  # a real row at +inf is no padding: its label must come back
        mh.assert_knn_matches_rel((np.array([[3, -1, -1]], dtype=np.int64), want[1], cnt), want, "label")
    with pytest.raises(AssertionError):
        mh.assert_knn_matches_rel((lab, want[1], np.array([1], dtype=np.int32)), want, "count")
    small = (lab, np.array([[0.0, 2e-6, inf]], dtype=np.float32), cnt)
    mh.assert_knn_matches_rel((lab, np.array([[9e-6, 0.0, inf]], dtype=np.float32), cnt), small, "absolute below 1")
    assert SCORE_ATOL == 1e-5


def test_assert_fp64_matches_bars():
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((20, 16), dtype=np.float32) * mh.pow2(40)
    qs = rng.standard_normal((2, 16), dtype=np.float32) * mh.pow2(40)
    labels = np.array([[0, 4, -1], [7, 7, 19]], dtype=np.int64)
    for space in mh.SPACES:
        full = exact_scan.exact_distances(qs, rows, space)
        want = np.take_along_axis(full, np.maximum(labels, 0), axis=1)
        want[labels < 0] = np.inf
        mh.assert_fp64_matches(want, want.astype(np.float32), qs, rows, labels, space, space)
        off = want.copy()
        off[1, 2] += 1e-9 * max(1.0, abs(off[1, 2])) if space != "ip" else 1e-9 * np.abs(rows[19].astype(np.float64)) @ np.abs(qs[1])
        with pytest.raises(AssertionError):
            mh.assert_fp64_matches(off, None, qs, rows, labels, space, space)
        w32 = want.astype(np.float32)
        w32[0, 1] = np.nextafter(np.nextafter(w32[0, 1], np.float32(np.inf)), np.float32(np.inf))
        with pytest.raises(AssertionError):
            mh.assert_fp64_matches(want, w32, qs, rows, labels, space, space)
        # FLT_MAX against +inf is no "1 ulp": a finite fp32 face of an infinite rounding, or the reverse
        mh.assert_fp32_face(np.array([3.5e38, np.inf, 1.0]), np.array([np.inf, np.inf, np.nextafter(np.float32(1), np.float32(2))]), "ok")
        with pytest.raises(AssertionError):
            mh.assert_fp32_face(np.array([3.5e38]), np.array([mh.F32_MAX]), "finite face of an infinite rounding")
        with pytest.raises(AssertionError):
            mh.assert_fp32_face(np.array([float(mh.F32_MAX)]), np.array([np.inf], dtype=np.float32), "infinite face of FLT_MAX")
        pad = want.copy()
        pad[0, 2] = 3.4e38
        with pytest.raises(AssertionError):
            mh.assert_fp64_matches(pad, None, qs, rows, labels, space, space)


# ---------------------------------------------------------------- 1. uniform scale
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("e", mh.UNIFORM_EXPONENTS)
@pytest.mark.parametrize("d", mh.UNIFORM_DIMS)
def test_uniform_cases_are_finite_and_stable(d, e, space):
    rows, qs, deleted = mh.uniform_inputs(d, e)
    assert rows.shape == (mh.UNIFORM_N, d) and qs.shape == (mh.UNIFORM_NQ, d) and 100 < deleted.sum() < 200
    assert np.isfinite(rows).all() and np.isfinite(qs).all()
    assert mh.oracle_is_stable(qs, rows, mh.UNIFORM_K, space, deleted), "k = 10, all 70 queries"
    assert mh.oracle_is_stable(qs[:12], rows, mh.UNIFORM_BIG_K, space, deleted), "k = 100, 12 queries"
    masked = deleted | (mh.row_mask_for(mh.UNIFORM_N) == 0)
    assert mh.oracle_is_stable(qs[:12], rows, mh.UNIFORM_K, space, masked), "k = 10 under the row mask"


@pytest.mark.parametrize("d,space,e", mh.RANGE_CASES)
def test_uniform_range_cases_have_a_float32_radius_and_are_stable(d, space, e):
    rows, qs, deleted = mh.uniform_inputs(d, e)
    qs = qs[:mh.RANGE_NQ]
    radius = mh.range_radius(qs, rows, space, deleted)
    want = mh.oracle_range(qs, rows, radius, space, deleted)
    sizes = np.array([len(w[0]) for w in want])
    assert sizes.sum() > 0 and sizes.max() <= mh.RANGE_MAX_HITS, f"hits per query: {sizes}"
    assert mh.oracle_range_is_stable(qs, rows, radius, space, deleted)


# ---------------------------------------------------------------- 2. ladder corpora
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("layout", mh.LADDER_LAYOUTS)
@pytest.mark.parametrize("d", mh.LADDER_DIMS)
def test_ladder_cases_are_stable_through_tombstones_and_compaction(d, layout, space):
    rows, qs = mh.ladder_inputs(d, layout)
    assert rows.shape == (mh.LADDER_N, d) and qs.shape == (len(mh.LADDER), d)
    assert np.isfinite(rows).all() and np.isfinite(qs).all()
    for j, e in enumerate(mh.LADDER):  # every rung is there, in the corpus and among the queries
        assert np.abs(qs[j]).max() < 8 * 2.0 ** e and np.abs(qs[j]).max() > 2.0 ** e / 8
    assert mh.oracle_is_stable(qs, rows, mh.LADDER_K, space)
    l2 = mh.oracle_knn(qs, rows, mh.LADDER_K, "l2")[0]
    for j in range(len(mh.LADDER)):
        assert np.isin(l2[j], mh.planted_rows(j)).all(), f"rung {mh.LADDER[j]}: the l2 top 10 {l2[j]} are not the planted rows"
    nearest = mh.oracle_knn(qs, rows, 1, space)[0][:, 0]
    dead = np.zeros(mh.LADDER_N, dtype=bool)
    dead[nearest] = True
    assert mh.oracle_is_stable(qs, rows, mh.LADDER_K, space, dead), "after the tombstones"
    assert mh.oracle_is_stable(qs, rows[~dead], mh.LADDER_K, space), "after compaction"


# ---------------------------------------------------------------- 3. edge rows
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("d", mh.EDGE_DIMS)
def test_edge_row_cases_are_stable(d, space):
    rows, qs, deleted, places = mh.edge_inputs(d)
    assert rows.shape == (mh.EDGE_N, d) and mh.EDGE_N % 16 == len(mh.EDGE_KINDS), "the last panel is partial"
    assert np.isfinite(rows).all() and np.isfinite(qs).all()
    assert (places[0] < 16).all() and (places[1] >= mh.EDGE_N - len(mh.EDGE_KINDS)).all()
    assert deleted[places[2] + 1].all() and not deleted[places.ravel()].any()
    for p in places:  # the three placements hold the same bits, and those are the ones asked for
        assert np.array_equal(rows[p].view(np.uint32), rows[places[0]].view(np.uint32))
    for kind, v in enumerate(mh.EDGE_VALUES):
        assert (rows[places[0][kind]] == v).sum() == 1
    bf16_finite = np.float32(3.39e38).view(np.uint32) + np.uint32(0x8000) < np.uint32(0x7F800000)
    bf16_inf = np.float32(3.40e38).view(np.uint32) + np.uint32(0x8000) >= np.uint32(0x7F800000)
    assert bf16_finite and bf16_inf, "3.39e38 rounds to a finite bf16, 3.40e38 to inf"
    big = rows[places[0][-1]].astype(np.float64)
    assert np.sqrt((big * big).sum()) > float(mh.F32_MAX) and np.float32(np.sqrt((big * big).sum())) == np.inf
    back = qs[mh.EDGE_ORDINARY_QUERIES:mh.EDGE_ORDINARY_QUERIES + len(mh.EDGE_KINDS)]
    assert np.array_equal(back.view(np.uint32), rows[places[0]].view(np.uint32)), "each edge row is queried back"
    for k in (10, 64):
        assert mh.oracle_is_stable(qs, rows, k, space, deleted), f"k = {k}"
    if space == "l2":  # the stored FLT_MAX row queried back with radius 0: itself (three placements) and nothing else
        q = qs[mh.EDGE_ORDINARY_QUERIES:mh.EDGE_ORDINARY_QUERIES + 1]
        want = mh.oracle_range(q, rows, 0.0, "l2", deleted)
        assert want[0][0].tolist() == sorted(places[:, 0].tolist())
        assert mh.oracle_range_is_stable(q, rows, 0.0, "l2", deleted)


# ---------------------------------------------------------------- 4. odd queries on an ordinary index
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("d", mh.MIXED_DIMS)
def test_mixed_query_cases_are_stable_and_the_odd_queries_leave_every_window(d, space):
    rows, qs, deleted = mh.mixed_inputs(d)
    assert rows.shape == (mh.MIXED_N, d) and qs.shape == (mh.MIXED_ORDINARY + len(mh.MIXED_ODD), d)
    assert mh.inside_filter_window(rows, space), "the index is inside the window"
    leaving = mh.queries_leaving_window(qs, rows, space)
    assert np.nonzero(leaving)[0].tolist() == list(mh.MIXED_ODD_AT), f"queries outside the window: {np.nonzero(leaving)[0]}"
    assert (qs[mh.MIXED_ODD_AT[2]] == mh.F32_MAX).sum() == 1
    for k in mh.MIXED_KS:
        assert mh.oracle_is_stable(qs, rows, k, space, deleted), f"k = {k}"
    radius = mh.mixed_radius(d, space)
    want = mh.oracle_range(qs, rows, radius, space, deleted)
    sizes = np.array([len(w[0]) for w in want])
    ordinary = np.delete(np.arange(qs.shape[0]), mh.MIXED_ODD_AT)
    assert sizes[ordinary].sum() > 0 and sizes.max() <= mh.RANGE_MAX_HITS, f"hits per query: {sizes}"
    assert mh.oracle_range_is_stable(qs, rows, radius, space, deleted)


def test_queries_leaving_window_follows_the_uniform_cases():
    for e, space, want in ((-20, "l2", 0), (-20, "cosine", 0), (-20, "ip", 70), (-40, "ip", 70), (40, "ip", 0), (63, "ip", 0)):
        rows, qs, _ = mh.uniform_inputs(64, e)
        assert mh.inside_filter_window(rows, space) and int(mh.queries_leaving_window(qs, rows, space).sum()) == want, (e, space)
