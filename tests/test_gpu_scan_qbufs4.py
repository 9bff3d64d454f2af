"""The four-buffer int8 scan body (tools/gen_scan_asm.py, generate(..., qbufs=4); kernels_filter.hip, launch_scan_space): full
passes (more than 128 queries) of a k <= 64 kNN call over a query image of six chunks (d = 641..768) keep chunks 2 and 3 in
LDS for the whole launch and stage two chunks per tile.  Integer accumulation is exact, so every answer must stay what the
exact scan gives.  Shapes, the smallest at which the control flow differs: 300,000 rows end in a round of 917 tiles on 256
workgroups (3 and 4 tiles each: up, down, up(, down)); d = 700 is a padded shadow of still six chunks; 20,000 rows are at
most one tile per workgroup, the last one partly filled, so nothing is staged after the prologue; 129 and 200 queries run the
16-tile body with empty query columns.  The body's staging area holds 304 entries per wave instead of 992: one case makes a
single wave append 1,024 in one launch.  A k = 100 call and a range call append far more and stay on the two-buffer body."""
import numpy as np
import pytest

from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.helpers import assert_knn_matches, assert_range_matches, oracle_knn
from tests.test_gpu_scan_zigzag import d64_bound

pytestmark = pytest.mark.gpu

N_BIG, D, NQ_MAX, K = 300_000, 768, 256, 10


@pytest.fixture(scope="module")
def corpus():
    """One draw for every case (a case takes the first n rows, d columns, nq queries); never modified."""
    rng = np.random.default_rng(20261)
    rows = rng.standard_normal((N_BIG, D), dtype=np.float32)
    qs = rng.standard_normal((NQ_MAX, D), dtype=np.float32)
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs


def filter_and_exact(rows, qs, space, k):
    """(the filter path's answer, the exact scan's, the filter call's stats); the filter call is made twice and must repeat."""
    eng = HipScanEngine(rows.shape[1], space, device=0, capacity_hint=rows.shape[0], strategy="filter")
    try:
        eng.append(rows)
        got = eng.search64(qs, k)
        st = eng.last_stats()
        again = eng.search64(qs, k)   # determinism: the same call, the same arrays
        for a, b in zip(got, again):
            assert np.array_equal(a, b)
        eng.set_strategy("exact")
        want = eng.search64(qs, k)
    finally:
        eng.close()
    return got, want, st


def assert_same_as_exact(got, want, st, space, rows, qs, tag):
    assert st["strategy_used"] == 2 and st["bound_dtype"] == 2 and st["fallback_queries"] == 0, st
    (labels, dist, counts, d64), (xl, xd, xc, x64) = got, want
    assert np.array_equal(labels, xl) and np.array_equal(counts, xc), \
        f"{tag}: ids differ from the exact scan for {(labels != xl).any(axis=1).sum()} queries"
    err, bound = float(np.abs(d64 - x64).max()), d64_bound(space, rows.shape[1], rows, qs)
    print(f"{tag}: max |fp64 distance - exact scan's| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound


CASES = [
    # (space, d, rows, queries)
    ("cosine", 768, N_BIG, 256), ("l2", 768, N_BIG, 256), ("ip", 768, N_BIG, 256),
    ("cosine", 700, N_BIG, 256),
    ("cosine", 768, 20_000, 256),
    ("cosine", 768, N_BIG, 129), ("cosine", 768, N_BIG, 200),
]


@pytest.mark.parametrize("space,d,n,nq", CASES)
def test_four_buffer_scan_returns_the_exact_scan(corpus, space, d, n, nq):
    rows = np.ascontiguousarray(corpus[0][:n, :d])
    qs = np.ascontiguousarray(corpus[1][:nq, :d])
    got, want, st = filter_and_exact(rows, qs, space, K)
    tag = f"qbufs4/{space}/d{d}/n{n}/nq{nq}"
    assert_same_as_exact(got, want, st, space, rows, qs, tag)
    assert_knn_matches((got[0][:8], got[1][:8], got[2][:8]), oracle_knn(qs[:8], rows, K, space), tag)


def test_a_wave_that_appends_more_than_its_staging_area(corpus):
    """Every query is one common unit vector plus N(0, 0.05^2) noise per component (cosine to that vector ~0.58; to a random
    row at most ~0.2), and four consecutive rows of one wave's 32-row slab in the last round are scaled copies of the vector:
    every query admits all four, so that wave appends 4 x 256 = 1,024 entries in one launch -- 304 of them fit its LDS area,
    the rest take the global path of the append routine, inside its 2,048-entry buffer."""
    rng = np.random.default_rng(20262)
    v = rng.standard_normal(D)
    v = (v / np.linalg.norm(v)).astype(np.float32)
    qs = (v[None, :] + rng.normal(0.0, 0.05, (NQ_MAX, D))).astype(np.float32)
    first = 200_000                      # past the first round (65,280 rows); 200,000 = 781 x 256 + 2 x 32: wave 2 of tile 781
    assert first >= 65_280 and first % 32 == 0
    planted = np.arange(first, first + 4)
    rows = np.array(corpus[0])
    rows[planted] = v[None, :] * np.array([1.0, 2.0, 0.5, 4.0], dtype=np.float32)[:, None]
    got, want, st = filter_and_exact(rows, qs, "cosine", K)
    assert_same_as_exact(got, want, st, "cosine", rows, qs, "qbufs4/staging-area")
    assert (np.sort(got[0][:, :4], axis=1) == planted[None, :]).all(), "the four planted rows are every query's top four"


def test_big_k_and_range_calls_keep_their_answers(corpus):
    """k = 100 (a big-k pass) and a range call on the same index: their scans append per wave far more than the four-buffer
    body's staging area holds, the dispatch leaves them on the two-buffer body (only run_filter_pass sets the flag), and
    they agree with the exact scan / the oracle as before."""
    rows, qs = corpus[0], np.ascontiguousarray(corpus[1][:129])
    eng = HipScanEngine(D, "cosine", device=0, capacity_hint=N_BIG, strategy="filter")
    try:
        eng.append(rows)
        got = eng.search64(qs, 100)
        st = eng.last_stats()
        eng.set_strategy("exact")
        want = eng.search64(qs, 100)
        eng.set_strategy("filter")
        radius = float(np.median(want[3][:, 29]))        # about 30 hits per query
        hits = eng.range(qs, radius, 64)
        st_range = eng.last_stats()
        eng.set_strategy("exact")
        exact_hits = eng.range(qs, radius, 64)
    finally:
        eng.close()
    assert st["strategy_used"] == 2 and st["fallback_queries"] == 0, st
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    err, bound = float(np.abs(got[3] - want[3]).max()), d64_bound("cosine", D, rows, qs)
    print(f"qbufs4/k100: max |fp64 distance - exact scan's| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert st_range["strategy_used"] == 2 and st_range["fallback_queries"] == 0, st_range
    # every query against the exact scan's range call, the first 16 against the NumPy oracle as well (its fp64 matrix of all
    # 129 x 300,000 pairs would take longer than the rest of this file)
    assert_range_matches(hits, [exact_hits[i] for i in range(len(qs))], "qbufs4/range/exact-scan")
    assert sum(len(exact_hits[i][0]) for i in range(len(qs))) >= 10 * len(qs)
    assert_range_matches([hits[i] for i in range(16)], exact_scan.range_query(qs[:16], rows, radius, "cosine"), "qbufs4/range/oracle")
