"""The int8 scan walks the k-chunks of the query image zig-zag (tools/gen_scan_asm.py, q_schedule): upwards in a workgroup's
even tiles, downwards in its odd ones.  Integer accumulation is exact, so every answer must stay what the exact scan gives.
The shapes are the smallest at which the control flow differs: 300,000 rows end in a round of 917 tiles on 256 workgroups
(3 and 4 tiles each: up, down, up(, down)) after one of 240 tiles (one tile or none); d = 256 / 512 / 768 / 1024 are 2 (the
single body, image fully resident), 4 (no middle body), 6 and 8 (middle body twice) chunks; d = 300 is a padded shadow;
20,000 rows are a partly filled last tile with at most one tile per workgroup; batches of 40 / 100 / 256 run the bodies of 4 /
8 / 16 query tiles; l2 adds the offsets that enter through the first executed k-step's C operand."""
import numpy as np
import pytest

from mlvectordb_amd.engine import HipScanEngine
from tests.helpers import assert_knn_matches, oracle_knn

pytestmark = pytest.mark.gpu

N_BIG, D_MAX, NQ_MAX, K = 300_000, 1024, 256, 10


@pytest.fixture(scope="module")
def corpus():
    """One draw for every case (a case takes the first n rows, d columns, nq queries); never modified."""
    rng = np.random.default_rng(20260)
    rows = rng.standard_normal((N_BIG, D_MAX), dtype=np.float32)
    qs = rng.standard_normal((NQ_MAX, D_MAX), dtype=np.float32)
    rows.setflags(write=False)
    qs.setflags(write=False)
    return rows, qs


def d64_bound(space, d, rows, qs):
    """Two fp64 evaluations of one distance differ by the order of a d-term sum of exact products: at most d 2^-53 times the sum of
    the terms' magnitudes (<= |q| |x| by Cauchy-Schwarz; l2: <= (|q| + |x|)^2), twice for the two sides, and as much again for
    the norms, the square roots and the division of cosine."""
    qn = float(np.linalg.norm(qs.astype(np.float64), axis=1).max())
    xn = float(np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1).max()))
    scale = {"cosine": 1.0, "ip": qn * xn, "l2": (qn + xn) ** 2}[space]
    return 4.0 * d * 2.0 ** -53 * scale


CASES = [
    # (space, d, rows, queries)
    ("cosine", 256, N_BIG, 256), ("cosine", 512, N_BIG, 256), ("cosine", 768, N_BIG, 256), ("cosine", 1024, N_BIG, 256),
    ("l2", 512, N_BIG, 256), ("l2", 768, N_BIG, 256), ("ip", 768, N_BIG, 256),
    ("cosine", 768, N_BIG, 40), ("cosine", 768, N_BIG, 100),
    ("cosine", 300, N_BIG, 256),
    ("cosine", 768, 20_000, 256),
]


@pytest.mark.parametrize("space,d,n,nq", CASES)
def test_zigzag_scan_returns_the_exact_scan(corpus, space, d, n, nq):
    rows = np.ascontiguousarray(corpus[0][:n, :d])
    qs = np.ascontiguousarray(corpus[1][:nq, :d])
    eng = HipScanEngine(d, space, device=0, capacity_hint=n, strategy="filter")
    try:
        eng.append(rows)
        labels, dist, counts, d64 = eng.search64(qs, K)
        st = eng.last_stats()
        assert st["strategy_used"] == 2 and st["bound_dtype"] == 2 and st["fallback_queries"] == 0, st
        again = eng.search64(qs, K)   # determinism: the same call, the same arrays
        for a, b in zip((labels, dist, counts, d64), again):
            assert np.array_equal(a, b)
        eng.set_strategy("exact")
        xl, xd, xc, x64 = eng.search64(qs, K)
    finally:
        eng.close()
    assert np.array_equal(labels, xl) and np.array_equal(counts, xc), f"ids differ from the exact scan for {(labels != xl).any(axis=1).sum()} queries"
    err, bound = float(np.abs(d64 - x64).max()), d64_bound(space, d, rows, qs)
    print(f"{space} d{d} n{n} nq{nq}: max |fp64 distance - exact scan's| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert_knn_matches((labels[:8], dist[:8], counts[:8]), oracle_knn(qs[:8], rows, K, space), f"zigzag/{space}/d{d}/n{n}/nq{nq}")
