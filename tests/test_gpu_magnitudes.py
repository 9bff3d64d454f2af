"""kNN, range and pair distances across the whole finite float32 range, through HipScanEngine (the C ABI: the Python Index,
which refuses NaN/inf, is not involved).  The contract (DESIGN, "Magnitudes"): every finite float32 row and query is answered
with the oracle's ids.

The reference is oracle.exact_scan (fp64) alone; tests/test_magnitudes_host.py holds every case used here to its
preconditions on the CPU.  Rows go in in two appends.  Which route served a call is recorded, not guessed: every call's
strategy_used / bound_dtype / fallback_queries goes to the file MLVDB_ROUTE_LOG names (JSON lines, when it is set), and a
forced-filter call on an index inside the filter path's magnitude window must still report the filter route (record).  A
call the library serves by its exact scan or fallback passes as long as the answer is the oracle's.
"""
import numpy as np
import pytest

from tests import magnitude_helpers as mh
from tests.helpers import assert_range_matches

pytestmark = pytest.mark.gpu

STRATEGIES = ("exact", "filter")
open_engine, record = mh.open_engine, mh.record  # (shared with tests/test_gpu_magnitudes_families.py)


# ---------------------------------------------------------------- 1. uniform scale
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("e", mh.UNIFORM_EXPONENTS)
@pytest.mark.parametrize("d", mh.UNIFORM_DIMS)
def test_uniform_scale(d, e, space):
    """A whole corpus (3000 rows, 5 % tombstoned) and its queries in units of 2**e.  d = 64: the bf16 body; 100: the zero-padded
    int8 shadow; 256: the int8-only index and the small-batch chain.  2, 12 and 70 queries (the 1-2-query chain, the narrow
    kernel, a pass of 8 query tiles) at k = 10, 12 queries at k = 100 (a big-k pass on the mid shadow) and under a row mask."""
    rows, qs, deleted = mh.uniform_inputs(d, e)
    n = rows.shape[0]
    want10 = mh.oracle_knn(qs, rows, mh.UNIFORM_K, space, deleted)
    want100 = mh.oracle_knn(qs[:12], rows, mh.UNIFORM_BIG_K, space, deleted)
    mask = mh.row_mask_for(n)
    want_masked = mh.oracle_knn(qs[:12], rows, mh.UNIFORM_K, space, deleted | (mask == 0))
    for strategy in STRATEGIES:
        tag = f"uniform/{space}/d{d}/e{e}/{strategy}"
        eng = open_engine(rows, space, strategy, deleted)
        try:
            for nq in mh.UNIFORM_BATCHES:
                got = eng.search(qs[:nq], mh.UNIFORM_K)
                record(eng, f"{tag}/nq{nq}", rows, strategy, qs[:nq])
                mh.assert_knn_matches_rel(got, tuple(w[:nq] for w in want10), f"{tag}/nq{nq}")
            got = eng.search(qs[:12], mh.UNIFORM_BIG_K)
            record(eng, f"{tag}/k100", rows, strategy, qs[:12])
            mh.assert_knn_matches_rel(got, want100, f"{tag}/k100")
            got = eng.search(qs[:12], mh.UNIFORM_K, mask=mask)
            record(eng, f"{tag}/masked", rows, strategy, qs[:12])
            mh.assert_knn_matches_rel(got, want_masked, f"{tag}/masked")
        finally:
            eng.close()


# ---------------------------------------------------------------- 2. ladder corpora
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("layout", mh.LADDER_LAYOUTS)
@pytest.mark.parametrize("d", mh.LADDER_DIMS)
def test_ladder_corpora(d, layout, space):
    """Rows from 2**-140 to 2**124 in one index, a query and twelve planted neighbours per rung; then the nearest row of every
    query tombstoned; then compacted (the oracle on rows[old])."""
    rows, qs = mh.ladder_inputs(d, layout)
    k = mh.LADDER_K
    want = mh.oracle_knn(qs, rows, k, space)
    dead = np.zeros(rows.shape[0], dtype=bool)
    dead[want[0][:, 0]] = True
    want_dead = mh.oracle_knn(qs, rows, k, space, dead)
    want_compact = mh.oracle_knn(qs, rows[~dead], k, space)
    for strategy in STRATEGIES:
        tag = f"ladder/{layout}/{space}/d{d}/{strategy}"
        eng = open_engine(rows, space, strategy)
        try:
            got = eng.search(qs, k)
            record(eng, f"{tag}/built", rows, strategy)
            mh.assert_knn_matches_rel(got, want, f"{tag}/built")
            assert eng.tombstone(np.nonzero(dead)[0]) == int(dead.sum())
            got = eng.search(qs, k)
            record(eng, f"{tag}/tombstoned", rows, strategy)
            mh.assert_knn_matches_rel(got, want_dead, f"{tag}/tombstoned")
            old = eng.compact()
            assert np.array_equal(old, np.nonzero(~dead)[0]), f"{tag}: compact() kept other rows than the live ones"
            got = eng.search(qs, k)
            record(eng, f"{tag}/compacted", rows, strategy)
            mh.assert_knn_matches_rel(got, want_compact, f"{tag}/compacted")
        finally:
            eng.close()


# ---------------------------------------------------------------- 3. edge rows
@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("d", mh.EDGE_DIMS)
def test_edge_rows(d, space, strategy):
    """Single components at +-FLT_MAX, on both sides of bf16's overflow point and at the smallest subnormal and normal, and
    a row whose norm is no float32, in the first panel, in the last, partial one and beside tombstones: all of them stay
    live rows (counts), come back bit for bit (get_rows), and every query gets the oracle's ids at k = 10 and k = 64."""
    rows, qs, deleted, places = mh.edge_inputs(d)
    n = rows.shape[0]
    tag = f"edge/{space}/d{d}/{strategy}"
    eng = open_engine(rows, space, strategy, deleted)
    try:
        for k in (10, 64):
            got = eng.search(qs, k)
            record(eng, f"{tag}/k{k}", rows, strategy)
            mh.assert_knn_matches_rel(got, mh.oracle_knn(qs, rows, k, space, deleted), f"{tag}/k{k}")
        assert eng.counts() == (n, int(deleted.sum())), f"{tag}: counts() {eng.counts()}: an edge row is not a live row"
        assert np.array_equal(eng.get_rows(0, n).view(np.uint32), rows.view(np.uint32)), f"{tag}: get_rows() changed bits"
    finally:
        eng.close()


# ---------------------------------------------------------------- 4. the fp64 faces
def fp64_corpora():
    for d in (64, 256):
        yield f"ladder-blocks/d{d}", mh.ladder_inputs(d, "blocks") + (None,)
        yield f"edge/d{d}", mh.edge_inputs(d)[:3]


@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("corpus", ["ladder-blocks/d64", "ladder-blocks/d256", "edge/d64", "edge/d256"])
def test_fp64_faces(corpus, space):
    """mlvdb_pair_distances over the oracle's top 10 of every query, label -1 and a tombstoned label, and the out_dist64 of
    mlvdb_search_batch_device: within 1e-12 of the oracle's fp64 distance in units of the summed terms, finite for finite
    inputs whatever the fp32 face overflows to, and the fp32 face float32(fp64 face) to within 1 ulp."""
    import torch

    rows, qs, deleted = dict(fp64_corpora())[corpus]
    n, nq, k = rows.shape[0], qs.shape[0], 10
    if deleted is None:
        deleted = np.zeros(n, dtype=bool)
        deleted[mh.planted_rows(3)[0]] = True
    want = mh.oracle_knn(qs, rows, k, space, deleted)
    assert (want[0] >= 0).all()
    labels = np.concatenate([want[0], np.full((nq, 1), -1), np.full((nq, 1), np.nonzero(deleted)[0][0])], axis=1)
    tag = f"fp64/{corpus}/{space}"
    eng = open_engine(rows, space, "filter", deleted)
    try:
        d64, d32 = eng.pair_distances(qs, labels)
        mh.assert_fp64_matches(d64, d32, qs, rows, labels, space, f"{tag}/pairs")
        t_q = torch.from_numpy(qs.copy()).cuda()
        lab = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
        o64 = torch.empty((nq, k), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        eng.search_device(t_q.data_ptr(), nq, k, lab.data_ptr(), dist.data_ptr(), cnt.data_ptr(), o64.data_ptr(), stream)
        torch.cuda.synchronize()
        record(eng, f"{tag}/filter/device", rows, "filter")
        got = (lab.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy())
        mh.assert_knn_matches_rel(got, want, f"{tag}/device")
        mh.assert_fp64_matches(o64.cpu().numpy(), got[1], qs, rows, got[0], space, f"{tag}/device")
    finally:
        eng.close()


# ---------------------------------------------------------------- 5. range
@pytest.mark.parametrize("d,space,e", mh.RANGE_CASES)
def test_uniform_scale_through_range(d, space, e):
    """Range search on the uniform corpora wherever a radius is a float32: cosine at every scale, l2 from 2**-70 (the radius is
    a subnormal) to 2**60, ip at 2**+-20.  The radius is fp32 of the oracle's mean 10th-nearest distance."""
    rows, qs, deleted = mh.uniform_inputs(d, e)
    qs = qs[:mh.RANGE_NQ]
    radius = mh.range_radius(qs, rows, space, deleted)
    want = mh.oracle_range(qs, rows, radius, space, deleted)
    for strategy in STRATEGIES:
        tag = f"range/{space}/d{d}/e{e}/{strategy}/r{radius!r}"
        eng = open_engine(rows, space, strategy, deleted)
        try:
            got = eng.range(qs, radius, 64)
            record(eng, tag, rows, strategy, qs)
        finally:
            eng.close()
        assert_range_matches(got, want, tag)


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("d", mh.EDGE_DIMS)
def test_the_flt_max_row_queried_back_with_radius_zero(d, strategy):
    """l2 on the edge-row corpus: the stored FLT_MAX row as the query, radius 0 -- itself (its three placements, by label) at
    distance 0 and nothing else."""
    rows, qs, deleted, places = mh.edge_inputs(d)
    q = qs[mh.EDGE_ORDINARY_QUERIES:mh.EDGE_ORDINARY_QUERIES + 1]
    assert np.array_equal(q[0], rows[places[0, 0]]) and (q[0] == mh.F32_MAX).sum() == 1
    want = mh.oracle_range(q, rows, 0.0, "l2", deleted)
    tag = f"range/edge/l2/d{d}/{strategy}/r0"
    eng = open_engine(rows, "l2", strategy, deleted)
    try:
        got = eng.range(q, 0.0, 64)
        record(eng, tag, rows, strategy)
    finally:
        eng.close()
    assert_range_matches(got, want, tag)
    assert got[0][0].tolist() == sorted(places[:, 0].tolist()) and not got[0][1].any()


# ---------------------------------------------------------------- 6. odd queries on an ordinary index
@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("d", mh.MIXED_DIMS)
def test_odd_queries_share_a_pass_with_ordinary_ones(d, space, strategy):
    """An N(0,1) index inside every window; a batch of eight ordinary queries and three outside the window (x 2**-140, x 2**120,
    a FLT_MAX component), which the fused prep flags for the exact fallback while the ordinary ones go through the filter with
    them -- the per-pass state (common l2 step, smallest query scale, largest query error) is shared.  Then the odd queries
    alone, one and two at a time (the 1-2-query chain).  kNN at k = 10 and k = 100 and range, every answer the oracle's; on
    the forced filter strategy the route stays the filter's and the fallbacks cover at least the odd queries (record)."""
    rows, qs, deleted = mh.mixed_inputs(d)
    radius = mh.mixed_radius(d, space)
    odd = np.array(mh.MIXED_ODD_AT)
    batches = [("all", np.arange(qs.shape[0]))] + [("odd" + "".join(map(str, sel)), odd[list(sel)]) for sel in mh.MIXED_ODD_ONLY]
    want_knn = {k: mh.oracle_knn(qs, rows, k, space, deleted) for k in mh.MIXED_KS}
    want_range = mh.oracle_range(qs, rows, radius, space, deleted)
    eng = open_engine(rows, space, strategy, deleted)
    try:
        for name, idx in batches:
            q = np.ascontiguousarray(qs[idx])
            for k in mh.MIXED_KS:
                tag = f"mixed/{space}/d{d}/{strategy}/{name}/k{k}"
                got = eng.search(q, k)
                record(eng, tag, rows, strategy, q)
                mh.assert_knn_matches_rel(got, tuple(w[idx] for w in want_knn[k]), tag)
            tag = f"mixed/{space}/d{d}/{strategy}/{name}/range"
            got = eng.range(q, radius, 64)
            record(eng, tag, rows, strategy, q)
            assert_range_matches(got, [want_range[i] for i in idx], tag)
    finally:
        eng.close()


# ---------------------------------------------------------------- 7. compaction narrows the norm range again
@pytest.mark.parametrize("space", mh.SPACES)
def test_a_row_outside_the_window_leaves_with_compaction(space):
    """One row x 2**121 (outside every window) in an N(0,1) index sends the forced filter strategy to the exact scans, still
    does once tombstoned (its bits are in the shadows' panels), and no longer after compact(): the norm range is rebuilt from
    the rows that stay.  The oracle's ids at every step."""
    rows, qs, _ = mh.mixed_inputs(64)
    rows = rows.copy()
    qs = qs[np.delete(np.arange(qs.shape[0]), mh.MIXED_ODD_AT)]
    big = 1234
    rows[big] *= mh.pow2(121)
    assert np.isfinite(rows).all() and not mh.inside_filter_window(rows, space)
    dead = np.zeros(rows.shape[0], dtype=bool)
    dead[big] = True
    assert mh.inside_filter_window(rows[~dead], space)
    k = 10
    eng = open_engine(rows, space, "filter")
    try:
        got = eng.search(qs, k)
        assert eng.last_stats()["strategy_used"] == 1, "a row outside the window: the exact scans serve the index"
        mh.assert_knn_matches_rel(got, mh.oracle_knn(qs, rows, k, space), f"compaction/{space}/built")
        assert eng.tombstone(np.array([big])) == 1
        got = eng.search(qs, k)
        assert eng.last_stats()["strategy_used"] == 1
        mh.assert_knn_matches_rel(got, mh.oracle_knn(qs, rows, k, space, dead), f"compaction/{space}/tombstoned")
        assert np.array_equal(eng.compact(), np.nonzero(~dead)[0])
        got = eng.search(qs, k)
        record(eng, f"compaction/{space}/filter/compacted", rows[~dead], "filter", qs)
        mh.assert_knn_matches_rel(got, mh.oracle_knn(qs, rows[~dead], k, space), f"compaction/{space}/compacted")
        eng.append(rows[big:big + 1])  # and an append after it widens the range again
        got = eng.search(qs, k)
        assert eng.last_stats()["strategy_used"] == 1
        mh.assert_knn_matches_rel(got, mh.oracle_knn(qs, np.concatenate([rows[~dead], rows[big:big + 1]]), k, space),
                                  f"compaction/{space}/appended")
    finally:
        eng.close()
