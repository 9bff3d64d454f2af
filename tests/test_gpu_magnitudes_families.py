"""The search families built on kNN, range and pair distances -- per-query filters, distinct, grouped, MMR, search by
examples, late interaction, hybrid, sparse -- across the whole finite float32 range, through HipScanEngine (the C ABI).  The
contract (DESIGN, "Magnitudes"): every finite float32 row and query is answered with the model's ids.

One test id is one cell: family / corpus / d / space / strategy (magnitude_helpers.family_cells, the list
tests/test_magnitudes_families_host.py holds to its preconditions on the CPU).  A cell asserts
1. ids: labels, counts, groups, group counts, pick ranks, match labels and list ranks equal the model's (tests/*_helpers.py,
   NumPy fp64) for every query the host file does not leave out (none but on ``edge``); padding is label -1 / INT64_MIN,
   never "not finite";
2. fp64 distances within magnitude_helpers.family_fp64_bar of the oracle's, finite for finite inputs, the fp32 face their
   rounding;
3. the bit contracts, for every query: distances are ``pair_distances`` of the same handle, MMR is the greedy replayed on the
   device's own candidates, a late-interaction score the sequential sum of its match distances, a fused score
   ``hybrid_helpers.fuse_lists`` on the device's own components;
4. routes: magnitude_helpers.record after every family call.

Engines are shared between the cells of one (corpus, d, space, strategy): one is open at a time.
"""
import time

import numpy as np
import pytest

from mlvectordb_amd import _native
from tests import magnitude_helpers as mh
from tests.distinct_helpers import ABSENT
from tests.grouped_helpers import check_grouped
from tests.helpers import assert_range_matches
from tests.hybrid_helpers import fuse_lists
from tests.like_helpers import cosine_query_bound, example_sets, like_queries, like_strip, most_examples
from tests.maxsim_helpers import check_maxsim
from tests.mmr_helpers import mmr_from_candidates
from tests.sparse_helpers import SparseOracleEngine, dense_scores, rank, sparse_csr

pytestmark = pytest.mark.gpu

CELLS = sorted(((f, c, d, s, st) for f, c, d, s in mh.family_cells() for st in mh.FAMILY_STRATEGIES),
               key=lambda x: (x[1], x[2], x[3], x[4], mh.FAMILIES.index(x[0])))  # the cells of one engine stand together
DISTINCT_OVERSAMPLE_DEFAULT = 4
bits = mh.bits


def cell_id(cell):
    f, c, d, s, st = cell
    return f"{f}/{c}/d{d}/{s}/{st}"


@pytest.fixture(scope="module")
def engines():
    """engines(corpus, d, space, strategy) -> the filled engine of that key; the one before it is closed."""
    state = {"key": None, "eng": None}

    def get(corpus, d, space, strategy):
        key = (corpus, d, space, strategy)
        if state["key"] != key:
            if state["eng"] is not None:
                state["eng"].close()
            state["key"] = state["eng"] = None
            c = mh.family_case(corpus, d)
            eng = mh.open_engine(c.rows, space, strategy, c.deleted)
            try:
                mh.fill_engine(eng, c)
                eng.last_stats()
            except Exception:
                eng.close()
                raise
            state["key"], state["eng"] = key, eng
        return state["eng"]

    yield get
    if state["eng"] is not None:
        state["eng"].close()


def served_by(family, variant, strategy):
    """The strategy ``record`` holds the call to: late interaction and distinct's grouped scan (DISTINCT_OVERSAMPLE = 0) are
    exact scans of their own whatever is forced (they report the exact route); every other family ends in the plain device
    search, which follows the forced strategy."""
    return "exact" if family == "maxsim" or (family == "distinct" and variant == "scan") else strategy


def routed_queries(family, variant, c, got):
    """The queries whose window decides ``fallback_queries`` of the call just made (None: the call has no filter pass)."""
    if family in ("each", "range_each"):  # the gathered program's queries are walked exactly: no filter pass, no fallback
        return c.qs[c.program_of_query != mh.GATHERED_PROGRAM]
    if family == "like":
        return got[4]
    if served_by(family, variant, "filter") == "exact":
        return None
    return c.qs


def assert_pair_bits(eng, qs, lab, d64, d32, tag):
    nq = qs.shape[0]
    p64, p32 = eng.pair_distances(qs, np.asarray(lab).reshape(nq, -1))
    assert np.array_equal(bits(p64), bits(np.asarray(d64).reshape(nq, -1))), f"{tag}: fp64 differs from pair_distances"
    if d32 is not None:
        assert np.array_equal(bits(p32), bits(np.asarray(d32).reshape(nq, -1))), f"{tag}: fp32 differs from pair_distances"


# ---------------------------------------------------------------- what each family's answer is held to beyond its ids
def check_each(eng, c, space, variant, got, want, excluded, tag):
    lab, d32, cnt, d64, routes = got
    assert np.isposinf(d32[lab < 0]).all() and ((lab >= 0).sum(axis=1) == cnt).all(), f"{tag}: padding is not the tail"
    mh.assert_family_fp64(d64, d32, c.qs, c.rows, lab, space, tag)
    assert_pair_bits(eng, c.qs, lab, d64, d32, tag)
    print(f"{tag}: routes {[_native.ROUTE_NAMES[int(r)] for r in routes]}")
    if c.corpus == "mixed":  # both routes served a query, the odd ones among them (the host file: which program is which)
        assert [int(r) for r in routes] == [_native.ROUTE_SCAN, _native.ROUTE_SCAN, _native.ROUTE_GATHER], f"{tag}: {routes}"


def check_range_each(eng, c, space, variant, got, want, excluded, tag):
    hits, routes = got
    radius = mh.family_radius(c, space)
    keep = [i for i in range(c.nq) if i not in excluded]
    assert_range_matches([hits[i] for i in keep], [want[0][i] for i in keep], tag)
    for i in range(c.nq):
        lab, d32 = np.asarray(hits[i][0]), np.asarray(hits[i][1])
        assert (lab >= 0).all() and (d32 <= np.float32(radius)).all() and np.unique(lab).size == lab.size, f"{tag}: query {i}"
        if lab.size:
            p64, p32 = eng.pair_distances(c.qs[i:i + 1], lab[None, :])
            assert np.array_equal(bits(p32[0]), bits(d32)), f"{tag}: query {i}: fp32 differs from pair_distances"
            assert np.array_equal(np.lexsort((lab, p64[0])), np.arange(lab.size)), f"{tag}: query {i}: not nearest first"
    print(f"{tag}: routes {[_native.ROUTE_NAMES[int(r)] for r in routes]}")
    if c.corpus == "mixed":
        assert int(routes[mh.GATHERED_PROGRAM]) == _native.ROUTE_GATHER and int(routes[0]) == _native.ROUTE_SCAN, f"{tag}: {routes}"


def check_distinct(eng, c, space, variant, got, want, excluded, tag):
    lab, d32, cnt, d64, grp = got
    pad = lab < 0
    assert np.isposinf(d32[pad]).all() and (grp[pad] == ABSENT).all() and ((~pad).sum(axis=1) == cnt).all(), f"{tag}: padding"
    assert np.array_equal(grp[~pad], c.group[lab[~pad]]) and (grp[~pad] != ABSENT).all(), f"{tag}: a group is not its row's"
    mh.assert_family_fp64(d64, d32, c.qs, c.rows, lab, space, tag)
    assert_pair_bits(eng, c.qs, lab, d64, d32, tag)


def check_grouped_cell(eng, c, space, variant, got, want, excluded, tag):
    wl, _, wc, wgc, wd, wg = want
    check_grouped(eng, c.qs, mh.GROUPED_K, mh.GROUPED_SIZE, got, (wl, wd, wc, wgc, wg), tag, magnitudes=(c.rows, space, excluded))
    mh.assert_fp32_face(got[4], got[1], tag)


def check_mmr(eng, c, space, variant, got, want, excluded, tag):
    fetch, lam = int(variant.split("/")[0][1:]), float(variant.split("lam")[1])
    lab, d32, cnt, d64, rank_, obj = got
    assert np.isposinf(d32[lab < 0]).all() and (rank_[lab < 0] == -1).all() and ((lab >= 0).sum(axis=1) == cnt).all(), tag
    mh.assert_family_fp64(d64, d32, c.qs, c.rows, lab, space, tag)
    cl, cd32, cc, cd64 = eng.search64(c.qs, fetch)
    P = {}
    for i in range(c.nq):
        cands = cl[i, :cc[i]]
        if cands.size:
            P[i] = eng.pair_distances(eng.get_rows_at(cands), np.broadcast_to(cands, (cands.size, cands.size)))[0]
    replay, _ = mmr_from_candidates(cl, cd32, cc, cd64, lambda i, _: P[i], mh.MMR_K, lam)
    for name, g, w in zip(("labels", "dist", "counts", "dist64", "rank", "objective"), got, replay):
        assert np.array_equal(bits(g), bits(w)), f"{tag}: {name} differs from the greedy replayed on the device's own bits"


def check_like(eng, c, space, variant, got, want, excluded, tag):
    lab, d32, cnt, d64, qs = got
    w = tuple(float(x) for x in variant.split("/")[0][1:].split(","))
    weights = np.tile(np.array(w, dtype=np.float64), c.nq)
    base = c.qs if variant.endswith("/base") else None
    with np.errstate(over="ignore"):
        model_qs, scale = like_queries(c.rows, c.like_labels, weights, c.like_offsets, space, base)
    assert qs.dtype == np.float32 and np.isfinite(qs).all(), f"{tag}: a synthesised query is not finite"
    if space != "cosine":
        assert np.array_equal(bits(qs), bits(model_qs)), f"{tag}: the synthesised queries differ from like_queries"
        mh.assert_family_ids("like", c, got, want, excluded, tag)
    else:
        # like_helpers.cosine_query_bound is in units of the query's own terms (one float32 spacing of the component +
        # 1e-12 of the summed |terms|): it scales with the case.  The ids are then the model's for the device's queries.
        err = np.abs(qs.astype(np.float64) - model_qs.astype(np.float64))
        bound = cosine_query_bound(model_qs, scale)
        assert (err <= bound).all(), f"{tag}: a synthesised component is {float((err / bound).max()):.3f} bounds off"
        most = most_examples(c.like_labels, c.like_offsets)
        ol, od, oc = mh.oracle_knn(qs, c.rows, mh.LIKE_K + most, space, c.deleted)
        ref = like_strip(ol, od, oc, np.zeros(ol.shape), example_sets(c.like_labels, c.like_offsets), mh.LIKE_K)
        mh.assert_family_ids("like", c, got, (ref[0], None, ref[2]), excluded, tag)
    assert np.isposinf(d32[lab < 0]).all() and ((lab >= 0).sum(axis=1) == cnt).all(), f"{tag}: padding is not the tail"
    mh.assert_family_fp64(d64, d32, qs, c.rows, lab, space, tag)
    most = most_examples(c.like_labels, c.like_offsets)
    plain = like_strip(*eng.search64(qs, mh.LIKE_K + most), example_sets(c.like_labels, c.like_offsets), mh.LIKE_K)
    for name, g, p in zip(("labels", "dist", "counts", "dist64"), got, plain):
        assert np.array_equal(bits(g), bits(p)), f"{tag}: {name} differs from the plain search of the returned queries"


def check_maxsim_cell(eng, c, space, variant, got, want, excluded, tag):
    wg, _, wc, ws, wml, wmd = want
    toks = np.ascontiguousarray(c.qs[c.token_of])
    check_maxsim(eng, toks, c.token_offsets, mh.MAXSIM_K, got, (wg, ws, wc, wml, wmd), tag, magnitudes=(c.rows, space, excluded))


def check_hybrid(eng, c, space, variant, got, want, excluded, tag):
    lab, fused, cnt, d64, s64, rd, rs = got
    k, fetch = mh.HYBRID_K, mh.HYBRID_FETCH
    pad = lab < 0
    assert np.isposinf(d64[pad]).all() and np.isneginf(fused[pad]).all() and ((~pad).sum(axis=1) == cnt).all(), f"{tag}: padding"
    assert np.isfinite(fused[~pad]).all() and np.isfinite(s64[~pad]).all(), f"{tag}: a score of finite inputs is not finite"
    mh.assert_family_fp64(d64, None, c.qs, c.rows, lab, space, tag)
    assert_pair_bits(eng, c.qs, lab, d64, None, tag)
    scores, mass = dense_scores(mh.sparse_queries(c.nq), c.sparse_list)
    safe = np.where(pad, 0, lab)
    err = np.abs(s64 - np.take_along_axis(scores, safe, axis=1))
    assert (err[~pad] <= mh.SPARSE_EPS * np.take_along_axis(mass, safe, axis=1)[~pad]).all(), f"{tag}: a sparse component is off"
    # the fusion on the device's own bits: its two lists, and every component of the union from a call with k = the union
    dl, _, dc, dd64 = eng.search64(c.qs, fetch)
    sl, _, sc, ss64 = eng.search_batch_sparse(mh.SPARSE, c.sparse_queries, fetch)
    full = eng.search_hybrid(c.qs, mh.SPARSE, c.sparse_queries, 2 * fetch, fetch, fetch, method=variant, components=True)
    at = {(i, int(l)): j for i in range(c.nq) for j, l in enumerate(full[0][i, :full[2][i]])}
    replay = fuse_lists(dl, dd64, dc, sl, ss64, sc, lambda i, ls: np.array([full[3][i, at[i, int(l)]] for l in ls]),
                        lambda i, ls: np.array([full[4][i, at[i, int(l)]] for l in ls]), k, variant, (1.0, 1.0), 60.0)
    for name, g, w in zip(("labels", "fused", "counts", "dist64", "sparse64", "rank_dense", "rank_sparse"), got, replay):
        assert np.array_equal(bits(g), bits(w)), f"{tag}: {name} differs from the fusion of the device's own components"


CHECKS = {"each": check_each, "range_each": check_range_each, "distinct": check_distinct, "grouped": check_grouped_cell,
          "mmr": check_mmr, "like": check_like, "maxsim": check_maxsim_cell, "hybrid": check_hybrid}


@pytest.mark.parametrize("family,corpus,d,space,strategy", CELLS, ids=[cell_id(c) for c in CELLS])
def test_family_cell(engines, family, corpus, d, space, strategy):
    c = mh.family_case(corpus, d)
    want = mh.family_expected(family, corpus, d, space)
    excluded = mh.family_excluded(family, corpus, d, space)
    eng = engines(corpus, d, space, strategy)
    for variant, tuning, call in mh.family_variants(family, c, space):
        tag = f"{family}/{corpus}/d{d}/{space}/{strategy}/{variant}"
        t0 = time.perf_counter()
        if tuning:
            eng.set_tuning(**tuning)
        try:
            eng.last_stats()  # (the statistics accumulate until they are read: the checks of the cell before searched too)
            got = call(eng)
            mh.record(eng, tag, c.rows, served_by(family, variant, strategy), routed_queries(family, variant, c, got))
        finally:
            if tuning:
                eng.set_tuning(DISTINCT_OVERSAMPLE=DISTINCT_OVERSAMPLE_DEFAULT)
        if not (family == "like" and space == "cosine"):  # (check_like: the ids of the device's own cosine queries)
            mh.assert_family_ids(family, c, got, want[variant], excluded[variant], tag)
        with np.errstate(over="ignore"):
            CHECKS[family](eng, c, space, variant, got, want[variant], excluded[variant], tag)
        print(f"{tag}: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------- the device route every family stands on
@pytest.mark.parametrize("strategy", mh.FAMILY_STRATEGIES)
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("d", (64, 256))
def test_the_device_route_with_odd_queries(engines, d, space, strategy):
    """mlvdb_search_batch_device (no deferred fallback: the overflow decision stays on the device) on ``mixed``: eight
    ordinary queries and three outside every window in one pass, at k = 10 and 64 (the filter pass), 100 and 1024 (the big-k
    passes; the paged exact scan under the exact strategy), labels, fp32 and fp64 left in torch buffers."""
    import torch

    c = mh.family_case("mixed", d)
    eng = engines("mixed", d, space, strategy)
    t_q = torch.from_numpy(c.qs.copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for k in mh.DEVICE_KS:
        tag = f"device/mixed/d{d}/{space}/{strategy}/k{k}"
        lab = torch.empty((c.nq, k), dtype=torch.int64, device="cuda")
        dist = torch.empty((c.nq, k), dtype=torch.float32, device="cuda")
        cnt = torch.empty(c.nq, dtype=torch.int32, device="cuda")
        o64 = torch.empty((c.nq, k), dtype=torch.float64, device="cuda")
        eng.last_stats()
        eng.search_device(t_q.data_ptr(), c.nq, k, lab.data_ptr(), dist.data_ptr(), cnt.data_ptr(), o64.data_ptr(), stream)
        torch.cuda.synchronize()
        mh.record(eng, tag, c.rows, strategy, c.qs)
        got = (lab.cpu().numpy(), dist.cpu().numpy(), cnt.cpu().numpy())
        mh.assert_knn_matches_rel(got, mh.oracle_knn(c.qs, c.rows, k, space, c.deleted), tag)
        mh.assert_family_fp64(o64.cpu().numpy(), got[1], c.qs, c.rows, got[0], space, tag)
        assert_pair_bits(eng, c.qs, got[0], o64.cpu().numpy(), got[1], tag)


# ---------------------------------------------------------------- tombstone + compact(): the attribute gather and the norm range
@pytest.mark.parametrize("strategy", mh.FAMILY_STRATEGIES)
@pytest.mark.parametrize("space", mh.SPACES)
def test_distinct_and_grouped_after_compaction(space, strategy):
    """U(124), d = 64: the nearest row of every query tombstoned on top of the corpus's own tombstones, then compact() -- the
    columns are gathered to the new labels and the norm range is rebuilt -- then distinct and grouped against the model put
    through the same calls."""
    c = mh.family_case("U124", 64)
    with np.errstate(over="ignore"):
        nearest = mh.oracle_knn(c.qs, c.rows, 1, space, c.deleted)[0][:, 0]
        model = mh.fill_engine(mh.family_model_class()(c.d, space), c, sparse=False)
    extra = np.unique(nearest)
    eng = mh.open_engine(c.rows, space, strategy, c.deleted)
    try:
        mh.fill_engine(eng, c, sparse=False)
        assert eng.tombstone(extra) == model.tombstone(extra) == extra.size
        old = eng.compact()
        assert np.array_equal(old, model.compact()) and old.size == c.n - int(c.deleted.sum()) - extra.size
        rows = c.rows[old]
        assert np.array_equal(eng.get_attr(mh.GROUP, 0, old.size), c.group[old])
        kept = mh.types.SimpleNamespace(qs=c.qs, rows=rows, group=c.group[old], nq=c.nq, corpus="U124", d=64)
        for family, call, check in (
                ("distinct", lambda e: e.search_distinct(c.qs, mh.DISTINCT_K, mh.GROUP, want64=True), check_distinct),
                ("grouped", lambda e: e.search_grouped(c.qs, mh.GROUPED_K, mh.GROUPED_SIZE, mh.GROUP, want64=True), check_grouped_cell)):
            tag = f"{family}/U124-compacted/d64/{space}/{strategy}"
            eng.last_stats()
            got = call(eng)
            mh.record(eng, tag, rows, strategy, c.qs)
            with np.errstate(over="ignore"):
                want = call(model)
                mh.assert_family_ids(family, kept, got, want, (), tag)
                check(eng, kept, space, "list", got, want, (), tag)
    finally:
        eng.close()


# ---------------------------------------------------------------- sparse weights at the ends of float32
def test_sparse_scores_with_weights_at_the_ends_of_float32():
    """mlvdb_search_batch_sparse alone, over ordinary dense rows: rows and queries whose weights are +-FLT_MAX, 2**-149,
    2**-126 and N(0,1) x 2**-140 / 2**120 mixed in one vector.  Every fp64 score within the reordering bound of the model's
    (2 x 255 x 2**-53 x sum |wq wr|: in units of the products, whatever their scale) and finite, the ranking by (score64,
    label), the model's k-th row returned or beaten, the fp32 face the rounded score (+-inf for a real row beyond FLT_MAX);
    the ids are the model's wherever its ranking is beyond the bound; a pair scores the same 64 bits in two batches."""
    rows, queries = mh.sparse_edge_case()
    dense = mh.mixed_inputs(64)[0][:mh.SPARSE_EDGE_N]
    k = mh.SPARSE_EDGE_K
    model = SparseOracleEngine(64, "l2")
    model.append(dense)
    model.define_attr(0, "sparse")
    model.set_attr_sparse(0, 0, sparse_csr(rows))
    eng = mh.open_engine(dense, "l2", "exact")
    try:
        eng.define_attr(0, "sparse")
        eng.set_attr_sparse(0, 0, sparse_csr(rows))
        lab, s32, cnt, s64 = eng.search_batch_sparse(0, sparse_csr(queries), k)
        scores, mass = dense_scores(queries, rows)
        cand = model.candidates(0)
        wl, ws64, wc = rank(scores, cand, k + 1)
        apart = mh.sparse_ranks_apart(scores, mass, wl, cand)
        assert (cnt == k).all() and (lab >= 0).all()
        for q in range(len(queries)):
            got, s = lab[q], s64[q]
            assert cand[got].all() and np.unique(got).size == k and np.isfinite(s).all(), f"query {q}"
            bound = mh.SPARSE_EPS * mass[q]
            err = np.abs(s - scores[q, got])
            print(f"sparse edge q={q}: worst error / bound {float((err / np.maximum(bound[got], 5e-324)).max()):.3e}, apart {apart[q]}")
            assert (err <= bound[got]).all(), f"query {q}: a score is {float((err / bound[got]).max()):.3f} bounds off"
            assert np.array_equal(np.lexsort((got, -s)), np.arange(k)), f"query {q}: not sorted by (-score64, label)"
            assert (s >= scores[q, wl[q, k - 1]] - bound[wl[q, k - 1]]).all(), f"query {q}: the model's k-th row beats a returned one"
            if apart[q]:
                assert np.array_equal(got, wl[q, :k]), f"query {q}: ids {got.tolist()}, the model's {wl[q, :k].tolist()}"
        with np.errstate(over="ignore"):
            assert np.array_equal(bits(s32), bits(s64.astype(np.float32))), "fp32 is not the rounded fp64"
        assert np.isinf(s32).any(), "no score beyond FLT_MAX: the case lost its point"
        # purity: the same pair in another batch, at another place in its tile, under another k
        seen = {(q, int(l)): int(b) for q in range(len(queries)) for l, b in zip(lab[q], bits(s64[q]))}
        order = np.arange(len(queries))[::-1]
        lab2, _, cnt2, s642 = eng.search_batch_sparse(0, sparse_csr([queries[i] for i in order[:5]]), 64)
        hit = 0
        for j, q in enumerate(order[:5]):
            for l, b in zip(lab2[j, :cnt2[j]], bits(s642[j, :cnt2[j]])):
                if (int(q), int(l)) in seen:
                    hit += 1
                    assert seen[int(q), int(l)] == int(b), f"query {q}, label {l}: the score depends on the batch"
        assert hit >= 5 * k
    finally:
        eng.close()
