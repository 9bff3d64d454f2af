"""Preconditions of tests/test_gpu_magnitudes_families.py, on the model engines alone (no GPU): for every cell that file
runs (magnitude_helpers.family_cells: the same list), the model's own ids do not depend on the order of summation
(family_unstable: the columns as given, reversed and under a seeded permutation), so a device answer that differs is the
device's fault; and every input the cells send is what they say it is -- finite like queries, float32 radii, programs on
the intended side of the gather / scan route plan, brute-force restatements equal to the vectorised models.

The bar: no unstable query on the uniform, ladder and mixed corpora, for any family; on ``edge`` (FLT_MAX rows queried back,
where terms cancel) at most one query in three of a case may be left out of the id comparison, and the device file still
holds those queries to its self-consistency checks.  A seed or parameter that fails is replaced in magnitude_helpers.py."""
import numpy as np
import pytest

from oracle import exact_scan
from tests import magnitude_helpers as mh
from tests.distinct_helpers import ABSENT, distinct_knn, distinct_knn_brute
from tests.grouped_helpers import grouped_knn, grouped_knn_brute
from tests.like_helpers import like_queries
from tests.maxsim_helpers import maxsim_brute, maxsim_oracle
from tests.mmr_helpers import MmrOracleEngine, mmr_select_brute
from tests.sparse_helpers import dense_scores, rank
from tests.where_helpers import eval_program

CELLS = mh.family_cells()
CASES = [(c, d, s) for c, d in mh.FAMILY_CORPORA for s in mh.SPACES]


def test_the_matrix_is_what_both_files_run():
    assert len(CELLS) == len(set(CELLS))
    for family in mh.FAMILIES:
        mine = [cell for cell in CELLS if cell[0] == family]
        if family == "range_each":  # cosine everywhere; l2 at U(-64), U(40) and mixed; ip at mixed alone
            assert len(mine) == len(mh.FAMILY_CORPORA) + (2 * 2 + 2) + 2
        else:
            assert len(mine) == 3 * len(mh.FAMILY_CORPORA)
    sizes = {(c, d): mh.family_case(c, d) for c, d in mh.FAMILY_CORPORA}
    assert all(v.n == 3000 and v.nq == 12 for (c, _), v in sizes.items() if c.startswith("U"))
    assert all(v.n == 4096 and v.nq == 10 for (c, _), v in sizes.items() if c == "ladder")
    assert sizes["edge", 64].n == 4105 and sizes["edge", 64].nq == 17 and sizes["edge", 64].n % 16 == 9
    assert all(v.n == 3000 and v.nq == 11 and v.odd.tolist() == [1, 4, 9] for (c, _), v in sizes.items() if c == "mixed")


# ---------------------------------------------------------------- stability, cell by cell
@pytest.mark.parametrize("family,corpus,d,space", CELLS, ids=["/".join(map(str, c)) for c in CELLS])
def test_the_models_ids_do_not_depend_on_the_order_of_summation(family, corpus, d, space):
    c = mh.family_case(corpus, d)
    unstable = mh.family_unstable(family, corpus, d, space)
    assert set(unstable) == {name for name, _, _ in mh.family_variants(family, c, space)}
    nq = len(mh.MAXSIM_LENGTHS) if family == "maxsim" else c.nq
    print(f"{family}/{corpus}/d{d}/{space}: queries left out per variant "
          f"{ {name: len(v) for name, v in unstable.items()} } of {nq}")
    for name, queries in unstable.items():
        if corpus == "edge":
            assert len(queries) * mh.EDGE_EXCLUDED_CAP <= nq, f"{name}: {queries} of {nq} queries are unstable: over a third"
        else:
            assert not queries, f"{name}: the model's ids of queries {queries} depend on the order of summation"
        assert mh.family_excluded(family, corpus, d, space)[name] == queries


# ---------------------------------------------------------------- the columns, the programs and their routes
@pytest.mark.parametrize("corpus,d", mh.FAMILY_CORPORA)
def test_columns_are_functions_of_the_label_and_every_program_takes_its_intended_route(corpus, d):
    c = mh.family_case(corpus, d)
    label = np.arange(c.n)
    assert np.array_equal(c.bucket, label % 4)
    assert np.array_equal(c.group == ABSENT, label % 11 == 5) and np.array_equal(c.group[c.group != ABSENT],
                                                                                 (label % 37)[label % 11 != 5])
    if corpus == "ladder":  # every group holds every rung of the ladder
        for g in range(37):
            assert {int(r) for r in label[c.group == g] % len(mh.LADDER)} == set(range(len(mh.LADDER)))
    if corpus == "edge":    # every edge row shares its group with ordinary rows
        places = mh.edge_inputs(d)[3]
        for p in places.ravel():
            assert c.group[p] == ABSENT or ((c.group == c.group[p]) & ~c.deleted).sum() > 50
    live = int((~c.deleted).sum())
    cols = {mh.GROUP: c.group, mh.BUCKET: c.bucket}
    want = ("scan", "scan", "gather")
    assert want[mh.GATHERED_PROGRAM] == "gather"
    for p, program in enumerate(c.programs):
        matches = int((eval_program(program, cols, c.n) & ~c.deleted).sum())
        queries = int((c.program_of_query == p).sum())
        assert queries >= 2, "every program has queries"
        assert mh.route_plan(matches, queries, live) == want[p], f"program {p}: {matches} of {live} rows, {queries} queries"
        assert matches >= 3 * mh.EACH_K, "a filtered query still has k rows to find"
    assert (c.program_of_query == -1).sum() >= 2
    if corpus == "mixed":  # the odd queries sit under the gathered program and under a scanned one
        assert {int(c.program_of_query[i]) for i in c.odd} == {mh.GATHERED_PROGRAM, 0}
        toks = c.token_of[:mh.MAXSIM_LENGTHS[0]]  # and the first late-interaction query holds an odd token beside ordinary ones
        assert np.isin(toks, c.odd).any() and not np.isin(toks, c.odd).all()
    # the sparse column: <= 16 of 64 terms, about a row in ten without a vector
    lens = [len(r) for r in c.sparse_list if r is not None]
    assert max(lens) == mh.SPARSE_MAX_NNZ and min(lens) == 0 and 0.05 < c.sparse_list.count(None) / c.n < 0.15
    assert all(0 <= t < mh.SPARSE_VOCAB for r in c.sparse_list if r for t in r)


@pytest.mark.parametrize("corpus,d,space", CASES)
def test_distincts_list_pass_finishes_every_query(corpus, d, space):
    """So ``fallback_queries`` of a distinct or grouped call counts what the search under it adds and nothing else."""
    c = mh.family_case(corpus, d)
    with np.errstate(over="ignore"):
        assert mh.distinct_list_short(c, space) == []


# ---------------------------------------------------------------- like queries and range radii
@pytest.mark.parametrize("corpus,d,space", CASES)
def test_every_synthesised_like_query_is_a_finite_float32(corpus, d, space):
    c = mh.family_case(corpus, d)
    assert not c.deleted[c.like_labels].any() and (c.like_labels.reshape(-1, 2)[:, 0] != c.like_labels.reshape(-1, 2)[:, 1]).all()
    assert c.like_weights == (mh.LIKE_WEIGHTS_EDGE if corpus == "edge" else mh.LIKE_WEIGHTS)
    if corpus == "edge":
        assert np.isin(c.like_labels, mh.edge_inputs(d)[3][0]).sum() >= len(mh.EDGE_KINDS)
    for w in c.like_weights:
        for base in (None, c.qs) if space == "cosine" else (None,):
            with np.errstate(over="ignore"):
                qs, _ = like_queries(c.rows, c.like_labels, np.tile(np.array(w, dtype=np.float64), c.nq), c.like_offsets, space, base)
            assert qs.dtype == np.float32 and np.isfinite(qs).all(), f"weights {w}: a synthesised query is not finite"
            assert qs.any(axis=1).all(), f"weights {w}: a synthesised query is zero"


@pytest.mark.parametrize("corpus,d,space", [c[1:] for c in CELLS if c[0] == "range_each"])
def test_every_range_each_radius_is_a_finite_float32_with_hits(corpus, d, space):
    c = mh.family_case(corpus, d)
    radius = mh.family_radius(c, space)
    assert np.isfinite(np.float32(radius)) and float(np.float32(radius)) == radius
    if space != "cosine" and corpus.startswith("U"):
        assert int(corpus[1:]) in mh.RANGE_EXPONENTS[space]
    hits = mh.family_expected("range_each", corpus, d, space)[f"r{radius!r}"][0]
    sizes = np.array([len(h[0]) for h in hits])
    ordinary = np.setdiff1d(np.arange(c.nq), c.odd)
    assert sizes[ordinary].sum() > 0 and sizes.max() <= mh.RANGE_MAX_HITS, f"hits per query: {sizes}"


# ---------------------------------------------------------------- the models against their definitions
@pytest.mark.parametrize("space", mh.SPACES)
@pytest.mark.parametrize("corpus,d", [("U124", 64), ("edge", 64)])
def test_each_brute_force_restatement_equals_its_model(corpus, d, space):
    c = mh.family_case(corpus, d)
    allowed = ~c.deleted
    with np.errstate(over="ignore"):
        dist = exact_scan.exact_distances(c.qs, c.rows, space)
    # distinct
    lab, d64, cnt, grp = distinct_knn(dist, c.group, allowed, mh.DISTINCT_K)
    for i, want in enumerate(distinct_knn_brute(dist, c.group, allowed, mh.DISTINCT_K)):
        assert cnt[i] == len(want)
        assert [(float(d64[i, j]), int(lab[i, j]), int(grp[i, j])) for j in range(cnt[i])] == want
    # grouped
    lab, d64, cnt, gcnt, grp = grouped_knn(dist, c.group, allowed, mh.GROUPED_K, mh.GROUPED_SIZE)
    for i, want in enumerate(grouped_knn_brute(dist, c.group, allowed, mh.GROUPED_K, mh.GROUPED_SIZE)):
        assert cnt[i] == len(want)
        for j, (code, members) in enumerate(want):
            assert grp[i, j] == code and gcnt[i, j] == len(members)
            assert [(float(d64[i, j, t]), int(lab[i, j, t])) for t in range(gcnt[i, j])] == members
    # late interaction
    toks = c.token_of
    g, s64, cnt, ml, md = maxsim_oracle(dist[toks], c.group, allowed, c.token_offsets, mh.MAXSIM_K)
    for i, want in enumerate(maxsim_brute(dist[toks], c.group, allowed, c.token_offsets, mh.MAXSIM_K)):
        assert cnt[i] == len(want)
        t0, t1 = int(c.token_offsets[i]), int(c.token_offsets[i + 1])
        for j, (score, code, matches) in enumerate(want):
            assert (float(s64[i, j]), int(g[i, j])) == (score, code)
            assert [(float(md[t, j]), int(ml[t, j])) for t in range(t0, t1)] == matches
    # diversified: the greedy restated on the family model's own distances (mmr_distances for both terms of the objective);
    # MmrOracleEngine, whose two distances come from matrix products of two shapes, picks the same rows for every query
    # that is no stored row.  A stored row queried back ties the objectives of lambda = 0.5 at exactly 0.
    stored = [i for i in range(c.nq) if (c.rows[allowed].view(np.uint32) == c.qs[i].view(np.uint32)).all(axis=1).any()]
    assert stored, "the corpus queries a stored row back"
    with np.errstate(over="ignore"):
        model = mh.family_model(c, space)
        for lam in mh.MMR_LAMBDAS:
            got = model.search_mmr(c.qs, mh.MMR_K, mh.MMR_FETCH, lam, want64=True)
            whole = MmrOracleEngine.search_mmr(model, c.qs, mh.MMR_K, mh.MMR_FETCH, lam, want64=True)
            other = np.setdiff1d(np.arange(c.nq), stored)
            for a, b in ((got[0], whole[0]), (got[2], whole[2]), (got[4], whole[4])):
                assert np.array_equal(a[other], b[other])
            cl, _, cc, _ = model.search64(c.qs, mh.MMR_FETCH)
            for i in range(c.nq):
                cands = cl[i, :cc[i]]
                dq = mh.mmr_distances(c.qs[i], c.rows[cands], space)
                P = np.stack([mh.mmr_distances(c.rows[s], c.rows[cands], space) for s in cands])
                picks, objs = mmr_select_brute(dq, P, mh.MMR_K, lam)
                assert got[4][i, :len(picks)].tolist() == picks and got[5][i, :len(picks)].tolist() == objs
                if i in stored and lam == 0.5 and cands[0] in np.flatnonzero((c.rows.view(np.uint32) == c.qs[i].view(np.uint32)).all(axis=1)):
                    # d(q, i) = D(c_0, i) bit for bit: after the first pick every objective is exactly 0
                    assert picks[1] == 1 and objs[1] == 0, "the second pick ties at exactly 0 and falls to the position"


# ---------------------------------------------------------------- the bars
def test_the_l2_bar_is_in_units_of_the_summed_terms():
    rng = np.random.default_rng(3)
    for e in (-140, 0, 124):
        rows = rng.standard_normal((20, 16), dtype=np.float32) * mh.pow2(e)
        qs = rng.standard_normal((2, 16), dtype=np.float32) * mh.pow2(e)
        labels = np.array([[0, 4, -1], [7, 7, 19]], dtype=np.int64)
        for space in mh.SPACES:
            full = exact_scan.exact_distances(qs, rows, space)
            want = np.take_along_axis(full, np.maximum(labels, 0), axis=1)
            want[labels < 0] = np.inf
            with np.errstate(over="ignore"):
                mh.assert_family_fp64(want, want.astype(np.float32), qs, rows, labels, space, space)
                mh.assert_family_fp64(want.reshape(2, 3, 1), None, qs, rows, labels.reshape(2, 3, 1), space, space)
            if space == "l2":  # an error of 1e-9 of the distance itself is over the bar at every scale (no floor of 1)
                off = want.copy()
                off[1, 2] *= 1 + 1e-9
                with pytest.raises(AssertionError):
                    mh.assert_family_fp64(off, None, qs, rows, labels, space, space)
                bar = mh.family_fp64_bar(qs, rows, np.maximum(labels, 0), want, space)
                assert (bar[labels >= 0] >= 1e-12 * want[labels >= 0]).all() and (bar <= 4e-12 * 16 * 36 * 4.0 ** e).all()
            pad = want.copy()
            pad[0, 2] = 3.4e38
            with pytest.raises(AssertionError):  # padding is +inf, whatever the scale
                mh.assert_family_fp64(pad, None, qs, rows, labels, space, space)
            nan = want.copy()
            nan[0, 0] = np.inf
            with pytest.raises(AssertionError):  # a real pair's fp64 distance is finite
                mh.assert_family_fp64(nan, None, qs, rows, labels, space, space)


# ---------------------------------------------------------------- sparse weights at the ends of float32
def test_the_sparse_edge_case_holds_every_kind_of_weight_and_ranks_apart():
    rows, queries = mh.sparse_edge_case()
    assert len(rows) == mh.SPARSE_EDGE_N and len(queries) == mh.SPARSE_EDGE_NQ
    weights = np.array([w for r in rows + queries if r for w in r.values()], dtype=np.float64)
    assert np.isfinite(weights).all() and (weights != 0).all()
    assert np.array_equal(weights.astype(np.float32).astype(np.float64), weights), "every weight is a float32"
    fmax = float(mh.F32_MAX)
    for name, sel in (("+FLT_MAX", weights == fmax), ("-FLT_MAX", weights == -fmax), ("2**-149", weights == 2.0 ** -149),
                      ("2**-126", weights == 2.0 ** -126), ("subnormal", (np.abs(weights) < 2.0 ** -126) & (np.abs(weights) > 2.0 ** -149)),
                      ("2**120 N(0,1)", (np.abs(weights) > 2.0 ** 115) & (np.abs(weights) < 2.0 ** 124))):
        assert sel.sum() > 20, name
    mixed = sum(1 for r in rows if r and max(abs(w) for w in r.values()) == fmax and min(abs(w) for w in r.values()) < 2.0 ** -126)
    assert mixed > 50, "rows that hold FLT_MAX and a subnormal at once"
    assert all(len(r) <= mh.SPARSE_MAX_NNZ for r in rows + queries if r) and rows.count(None) > 30
    scores, mass = dense_scores(queries, rows)
    assert np.isfinite(scores).all() and np.isfinite(mass).all() and mass.max() > 1e75, "FLT_MAX x FLT_MAX is an fp64"
    cand = np.array([r is not None for r in rows])
    lab, s64, cnt = rank(scores, cand, mh.SPARSE_EDGE_K + 1)
    assert (cnt == mh.SPARSE_EDGE_K + 1).all()
    apart = mh.sparse_ranks_apart(scores, mass, lab, cand)
    print("queries ranked beyond the reordering bound:", np.flatnonzero(apart).tolist())
    assert apart[-6:].all(), f"the queries over the plain terms do not all rank beyond the reordering bound: {apart[-6:]}"
