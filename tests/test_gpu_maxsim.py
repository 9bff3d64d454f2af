"""Late-interaction search on the MI355X (include/mlvdb_maxsim.h) through the C ABI against the NumPy oracle
(tests/maxsim_helpers.py).  Groups, counts and match labels equal the oracle exactly; fp64 scores are within
SCORE_ATOL x max(1, |s|) of it; the match distances are bit-equal to ``pair_distances`` of the returned pairs and the fp64
score is bit-equal to their sequential sum.  Rows and tokens are Gaussian (``tests.helpers.make_case``).  Checked on the CPU against the oracle
over every case of test a below (T up to 33 and the ragged batch included): the smallest relative gap between neighbouring
document scores among the first 66 is 2.2e-7, the smallest gap between the best and the second-best row of a (token,
document) 3.0e-7 -- both eight orders above fp64 rounding, so exact id equality with the oracle is a fair demand."""
import functools
import uuid

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, VectorDTO
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.distinct_helpers import ABSENT
from tests.facet_helpers import colliding_keys, facet_hash
from tests.helpers import SCORE_ATOL, make_case
from tests.maxsim_helpers import check_maxsim, maxsim_oracle, offsets_of, oracle_index
from tests.where_helpers import SCHEMA, py_match, random_filter, random_metadata

pytestmark = pytest.mark.gpu

INT64_MAX = np.iinfo(np.int64).max


def _engine(space, rows, groups, tomb=None):
    eng = HipScanEngine(rows.shape[1], space, device=0)
    eng.append(rows)
    eng.define_attr(0, "int64")
    eng.set_attr(0, 0, np.ascontiguousarray(groups, dtype=np.int64))
    if tomb is not None and tomb.any():
        eng.tombstone(np.flatnonzero(tomb))
    return eng


def _check(eng, toks, off, k, want, tag, **kw):
    """One call against the oracle's (groups, score64, counts, match labels, match dist64) for this k; the bit contracts."""
    return check_maxsim(eng, toks, off, k, eng.search_maxsim(toks, off, k, 0, want_matches=True, **kw), want, tag)


def _documents(rng, n, lo, hi):
    """Contiguous documents of lo..hi rows over n rows: one code per row (codes 0, 1, ...)."""
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(lo, hi + 1)))
    return np.repeat(np.arange(len(sizes)), sizes)[:n].astype(np.int64)


# ---------------------------------------------------------------- a. token tiles, spaces, dims, both layouts
TILE_SHAPES = {48: (5000, 1, 9), 200: (3000, 1, 40), 768: (2500, 300, 900)}  # d -> (rows, rows per document lo..hi)
TS = (1, 7, 8, 9, 33)
RAGGED = (1, 9, 8, 33)


@functools.lru_cache(maxsize=None)
def _case_a(space, d, layout):
    """(rows, groups, tombstones, tokens, the oracle per call) -- computed once, left unchanged."""
    n, lo, hi = TILE_SHAPES[d]
    rows, toks = make_case(300 + d, n, d, sum(RAGGED))
    rng = np.random.default_rng(7 * d + len(space))
    groups = _documents(rng, n, lo, hi)
    if layout == "scattered":
        groups = rng.permutation(groups)  # the same documents, their rows all over the corpus
    groups[rng.random(n) < 0.05] = ABSENT
    tomb = rng.random(n) < 0.08
    dist = exact_scan.exact_distances(toks, rows, space)
    calls = {}
    for T in TS:
        calls[(T,)] = maxsim_oracle(dist[:T], groups, ~tomb, offsets_of([T]), 64)
    calls[RAGGED] = maxsim_oracle(dist, groups, ~tomb, offsets_of(RAGGED), 64)
    for want in calls.values():
        for a in want:
            a.setflags(write=False)
    return rows, groups, tomb, toks, calls


def _cut(want, k):
    wg, ws, wc, wml, wmd = want
    return wg[:, :k], ws[:, :k], np.minimum(wc, k).astype(np.int32), wml[:, :k], wmd[:, :k]


@pytest.mark.parametrize("layout", ["contiguous", "scattered"])
@pytest.mark.parametrize("d", [48, 200, 768])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_token_tiles_equal_the_oracle(space, d, layout):
    rows, groups, tomb, toks, calls = _case_a(space, d, layout)
    eng = _engine(space, rows, groups, tomb)
    try:
        for lengths, want in calls.items():
            ntok = sum(lengths)
            for k in (1, 10, 64):
                _check(eng, toks[:ntok], offsets_of(lengths), k, _cut(want, k), f"a_{space}_{d}_{layout}_T{lengths}_k{k}")
    finally:
        eng.close()


# ---------------------------------------------------------------- b. rows and panels
@pytest.mark.parametrize("n", [1, 15, 17, 1005])
def test_small_corpora_and_k_above_the_number_of_documents(n):
    d = 24
    rows, toks = make_case(40 + n, n, d, 12)
    groups = (np.arange(n) // 4).astype(np.int64)  # documents of 4 rows: ceil(n / 4) of them
    ndocs = -(-n // 4)
    off = offsets_of([3, 8, 1])
    for space in ("l2", "cosine", "ip"):
        dist = exact_scan.exact_distances(toks, rows, space)
        eng = _engine(space, rows, groups)
        try:
            for k in (1, 10, 64):
                _, cnt, _, _, _ = _check(eng, toks, off, k, maxsim_oracle(dist, groups, np.ones(n, bool), off, k), f"b_{space}_{n}_k{k}")
                assert cnt.tolist() == [min(k, ndocs)] * 3
        finally:
            eng.close()


# ---------------------------------------------------------------- c. document shapes
def test_one_document_holding_every_row_and_a_bool_column():
    n, d = 2000, 32
    rows, toks = make_case(51, n, d, 10)
    off = offsets_of([9, 1])
    dist = exact_scan.exact_distances(toks, rows, "cosine")
    rng = np.random.default_rng(51)
    for name, groups in (("one", np.full(n, 42, np.int64)), ("bool", rng.integers(0, 2, n).astype(np.int64))):
        eng = _engine("cosine", rows, groups)
        try:
            _, cnt, _, _, _ = _check(eng, toks, off, 5, maxsim_oracle(dist, groups, np.ones(n, bool), off, 5), f"c_{name}")
            assert cnt.tolist() == [np.unique(groups).size] * 2
        finally:
            eng.close()


def test_codes_negative_near_int64_max_and_in_one_probe_chain():
    n, d = 1500, 16
    rows, toks = make_case(52, n, d, 17)
    off = offsets_of([8, 9])
    # 40 documents: the table has 128 slots; 12 of the codes share one probe chain, the others are extreme values
    chain = colliding_keys(128, 12, slot=5, start=1000)
    assert np.unique(facet_hash(chain) & np.uint64(127)).tolist() == [5]
    extreme = np.array([ABSENT + 1, ABSENT + 2, -1, -2, 0, 1, INT64_MAX, INT64_MAX - 1], np.int64)
    codes = np.concatenate([chain, extreme, np.arange(-30, -10, dtype=np.int64)])
    rng = np.random.default_rng(52)
    groups = codes[rng.integers(0, codes.size, n)]
    dist = exact_scan.exact_distances(toks, rows, "l2")
    eng = _engine("l2", rows, groups)
    try:
        grp, cnt, _, _, _ = _check(eng, toks, off, 64, maxsim_oracle(dist, groups, np.ones(n, bool), off, 64), "c_codes")
        assert cnt.tolist() == [codes.size] * 2 and set(grp[0, :codes.size].tolist()) == set(codes.tolist())
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _case_own(space):
    n, d = 5005, 48
    rows, toks = make_case(53, n, d, 9)
    return rows, toks, exact_scan.exact_distances(toks, rows, space)


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_every_row_its_own_document_ranks_over_several_blocks_and_t1_equals_the_plain_search(space):
    """G = 5005 documents: the rank kernel runs 20 blocks per query.  With T = 1 the call is the plain search, bit for bit."""
    rows, toks, dist = _case_own(space)
    n = rows.shape[0]
    groups = (np.arange(n, dtype=np.int64) * 7 - 3000)  # distinct codes, ascending with the label
    eng = _engine(space, rows, groups)
    try:
        off = offsets_of([9])
        _check(eng, toks, off, 64, maxsim_oracle(dist, groups, np.ones(n, bool), off, 64), f"c_own_{space}")
        one = offsets_of([1] * 9)
        grp, cnt, s64, ml, md = _check(eng, toks, one, 10, maxsim_oracle(dist, groups, np.ones(n, bool), one, 10), f"c_own1_{space}")
        _, s32, _, _, _, _ = eng.search_maxsim(toks, one, 10, 0)
        eng.set_strategy("exact")
        lab, d32, pc, d64 = eng.search64(toks, 10)
        assert np.array_equal(ml, lab) and np.array_equal(grp, groups[lab]) and np.array_equal(cnt, pc)
        assert np.array_equal(s64.view(np.int64), d64.view(np.int64)) and np.array_equal(md.view(np.int64), d64.view(np.int64))
        assert np.array_equal(s32.view(np.int32), d32.view(np.int32))
    finally:
        eng.close()


# ---------------------------------------------------------------- d. anchors
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_one_token_per_query_equals_search_distinct_bit_for_bit(space):
    n, d, nq = 3000, 200, 9
    rows, toks = make_case(61, n, d, nq)
    rng = np.random.default_rng(61)
    groups = rng.permutation(_documents(rng, n, 1, 40))
    groups[rng.random(n) < 0.1] = ABSENT
    tomb = rng.random(n) < 0.1
    eng = _engine(space, rows, groups, tomb)
    try:
        for k in (1, 10, 64):
            grp, s32, cnt, s64, ml, md = eng.search_maxsim(toks, offsets_of([1] * nq), k, 0, want_matches=True)
            lab, d32, dc, d64, dg = eng.search_distinct(toks, k, 0, want64=True)
            assert np.array_equal(grp, dg) and np.array_equal(cnt, dc) and np.array_equal(ml, lab), (space, k)
            assert np.array_equal(s64.view(np.int64), d64.view(np.int64)) and np.array_equal(md.view(np.int64), d64.view(np.int64))
            assert np.array_equal(s32.view(np.int32), d32.view(np.int32))
    finally:
        eng.close()


def test_ip_with_dot_products_of_both_signs_orders_negative_and_positive_distances():
    n, d = 1200, 16
    rows, toks = make_case(62, n, d, 9)
    rows, toks = rows * 2.0, toks * 2.0  # |<q, x>| well above 1: distances 1 - <q, x> of both signs
    groups = _documents(np.random.default_rng(62), n, 1, 6)
    dist = exact_scan.exact_distances(toks, rows, "ip")
    off = offsets_of([9])
    want = maxsim_oracle(dist, groups, np.ones(n, bool), off, 64)
    assert (want[4][np.isfinite(want[4])] < 0).any() and (want[4][np.isfinite(want[4])] > 0).any()
    eng = _engine("ip", rows, groups)
    try:
        _check(eng, toks, off, 64, want, "d_ip_signs")
    finally:
        eng.close()


# ---------------------------------------------------------------- e. liveness
def test_a_document_without_counted_rows_disappears():
    n, d = 900, 16
    rows, toks = make_case(71, n, d, 8)
    groups = (np.arange(n) // 9).astype(np.int64)  # 100 documents of 9 rows
    tomb = np.zeros(n, bool)
    tomb[groups == 17] = True           # every row tombstoned
    tomb[(groups == 18) & (np.arange(n) % 9 < 8)] = True  # one row left
    groups[groups == 19] = ABSENT       # every value absent
    off = offsets_of([8])
    dist = exact_scan.exact_distances(toks, rows, "l2")
    eng = _engine("l2", rows, groups, tomb)
    try:
        grp, cnt, _, ml, _ = _check(eng, toks, off, 64, maxsim_oracle(dist, groups, ~tomb, off, 64), "e_gone")
        eng.tombstone(np.flatnonzero(groups != 18))  # then everything but that one row
        grp, cnt, _, ml, _ = _check(eng, toks, off, 64, maxsim_oracle(dist, groups, ~tomb & (groups == 18), off, 64), "e_last")
        assert cnt.tolist() == [1] and grp[0, 0] == 18 and set(ml[:, 0].tolist()) == {18 * 9 + 8}
        eng.tombstone(np.array([18 * 9 + 8]))       # fully tombstoned: padding
        grp, s32, cnt, s64, ml, md = eng.search_maxsim(toks, off, 5, 0, want_matches=True)
        assert cnt.tolist() == [0] and (grp == ABSENT).all() and np.isinf(s32).all() and np.isinf(s64).all()
        assert (ml == -1).all() and np.isinf(md).all()
    finally:
        eng.close()


def test_random_dict_filters_and_tombstones_count_only_the_matching_rows():
    rng = np.random.default_rng(72)
    n, d, k = 2000, 16, 10
    schema = dict(SCHEMA, doc="int")
    metas = random_metadata(rng, n)
    doc = rng.integers(0, 150, n).astype(np.int64)
    docs = np.full(n, ABSENT, np.int64)
    for j, (m, v) in enumerate(zip(metas, doc.tolist())):
        if rng.random() < 0.85:
            m["doc"], docs[j] = v, v
    rows, toks = make_case(72, n, d, 20)
    off = offsets_of([9, 3, 8])
    queries = [toks[off[i]:off[i + 1]] for i in range(3)]
    dist = exact_scan.exact_distances(toks, rows, "cosine")
    idx = Index(space="cosine", attributes=schema)
    try:
        ids = idx.add_arrays(rows, "ns", attributes=idx.extract_attributes(metas))
        live = np.ones(n, bool)
        gone = rng.choice(n, 300, replace=False)
        idx.remove([uuid.UUID(bytes=bytes(ids[j])) for j in gone], "ns")
        live[gone] = False
        emptied = 0
        for f in [None] + [random_filter(rng) for _ in range(8)] + [{"genre": "zydeco"}, {}, {"doc": {"$lt": 75}}]:
            allowed = live if f is None else live & np.array([py_match(f, m, schema) for m in metas])
            wg, ws, wc, wml, _ = maxsim_oracle(dist, docs, allowed, off, k)
            got = idx.search_late(queries, k, "ns", "cosine", "doc", where=f, matches=True)
            assert np.array_equal(got.counts, wc) and np.array_equal(got.match_labels, wml), f
            have = np.arange(k)[None, :] < wc[:, None]
            assert got.values[have].tolist() == wg[have].tolist() and (got.values[~have] == None).all(), f  # noqa: E711
            want = np.array([9.0, 3.0, 8.0])[:, None] - ws  # the sum of cosines
            assert (np.abs(got.scores[have] - want[have]) <= SCORE_ATOL * np.maximum(1.0, np.abs(want[have]))).all(), f
            emptied += int(wc[0] == 0)
        assert emptied >= 1  # ("zydeco" was never ingested: no row matches, every document disappears)
    finally:
        idx.close()


def test_after_append_tombstone_compact_and_attribute_updates_the_answer_follows():
    rng = np.random.default_rng(73)
    n, d = 1200, 16
    rows, toks = make_case(73, n, d, 17)
    off = offsets_of([8, 9])
    groups = rng.permutation(_documents(rng, n, 1, 9))
    tomb = np.zeros(n, bool)
    eng = _engine("l2", rows, groups)

    def check(tag):
        dist = exact_scan.exact_distances(toks, rows, "l2")
        return _check(eng, toks, off, 10, maxsim_oracle(dist, groups, ~tomb, off, 10), tag)

    try:
        check("e_start")
        more, _ = make_case(74, 100, d, 1)
        more[:17] = toks + 1e-3 * more[:17]  # the new rows are the nearest of their tokens: their documents take the lead
        more_groups = np.concatenate([np.full(17, 5000, np.int64), rng.integers(0, 50, 83)])
        assert eng.append(more) == n
        eng.set_attr(0, n, more_groups)
        rows, groups, tomb = np.vstack([rows, more]), np.concatenate([groups, more_groups]), np.concatenate([tomb, np.zeros(100, bool)])
        grp, _, _, _, _ = check("e_append")
        assert grp[:, 0].tolist() == [5000, 5000]
        dead = rng.choice(n + 100, 250, replace=False)
        eng.tombstone(dead)
        tomb[dead] = True
        check("e_tombstone")
        old = eng.compact()
        rows, groups, tomb = rows[old], groups[old], np.zeros(old.size, bool)
        check("e_compact")
        moved = rng.choice(old.size, 60, replace=False)
        values = np.where(np.arange(60) < 50, 7777, ABSENT).astype(np.int64)  # fifty rows join a new document, ten lose theirs
        assert eng.set_attr_at(0, moved, values) == 60
        groups = groups.copy()
        groups[moved] = values
        check("e_update")
    finally:
        eng.close()


# ---------------------------------------------------------------- f. ties
def test_identical_documents_rank_by_code_duplicates_match_the_lower_label_and_calls_repeat():
    n, d = 600, 16
    rows, toks = make_case(81, n, d, 8)
    groups = (np.arange(n) // 6).astype(np.int64) * 5 - 100  # 100 documents of 6 rows
    rows[30:36] = rows[12:18]   # document of rows 30..35 is a copy of the document of rows 12..17: equal scores
    rows[41] = rows[38]         # a duplicate row inside one document (rows 36..41)
    toks[0] = rows[38]          # ... which a token hits exactly
    toks[1] = rows[13]
    off = offsets_of([8])
    dist = exact_scan.exact_distances(toks, rows, "l2")
    want = maxsim_oracle(dist, groups, np.ones(n, bool), off, 64)
    eng = _engine("l2", rows, groups)
    try:
        grp, cnt, s64, ml, md = _check(eng, toks, off, 64, want, "f_ties")
        a, b = grp[0].tolist().index(int(groups[12])), grp[0].tolist().index(int(groups[30]))
        assert b == a + 1 and s64[0, a] == s64[0, b]  # equal scores: the smaller code first
        j = grp[0].tolist().index(int(groups[38]))
        assert ml[0, j] == 38 and md[0, j] == 0.0  # the lower label of the two copies
        first = eng.search_maxsim(toks, off, 64, 0, want_matches=True)
        again = eng.search_maxsim(toks, off, 64, 0, want_matches=True)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first, again))
    finally:
        eng.close()


# ---------------------------------------------------------------- g. chunking
def test_a_small_workspace_cuts_the_call_into_chunks_and_returns_the_same_bytes():
    rows, groups, tomb, toks, calls = _case_a("cosine", 48, "scattered")
    lengths = (9, 33, 1, 8, 7)  # 58 tokens x ~1000 documents x 8 B: ~0.45 MiB a query of 33 tokens ...
    rng = np.random.default_rng(91)
    toks = rng.standard_normal((sum(lengths) * 3, 48), dtype=np.float32)
    off = offsets_of(lengths * 3)
    eng = _engine("cosine", rows, groups, tomb)
    try:
        assert eng.get_tuning("MAXSIM_WS_MB") == 1024
        ndocs = np.unique(groups[~tomb & (groups != ABSENT)]).size
        assert int(off[-1]) * ndocs * 8 > 1 << 20  # ... so 1 MiB holds no more than a few queries of the fifteen
        first = eng.search_maxsim(toks, off, 10, 0, want_matches=True)
        eng.set_tuning(MAXSIM_WS_MB=1)
        small = eng.search_maxsim(toks, off, 10, 0, want_matches=True)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first, small))
        dist = exact_scan.exact_distances(toks, rows, "cosine")
        _check(eng, toks, off, 10, maxsim_oracle(dist, groups, ~tomb, off, 10), "g_chunks")
    finally:
        eng.close()


# ---------------------------------------------------------------- h. refusals at the entry
def test_the_entry_refuses_before_anything_is_launched():
    n, d = 100, 16
    rows, toks = make_case(95, n, d, 130)
    eng = _engine("l2", rows, np.arange(n, dtype=np.int64))
    eng.define_attr(1, "float64")
    lib = eng._lib
    try:
        eng.set_profiling(True)
        eng.last_stats()
        k = 65
        grp, s32, cnt = np.empty((2, k), np.int64), np.empty((2, k), np.float32), np.empty(2, np.int32)

        def call(off, k, attr, tokens=toks):
            off = np.asarray(off, np.int64)
            return lib.mlvdb_search_batch_maxsim(eng.handle, tokens.ctypes.data, off.ctypes.data, off.size - 1, k, attr, None,
                                                 grp.ctypes.data, s32.ctypes.data, cnt.ctypes.data, None, None, None)

        INVALID, UNSUPPORTED = 1, 6  # MLVDB_ERR_INVALID_ARG, MLVDB_ERR_UNSUPPORTED
        assert call([0, 1], 10, 1) == INVALID            # a float64 column
        assert call([0, 1], 10, 2) == INVALID            # an undefined column
        assert call([0, 1], 65, 0) == UNSUPPORTED        # k above MLVDB_MAX_TOPK
        assert call([0, 1], 0, 0) == INVALID
        assert call([0, 129], 10, 0) == INVALID          # 129 tokens
        assert call([1, 2], 10, 0) == INVALID            # does not start at 0
        assert call([0, 3, 3], 10, 0) == INVALID         # a query without tokens
        assert call([0, 3, 2], 10, 0) == INVALID         # descending
        assert lib.mlvdb_search_batch_maxsim(eng.handle, toks.ctypes.data, np.zeros(2, np.int64).ctypes.data, -1, 10, 0, None,
                                             grp.ctypes.data, s32.ctypes.data, cnt.ctypes.data, None, None, None) == INVALID
        assert lib.mlvdb_search_batch_maxsim(eng.handle, toks.ctypes.data, np.array([0, 1], np.int64).ctypes.data, 1, 10, 0,
                                             None, None, s32.ctypes.data, cnt.ctypes.data, None, None, None) == INVALID
        assert eng.last_stats()["scan_launches"] == 0    # nothing was launched for any of them
        assert call([0, 128], 10, 0) == 0 and cnt[0] == 10  # 128 tokens are served
    finally:
        eng.close()


def test_more_than_two_to_the_twenty_documents_overflow_and_exactly_that_many_are_served():
    from mlvectordb_amd.engine import MaxSimOverflow

    n, d = (1 << 20) + 1, 16
    rng = np.random.default_rng(96)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    toks = rows[[5, n - 2]] + np.float32(1e-3)
    eng = _engine("l2", rows, np.arange(n, dtype=np.int64) - 7)
    try:
        with pytest.raises(MaxSimOverflow):
            eng.search_maxsim(toks, offsets_of([1, 1]), 3, 0)
        eng.tombstone(np.array([9]))  # 2^20 documents are left
        grp, s32, cnt, s64, ml, md = eng.search_maxsim(toks, offsets_of([1, 1]), 3, 0, want_matches=True)
        eng.set_strategy("exact")
        lab, d32, pc, d64 = eng.search64(toks, 3)
        assert cnt.tolist() == [3, 3] and np.array_equal(ml, lab) and np.array_equal(grp, lab - 7) and ml[:, 0].tolist() == [5, n - 2]
        assert np.array_equal(s64.view(np.int64), d64.view(np.int64)) and np.array_equal(s32.view(np.int32), d32.view(np.int32))
    finally:
        eng.close()


def test_an_empty_index_answers_padding():
    eng = HipScanEngine(16, "l2", device=0)
    try:
        eng.define_attr(0, "int64")
        toks = np.ones((3, 16), np.float32)
        grp, s32, cnt, s64, ml, md = eng.search_maxsim(toks, offsets_of([2, 1]), 4, 0, want_matches=True)
        assert cnt.tolist() == [0, 0] and (grp == ABSENT).all() and np.isinf(s32).all() and np.isinf(s64).all()
        assert (ml == -1).all() and np.isinf(md).all()
    finally:
        eng.close()


# ---------------------------------------------------------------- i. protocol level
def test_search_late_and_find_documents_equal_the_oracle_index_on_a_str_column():
    rng = np.random.default_rng(97)
    n, d = 400, 24
    rows, toks = make_case(97, n, d, 7)
    titles = [f"doc-{int(v):03d}" if rng.random() < 0.9 else None for v in rng.integers(0, 60, n)]
    vectors = [VectorDTO(values=r.tolist(), metadata={"i": i} if t is None else {"i": i, "title": t})
               for i, (r, t) in enumerate(zip(rows, titles))]
    out = []
    for make in (lambda: Index(space="cosine", attributes={"title": "str"}), lambda: oracle_index({"title": "str"}, "cosine")):
        qp = QueryProcessor(InMemoryStorage(), make())
        qp.upsert_many(vectors)
        hits = qp._index.search_late([toks[:7], toks[:1]], 5, "default", "cosine", "title", matches=True)
        docs = qp.find_documents(toks[:7], 5, "default", "title", with_matches=True)
        plain = qp.find_documents(toks[:7], 5, "default", "title", where={"title": {"$ne": "doc-001"}})
        out.append((hits, docs, plain))
        qp._index.close()
    (hits, docs, plain), (whits, wdocs, wplain) = out
    assert hits.counts.tolist() == [5, 5] and np.array_equal(hits.values, whits.values)
    assert np.array_equal(hits.match_labels, whits.match_labels)
    assert np.abs(hits.scores - whits.scores).max() <= SCORE_ATOL * 7
    assert [x["value"] for x in docs] == [x["value"] for x in wdocs] == hits.values[0].tolist()
    assert [x["value"] for x in plain] == [x["value"] for x in wplain] and all("matches" not in x for x in plain)
    for got, want in zip(docs, wdocs):
        assert abs(got["score"] - want["score"]) <= SCORE_ATOL * 7
        assert [m["metadata"]["i"] for m in got["matches"]] == [m["metadata"]["i"] for m in want["matches"]]
        assert len(got["matches"]) == 7
        assert all(m["metadata"]["title"] == got["value"] for m in got["matches"])
        # the document's score is the sum of its matches' cosines
        assert abs(got["score"] - sum(m["score"] for m in got["matches"])) <= 1e-9
