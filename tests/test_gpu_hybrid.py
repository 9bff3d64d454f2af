"""Hybrid search on the MI355X (include/mlvdb_hybrid.h), at the engine level through the C ABI.
1. End to end against the pure model of tests/hybrid_helpers.py, bit for bit: dense components are small integers, sparse
   weights multiples of 1/8, the fusion weights and the RRF constant powers of two or small integers, so every leg value is
   exact in fp64 and the fused arithmetic -- one rounded operation per step on both sides -- must agree in all 64 bits.
2. A real-valued cosine case with no tolerance: every reported component against ``pair_distances`` and the sparse search's
   own score for the pair, and the fused score as NumPy fuses the two existing entries' lists with those components.
3. Edges, ``where``, the life cycle and the refusals.
2,003 x 64 rows (no multiple of 4, 64 or 256) appended in three batches, about 10 % tombstoned, about 10 % without a sparse
vector, some rows overwritten by label; rows of 0 / 1 / 15 / 16 / 17 / 255 nonzeros, terms 0 and 2^31 - 1, negative weights, and
terms t + 2^13 that alias a query's terms in the scorers' bitmap without being in the query."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.hybrid_helpers import METHODS, HybridOracleEngine, fuse_lists, fused_ties
from tests.sparse_helpers import TERM_MAX, exact_weight, random_corpus, random_vector, sparse_csr
from tests.tags_helpers import csr

pytestmark = pytest.mark.gpu

D = 64
SP, INT, FLT, TAGS = 0, 1, 2, 3  # the columns of every engine here; INT holds the row's own number: one program isolates a row
N = 2003
VOCAB = 64
CHUNK = _native.HYBRID_CHUNK
NAMES = ("labels", "fused", "counts", "dist64", "sparse64", "rank_dense", "rank_sparse")


def prog(ops, table=()):
    return W.Program(np.array(ops, dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def long_row(rng, exact):
    terms = list(range(VOCAB)) + list(range(10_000, 10_000 + 255 - VOCAB))
    return {t: (exact_weight(rng) if exact else float(np.float32(rng.standard_normal()) or 1.0)) for t in terms}


class Pair:
    """The HIP engine and the model, given the same calls."""

    def __init__(self, n, space, exact, seed=0, dead=0.1):
        self.rng = rng = np.random.default_rng(seed + n)
        self.exact, self.n, self.space = exact, n, space
        self.eng = HipScanEngine(D, space, device=0)
        self.model = HybridOracleEngine(D, space)
        for e in (self.eng, self.model):
            e.define_attr(SP, "sparse")
            e.define_attr(INT, "int64")
            e.define_attr(FLT, "float64")
            e.define_attr(TAGS, "int64_list")
        rows = (rng.integers(-4, 5, (n, D)).astype(np.float32) if exact else rng.standard_normal((n, D), dtype=np.float32))
        flts = rng.uniform(-1, 1, n)
        flts[rng.random(n) < 0.1] = np.nan
        tags = [None if i % 11 == 0 else sorted({int(t) for t in rng.integers(0, 6, int(rng.integers(0, 4)))}) for i in range(n)]
        vectors = random_corpus(rng, n, VOCAB, exact)
        if n > 8:
            for at in (4, n // 2, n - 1):
                vectors[at] = long_row(rng, exact)
            for at in range(5, n, 50):  # aliases of the queries' terms in the 8,192-bit bitmap, not in any query
                if vectors[at] is not None and len(vectors[at]) < 250:
                    for t in (1, 7, 63):
                        vectors[at][t + 2 ** 13] = exact_weight(rng) if exact else 1.25
        cuts = [0] + [n * (b + 1) // 3 for b in range(3)] if n >= 3 else [0, n]
        for lo, hi in zip(cuts[:-1], cuts[1:]):  # the rows and the pool both regrow on the way
            for e in (self.eng, self.model):
                assert e.append(rows[lo:hi]) == lo
                e.set_attr_sparse(SP, lo, sparse_csr(vectors[lo:hi]))
                e.set_attr(INT, lo, np.arange(lo, hi, dtype=np.int64))
                e.set_attr(FLT, lo, flts[lo:hi])
                e.set_attr_list(TAGS, lo, csr(tags[lo:hi]))
        gone = np.flatnonzero(rng.random(n) < dead) if n > 8 else np.zeros(0, np.int64)
        for e in (self.eng, self.model):
            e.tombstone(gone)
        if n > 8:  # overwritten by label: the old vectors stay behind in the pool as garbage
            labels = rng.choice(n, size=min(60, n // 4), replace=False).astype(np.int64)
            new = [None if i % 9 == 0 else {} if i % 9 == 1 else random_vector(rng, int(rng.integers(1, 20)), VOCAB, exact)
                   for i in range(labels.size)]
            got, want = self.both("set_attr_sparse_at", SP, labels, sparse_csr(new))
            assert got == want

    def close(self):
        self.eng.close()

    def both(self, entry, *args, **kw):
        return getattr(self.eng, entry)(*args, **kw), getattr(self.model, entry)(*args, **kw)

    def dense(self, nq):
        return (self.rng.integers(-4, 5, (nq, D)).astype(np.float32) if self.exact
                else self.rng.standard_normal((nq, D), dtype=np.float32))

    def sparse(self, nq):
        qs = [random_vector(self.rng, int(self.rng.integers(1, 33)), VOCAB, self.exact) for _ in range(nq)]
        qs[0][TERM_MAX] = -1.5
        qs[-1][0] = 2.0
        return qs

    def check(self, q, sq, k, fd, fs, method, weights=(1.0, 1.0), c=60.0, where=None, tag=""):
        """All seven outputs against the model, the floats in all 64 bits."""
        got, want = self.both("search_hybrid", q, SP, sparse_csr(sq), k, fd, fs, method=method, weights=weights, rrf_k=c,
                              where=where, components=True)
        for name, g, w in zip(NAMES, got, want):
            if g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
                bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))
                raise AssertionError(f"{tag} {method} k={k} fd={fd} fs={fs}: {name} differs in {bad.size} queries, first "
                                     f"{bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")
        lab3, fused3, cnt3 = self.eng.search_hybrid(q, SP, sparse_csr(sq), k, fd, fs, method=method, weights=weights, rrf_k=c,
                                                    where=where)
        assert np.array_equal(lab3, got[0]) and np.array_equal(_bits(fused3), _bits(got[1])) and np.array_equal(cnt3, got[2])
        return got


@pytest.fixture(scope="module")
def l2_pair():
    p = Pair(N, "l2", exact=True)
    yield p
    p.close()


@pytest.fixture(scope="module")
def ip_pair():
    p = Pair(N, "ip", exact=True, seed=2)
    yield p
    p.close()


@pytest.fixture(scope="module")
def cosine_pair():
    p = Pair(N, "cosine", exact=False, seed=1)
    yield p
    p.close()


# ---------------------------------------------------------------- exact inputs: bit for bit against the pure model
def test_the_corpus_holds_what_the_cases_need(l2_pair):
    rows, live = l2_pair.model.sparse_rows(SP), ~l2_pair.model._deleted
    lens = {len(r) for r, ok in zip(rows, live) if ok and r is not None}
    assert {0, 1, 15, 16, 17, 255} <= lens
    terms = {t for r, ok in zip(rows, live) if ok and r for t in r}
    assert {0, TERM_MAX, 1 + 2 ** 13, 63 + 2 ** 13} <= terms
    assert any(w < 0 for r in rows if r for w in r.values())
    absent = sum(r is None for r, ok in zip(rows, live) if ok)
    assert 100 < absent < 400 and 100 < l2_pair.eng.counts()[1] < 400
    used, alive = l2_pair.eng.list_stats(SP)
    assert (used, alive) == l2_pair.model.list_stats(SP) and used > alive
    assert l2_pair.eng.counts() == l2_pair.model.counts()


SHAPES = [(k, fd, fs) for k in (1, 10, 64) for fd in (1, 64, 65, 1024) for fs in (1, 64) if k <= fd + fs]
WEIGHTS = {"rrf": ((1.0, 2.0), 60.0), "linear": ((0.5, 4.0), 60.0), "relative": ((2.0, 1.0), 60.0)}


@pytest.mark.parametrize("space", ["l2", "ip"])
@pytest.mark.parametrize("method", METHODS)
def test_end_to_end_bit_for_bit(l2_pair, ip_pair, method, space):
    p = l2_pair if space == "l2" else ip_pair
    weights, c = WEIGHTS[method]
    absent = with_both = 0
    for i, (k, fd, fs) in enumerate(SHAPES):
        nq = (1, 7, 9)[i % 3]
        q, sq = p.dense(nq), p.sparse(nq)
        if i % 4 == 0:
            sq[nq // 2] = {}  # the sparse search's label-ordered zero-score list, no special case
        got = p.check(q, sq, k, fd, fs, method, weights, c, tag=f"{space} nq={nq}")
        lab, rs, ss = got[0], got[6], got[4]
        assert np.array_equal(got[2], np.minimum(k, p.model.search_hybrid(q, SP, sparse_csr(sq), fd + fs, fd, fs)[2]))
        rows = p.model.sparse_rows(SP)
        for qi, j in zip(*np.nonzero((lab >= 0) & (rs < 0))):
            if rows[lab[qi, j]] is None:  # only D contributes a row without a vector: its score is +0.0
                absent += 1
                assert _bits(ss)[qi, j] == 0
        with_both += int(((got[5] >= 0) & (rs >= 0)).sum())
    assert absent > 0 and with_both > 0


@pytest.mark.parametrize("method", METHODS)
def test_more_queries_than_one_chunk_and_a_1024_term_query(l2_pair, method):
    p = l2_pair
    nq = CHUNK + 3
    q, sq = p.dense(nq), p.sparse(nq)
    sq[CHUNK - 1] = {t: exact_weight(p.rng) for t in range(1024)}  # every term of the vocabulary and 960 no row holds
    sq[CHUNK] = {}
    weights, c = WEIGHTS[method]
    p.check(q, sq, 10, 40, 20, method, weights, c, tag="two chunks")


def test_ties_in_the_fused_score_go_to_the_lower_label(l2_pair):
    """Equal weights make RRF symmetric -- (rank_D, rank_S) = (a, b) and (b, a) fuse to the same bits -- and integer
    distances repeat: the model alone shows that these inputs do tie, so the label order is exercised, not masked."""
    p = l2_pair
    q, sq = p.dense(9), p.sparse(9)
    want = p.model.search_hybrid(q, SP, sparse_csr(sq), 64, 64, 64, method="rrf", weights=(1.0, 1.0), rrf_k=60.0)
    assert fused_ties(want[1], want[2]) > 0
    p.check(q, sq, 64, 64, 64, "rrf", (1.0, 1.0), 60.0, tag="rrf ties")
    want = p.model.search_hybrid(q, SP, sparse_csr([{}] * 9), 64, 64, 64, method="linear", weights=(1.0, 1.0))
    assert fused_ties(want[1], want[2]) > 0  # integer distances, no sparse score
    p.check(q, [{}] * 9, 64, 64, 64, "linear", (1.0, 1.0), tag="linear ties")


def test_a_zero_weight_reproduces_one_leg(l2_pair):
    p = l2_pair
    q, sq = p.dense(7), p.sparse(7)
    for method in ("linear", "relative"):
        got = p.check(q, sq, 64, 64, 64, method, (1.0, 0.0), tag="w_sparse = 0")
        dl, _, dc = p.eng.search(q, 64)
        assert np.array_equal(got[0], dl) and np.array_equal(got[5], np.tile(np.arange(64, dtype=np.int32), (7, 1)))  # = D
        got = p.check(q, sq, 64, 64, 64, method, (0.0, 1.0), tag="w_dense = 0")
        for i in range(7):  # the order of S over C: (score descending, label ascending)
            n = got[2][i]
            assert np.array_equal(np.lexsort((got[0][i, :n], -got[4][i, :n])), np.arange(n))
            in_s = got[6][i, :n] >= 0
            assert np.array_equal(got[6][i, :n][in_s], np.sort(got[6][i, :n][in_s]))
    got = p.check(q, sq, 64, 64, 64, "rrf", (1.0, 0.0), 0.0, tag="rrf w_sparse = 0")
    assert np.array_equal(got[0], p.eng.search(q, 64)[0])
    got = p.check(q, sq, 64, 64, 64, "rrf", (0.0, 1.0), 0.0, tag="rrf w_dense = 0")
    assert np.array_equal(got[0], p.eng.search_batch_sparse(SP, sparse_csr(sq), 64)[0])


# ---------------------------------------------------------------- real values: the completion and the fusion, no tolerance
def _pair_score(eng, sq, label, listed):
    """The score ``search_batch_sparse`` reports for (query, row): from the unfiltered list when the row is in it, else
    with k = 64 under the program that isolates the row; +0.0 when the row is no candidate (no vector)."""
    lab, s64 = listed
    at = np.flatnonzero(lab == label)
    if at.size:
        return s64[at[0]]
    lab, _, cnt, s64 = eng.search_batch_sparse(SP, sparse_csr([sq]), 64, prog([(W.EQ, INT, int(label), 0)]))
    assert cnt[0] <= 1 and (cnt[0] == 0 or lab[0, 0] == label)
    return s64[0, 0] if cnt[0] else 0.0


@pytest.mark.parametrize("method", METHODS)
def test_real_valued_cosine_components_are_the_other_entries_bits(cosine_pair, method):
    p, eng = cosine_pair, cosine_pair.eng
    nq, fd, fs, k = 3, 40, 24, 64  # k = fd + fs: every member of the union is a hit, every component is reported
    q, sq = p.dense(nq), p.sparse(nq)
    weights, c = ((0.75, 1.3), 7.5)
    lab, fused, cnt, d64, s64, rd, rs = eng.search_hybrid(q, SP, sparse_csr(sq), k, fd, fs, method=method, weights=weights,
                                                          rrf_k=c, components=True)
    dl, _, dc, dd64 = eng.search64(q, fd)
    sl, _, sc, ss64 = eng.search_batch_sparse(SP, sparse_csr(sq), fs)
    full = eng.search_batch_sparse(SP, sparse_csr(sq), 64)
    pd = eng.pair_distances(q, np.where(lab >= 0, lab, 0))[0]
    completed = 0
    for i in range(nq):
        n = cnt[i]
        assert n == np.union1d(dl[i, :dc[i]], sl[i, :sc[i]]).size and (rd[i, :n] < 0).any() and (rs[i, :n] < 0).any()
        assert np.array_equal(_bits(d64[i, :n]), _bits(pd[i, :n]))
        for j in range(n):
            want = _pair_score(eng, sq[i], lab[i, j], (full[0][i], full[3][i]))
            assert _bits(s64[i, j:j + 1])[0] == _bits(np.array([want]))[0], (i, j, lab[i, j])
            completed += rs[i, j] < 0 and want != 0.0
    assert completed > 0  # the gathered scorer produced scores of rows the sparse list does not hold
    at = {(i, int(l)): j for i in range(nq) for j, l in enumerate(lab[i, :cnt[i]])}
    want = fuse_lists(dl, dd64, dc, sl, ss64, sc, lambda i, ls: np.array([d64[i, at[i, int(l)]] for l in ls]),
                      lambda i, ls: np.array([s64[i, at[i, int(l)]] for l in ls]), k, method, weights, c)
    for name, g, w in zip(NAMES, (lab, fused, cnt, d64, s64, rd, rs), want):
        assert np.array_equal(_bits(g), _bits(w)), name


def test_rrf_without_components_skips_nothing_that_shows(cosine_pair):
    p = cosine_pair
    q, sq = p.dense(9), p.sparse(9)
    a = p.eng.search_hybrid(q, SP, sparse_csr(sq), 20, 100, 64, method="rrf", components=True)
    b = p.eng.search_hybrid(q, SP, sparse_csr(sq), 20, 100, 64, method="rrf")
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------- edges
def _ordered(n, sparse_descending, absent=(), dense_equal=False):
    """Row i has the dense vector (i, 0, ...) -- the zero query ranks the rows by number -- and the sparse vector
    {1: n - i} / 8 (descending: the sparse ranking is the dense one) or {1: i + 1} / 8 (the reverse)."""
    rows = np.zeros((n, D), np.float32)
    if not dense_equal:
        rows[:, 0] = np.arange(n)
    vectors = [None if i in absent else {1: ((n - i) if sparse_descending else (i + 1)) / 8.0} for i in range(n)]
    eng, model = HipScanEngine(D, "l2", device=0), HybridOracleEngine(D, "l2")
    for e in (eng, model):
        e.define_attr(SP, "sparse")
        e.append(rows)
        e.set_attr_sparse(SP, 0, sparse_csr(vectors))
    return eng, model


def _same(eng, model, q, sq, k, fd, fs, method, weights=(1.0, 1.0), c=1.0):
    got = eng.search_hybrid(q, SP, sparse_csr(sq), k, fd, fs, method=method, weights=weights, rrf_k=c, components=True)
    want = model.search_hybrid(q, SP, sparse_csr(sq), k, fd, fs, method=method, weights=weights, rrf_k=c, components=True)
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(_bits(g), _bits(w)), (name, method, k, fd, fs)
    return got


def test_overlap_and_union_sizes():
    q, sq = np.zeros((2, D), np.float32), [{1: 1.0}, {1: 2.0}]
    eng, model = _ordered(1200, sparse_descending=True, absent=(3,))
    try:
        for method in METHODS:
            got = _same(eng, model, q, sq, 2, 1, 1, method)  # identical lists: |C| = 1
            assert got[2].tolist() == [1, 1] and (got[5][:, 0] == 0).all() and (got[6][:, 0] == 0).all()
            got = _same(eng, model, q, sq, 64, 64, 64, method)  # D = rows 0..63, S = rows 0..64 without row 3: |C| = 65
            assert (got[2] == 64).all()
            assert model.search_hybrid(q, SP, sparse_csr(sq), 128, 64, 64, method=method)[2].tolist() == [65, 65]
            at = np.flatnonzero(got[0][0] == 3)  # row 3 has no vector: only D holds it
            assert at.size == 1 and got[6][0, at[0]] == -1 and _bits(got[4])[0, at[0]] == 0 and got[5][0, at[0]] == 3
            got = _same(eng, model, q, sq, 64, 64, 63, method)  # S = rows 0..63 without row 3, all of them in D: |C| = 64
            assert model.search_hybrid(q, SP, sparse_csr(sq), 127, 64, 63, method=method)[2].tolist() == [64, 64]
            got = _same(eng, model, q, sq, 10, 5, 10, method)  # partial: D inside S
            assert ((got[5] >= 0) | (got[6] >= 0)).all()
    finally:
        eng.close()
    eng, model = _ordered(1200, sparse_descending=False)
    try:
        for method in METHODS:
            got = _same(eng, model, q, sq, 64, 1024, 64, method)  # disjoint: D = rows 0..1023, S = rows 1199..1136
            assert model.search_hybrid(q, SP, sparse_csr(sq), 1088, 1024, 64, method=method)[2].tolist() == [1088, 1088]
            assert ((got[5] >= 0) != (got[6] >= 0)).all()
            got = _same(eng, model, q, sq, 64, 1, 64, method)  # |C| = 65, disjoint
            assert ((got[5] >= 0) != (got[6] >= 0)).all() and (got[2] == 64).all()
    finally:
        eng.close()


def test_relative_with_equal_components():
    q = np.zeros((2, D), np.float32)
    eng, model = _ordered(300, sparse_descending=True, dense_equal=True)
    try:
        got = _same(eng, model, q, [{1: 1.0}, {1: -1.0}], 20, 30, 10, "relative", (4.0, 1.0))  # dmax == dmin: nd = 0
        assert (got[3] == 0.0).all() and got[1][0, 0] == 1.0 and got[0][0, 0] == 0
    finally:
        eng.close()
    eng, model = _ordered(300, sparse_descending=True)
    try:
        got = _same(eng, model, q, [{}, {2: 1.0}], 20, 30, 10, "relative", (4.0, 1.0))  # smax == smin: ns = 0
        assert (_bits(got[4]) == 0).all() and got[1][0, 0] == 4.0 and got[0][0].tolist() == list(range(20))
    finally:
        eng.close()


@pytest.mark.parametrize("method", METHODS)
def test_an_index_of_five_rows(method):
    p = Pair(5, "l2", exact=True, seed=3)
    try:
        q, sq = p.dense(3), [p.sparse(1)[0], {}, {3: 1.0}]
        for k, fd, fs in ((1, 1, 1), (5, 5, 5), (64, 1024, 64), (64, 3, 64)):
            got = p.check(q, sq, k, fd, fs, method, tag="5 rows")
            assert (got[0][:, 5:] == -1).all() and np.isneginf(got[1][:, 5:]).all()
    finally:
        p.close()


def test_an_empty_index_and_a_dead_one_answer_padding():
    eng = HipScanEngine(D, "l2", device=0)
    try:
        eng.define_attr(SP, "sparse")
        q, sq = np.ones((2, D), np.float32), sparse_csr([{1: 1.0}, {}])
        for state in ("empty", "no values", "all dead"):
            if state == "no values":
                eng.append(np.ones((300, D), np.float32))
                got = eng.search_hybrid(q, SP, sq, 5, 10, 10, method="linear", components=True)
                assert (got[2] == 5).all() and (got[6] == -1).all() and (_bits(got[4]) == 0).all()  # D alone
                continue
            if state == "all dead":
                eng.tombstone(np.arange(300))
            for method in METHODS:
                lab, fused, cnt, d64, s64, rd, rs = eng.search_hybrid(q, SP, sq, 5, 10, 10, method=method, components=True)
                assert (lab == -1).all() and (cnt == 0).all() and np.isneginf(fused).all() and np.isposinf(d64).all(), state
                assert np.isneginf(s64).all() and (rd == -1).all() and (rs == -1).all(), state
        assert eng.search_hybrid(q[:0], SP, sparse_csr([]), 5, 10, 10)[0].shape == (0, 5)
    finally:
        eng.close()


# ---------------------------------------------------------------- where
def test_one_program_restricts_both_legs(l2_pair):
    p = l2_pair
    q, sq = p.dense(9), p.sparse(9)
    lit = np.array([0.25]).view(np.int64)[0]
    programs = {
        "int range": prog([(W.GE, INT, 500, 0), (W.LT, INT, 1500, 0), (W.AND, 0, 0, 0)]),
        "float lt or int in": prog([(W.LT, FLT, int(lit), 0), (W.IN, INT, 0, 2), (W.OR, 0, 0, 0)], [0, 5]),
        "tag": prog([(W.HAS, TAGS, 3, 0)]),
        "tags any": prog([(W.HAS_ANY, TAGS, 0, 2)], [1, 4]),
        "exists": prog([(W.EXISTS, SP, 0, 0)]),
        "not exists": prog([(W.EXISTS, SP, 0, 0), (W.NOT, 0, 0, 0)]),  # S is empty: the union is D
        "size 15..17": prog([(W.LEN, SP, 15, 17)]),
        "nothing": prog([(W.TRUE, 0, 0, 0), (W.NOT, 0, 0, 0)]),
        "few rows": prog([(W.IN, INT, 0, 3)], [7, 8, 9]),
    }
    for tag, w in programs.items():
        inside = p.model.match(w)
        for method in METHODS:
            weights, c = WEIGHTS[method]
            got = p.check(q, sq, 20, 30, 25, method, weights, c, where=w, tag=tag)
            lab = got[0][got[0] >= 0]
            assert inside[lab].all(), tag
        if tag == "nothing":
            assert (got[0] == -1).all() and (got[2] == 0).all()
        if tag == "not exists":
            assert (got[6] == -1).all() and (got[2] == 20).all()
    p.check(q, sq, 20, 30, 25, "rrf", tag="no program afterwards")


# ---------------------------------------------------------------- life cycle
def test_life_cycle():
    p = Pair(700, "l2", exact=True, seed=5)
    try:
        q, sq = p.dense(9), p.sparse(9) + [{}]
        q = np.concatenate([q, p.dense(1)])
        w = prog([(W.GE, INT, 100, 0)])

        def check(tag):
            for method in METHODS:
                weights, c = WEIGHTS[method]
                p.check(q, sq, 10, 40, 20, method, weights, c, tag=tag)
                p.check(q, sq, 64, 100, 64, method, weights, c, where=w, tag=tag + " where")
            assert p.eng.counts() == p.model.counts() and p.eng.list_stats(SP) == p.model.list_stats(SP), tag

        check("built")
        gone = p.rng.choice(700, 150, replace=False)
        for e in (p.eng, p.model):
            e.tombstone(gone)
        check("tombstoned")
        used, live = p.eng.list_stats(SP)
        assert used > live  # pool_used > pool_live before the compaction
        old, want_old = p.both("compact")
        assert np.array_equal(old, want_old) and p.eng.list_stats(SP) == (live, live)
        for e in (p.eng, p.model):  # (INT stays the row's own number: the programs above mean the same rows in both)
            e.set_attr(INT, 0, np.arange(old.size, dtype=np.int64))
        check("compacted")
        labels = np.arange(0, 200, 3, dtype=np.int64)
        new = [None if i % 5 == 0 else random_vector(p.rng, 6, VOCAB, True) for i in range(labels.size)]
        assert p.both("set_attr_sparse_at", SP, labels, sparse_csr(new)) == (labels.size, labels.size)
        check("overwritten by label")
    finally:
        p.close()


# ---------------------------------------------------------------- refusals: a status code, nothing written
def _raw(eng, q, offsets, terms, weights, k, fd, fs, method=0, wd=1.0, ws=1.0, c=60.0, attr=SP, where=None, null=()):
    lib = _native.load()
    q = np.ascontiguousarray(q, np.float32)
    offsets = np.asarray(offsets, np.int64)
    terms, weights = np.asarray(terms, np.int32), np.asarray(weights, np.float32)
    nq, kk = offsets.size - 1, max(k, 1)
    out = {"labels": np.full((nq, kk), 77, np.int64), "fused": np.full((nq, kk), 77.0), "counts": np.full(nq, 77, np.int32),
           "d64": np.full((nq, kk), 77.0), "s64": np.full((nq, kk), 77.0), "rd": np.full((nq, kk), 77, np.int32),
           "rs": np.full((nq, kk), 77, np.int32)}
    ptr = {n: (None if n in null else a.ctypes.data) for n, a in out.items()}
    wh = None
    if where is not None:
        wh, keep = HipScanEngine._where(where)
    rc = lib.mlvdb_search_batch_hybrid(eng.handle, None if "queries" in null else q.ctypes.data, attr,
                                       None if "offsets" in null else offsets.ctypes.data, terms.ctypes.data,
                                       weights.ctypes.data, nq, k, fd, fs, method, wd, ws, c,
                                       None if wh is None else C.byref(wh), ptr["labels"], ptr["fused"], ptr["counts"],
                                       ptr["d64"], ptr["s64"], ptr["rd"], ptr["rs"])
    untouched = all((a == 77).all() for a in out.values())
    return rc, untouched


def test_refusals_leave_the_outputs_and_the_handle_as_they_were(l2_pair):
    p, eng = l2_pair, l2_pair.eng
    q1 = np.ones((1, D), np.float32)
    nan_q = q1.copy()
    nan_q[0, 5] = np.nan
    ok = dict(q=q1, offsets=[0, 1], terms=[5], weights=[1.0], k=3, fd=10, fs=10)

    def call(**kw):
        return _raw(eng, **{**ok, **kw})

    invalid = {
        "int column": dict(attr=INT), "list column": dict(attr=TAGS), "undefined column": dict(attr=9), "attr -1": dict(attr=-1),
        "k = 0": dict(k=0), "fetch_dense = 0": dict(fd=0), "fetch_sparse = 0": dict(fs=0), "fetch_sparse < 0": dict(fs=-1),
        "k above the sum": dict(k=5, fd=2, fs=2),
        "method 3": dict(method=3), "method -1": dict(method=-1),
        "w_dense < 0": dict(wd=-1.0), "w_sparse nan": dict(ws=np.nan), "w_dense inf": dict(wd=np.inf), "w_sparse -inf": dict(ws=-np.inf),
        "c < 0": dict(c=-0.5), "c nan": dict(c=np.nan), "c inf": dict(c=np.inf),
        "nan in the dense query": dict(q=nan_q),
        "query of 1025 terms": dict(offsets=[0, 1025], terms=list(range(1025)), weights=[1.0] * 1025),
        "unsorted query": dict(offsets=[0, 2], terms=[5, 4], weights=[1.0, 1.0]),
        "nan query weight": dict(weights=[np.nan]), "inf query weight": dict(weights=[-np.inf]),
        "negative query term": dict(terms=[-5]),
        "offsets not from 0": dict(offsets=[1, 2], terms=[5, 6], weights=[1.0, 1.0]),
        "decreasing offsets": dict(q=np.ones((2, D), np.float32), offsets=[0, 1, 0]),
        "null queries": dict(null=("queries",)), "null offsets": dict(null=("offsets",)), "null labels": dict(null=("labels",)),
        "null fused": dict(null=("fused",)), "null counts": dict(null=("counts",)),
        "bad program": dict(where=prog([(W.EQ, SP, 1, 0)])),
        "unbalanced program": dict(where=prog([(W.AND, 0, 0, 0)])),
    }
    for tag, kw in invalid.items():
        assert call(**kw) == (1, True), tag  # MLVDB_ERR_INVALID_ARG
    unsupported = {"k = 65": dict(k=65, fd=100), "fetch_dense = 1025": dict(fd=1025), "fetch_sparse = 65": dict(fs=65)}
    for tag, kw in unsupported.items():
        assert call(**kw) == (6, True), tag  # MLVDB_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match=r"failed \(1\)"):
        eng.search_hybrid(q1, INT, sparse_csr([{1: 1.0}]), 3, 10, 10)
    assert call() == (0, False) and call(k=64, fd=1024, fs=64, null=("d64", "s64", "rd", "rs"))[0] == 0
    assert call(q=np.ones((0, D), np.float32), offsets=[0], terms=[], weights=[]) == (0, True)  # nq = 0
    # the handle answers as before
    q = p.dense(7)
    got, want = p.both("search", q, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    p.check(q, p.sparse(7), 10, 40, 20, "linear", tag="after the refusals")
