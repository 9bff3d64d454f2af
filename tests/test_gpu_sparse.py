"""Sparse vector columns on the MI355X (include/mlvdb_sparse.h), at the engine level through the C ABI: every call is made
on a ``HipScanEngine`` and on the model engine of tests/sparse_helpers.py (vectors as Python dicts, scores by NumPy fp64
over a dense matrix), and the answers are compared.  2,003 x 64 rows (no multiple of 4, 64 or 256) appended in three
batches, about 10 % tombstoned, about 10 % without a vector, some rows overwritten by label."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.sparse_helpers import (TERM_MAX, SparseOracleEngine, dense_scores, exact_weight, random_corpus, random_vector,
                                  sparse_csr, sparse_uncsr)

pytestmark = pytest.mark.gpu

D = 64
SP, INT, FLT = 0, 1, 2  # the columns of every engine here
N = 2003
ONE = 7      # the one row whose int value is UNIQUE (kept live, with a vector)
UNIQUE = 99
EPS = 2 * 255 * 2.0 ** -53  # reordering 255 fp64 additions: |error| <= EPS * sum |wq * wr|


def prog(ops, table=()):
    return W.Program(np.array(ops, dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


def long_row(rng, vocab, exact):
    """255 nonzeros: the whole small vocabulary and terms beyond it."""
    terms = list(range(min(vocab, 200))) + list(range(10_000, 10_000 + 255 - min(vocab, 200)))
    return {t: (exact_weight(rng) if exact else float(np.float32(rng.standard_normal()) or 1.0)) for t in terms}


class Pair:
    """The HIP engine and the model, given the same calls."""

    def __init__(self, n, vocab, exact, seed=0, batches=3, dead=0.1):
        self.rng = rng = np.random.default_rng(seed + n)
        self.vocab, self.exact, self.n = vocab, exact, n
        self.eng = HipScanEngine(D, "ip", device=0)
        self.model = SparseOracleEngine(D, "ip")
        for e in (self.eng, self.model):
            e.define_attr(SP, "sparse")
            e.define_attr(INT, "int64")
            e.define_attr(FLT, "float64")
        rows = rng.standard_normal((n, D), dtype=np.float32)
        ints = rng.integers(-2, 6, n).astype(np.int64)
        ints[rng.random(n) < 0.1] = W.INT64_ABSENT
        flts = rng.uniform(-1, 1, n)
        flts[rng.random(n) < 0.1] = np.nan
        vectors = random_corpus(rng, n, vocab, exact)
        if n > 8:
            for at in (4, n // 2, n - 1):
                vectors[at] = long_row(rng, vocab, exact)
            vectors[ONE] = random_vector(rng, 5, vocab, exact)
            ints[ONE] = UNIQUE
        cuts = [0] + [n * (b + 1) // batches for b in range(batches)] if n >= batches else [0, n]
        for lo, hi in zip(cuts[:-1], cuts[1:]):  # the rows and the pool both regrow on the way
            for e in (self.eng, self.model):
                assert e.append(rows[lo:hi]) == lo
                e.set_attr_sparse(SP, lo, sparse_csr(vectors[lo:hi]))
                e.set_attr(INT, lo, ints[lo:hi])
                e.set_attr(FLT, lo, flts[lo:hi])
        gone = np.flatnonzero(rng.random(n) < dead) if n > 8 else np.zeros(0, np.int64)
        gone = gone[gone != ONE]
        for e in (self.eng, self.model):
            e.tombstone(gone)
        if n > 8:  # overwritten by label: the old vectors stay behind in the pool as garbage (tombstoned rows are skipped)
            labels = rng.choice(np.setdiff1d(np.arange(n), [ONE]), size=min(60, n // 4), replace=False).astype(np.int64)
            new = [None if i % 9 == 0 else {} if i % 9 == 1 else random_vector(rng, int(rng.integers(1, 20)), vocab, exact)
                   for i in range(labels.size)]
            got, want = self.both("set_attr_sparse_at", SP, labels, sparse_csr(new))
            assert got == want

    def close(self):
        self.eng.close()

    def both(self, method, *args, **kw):
        return getattr(self.eng, method)(*args, **kw), getattr(self.model, method)(*args, **kw)

    def query(self, length, terms=None):
        return random_vector(self.rng, length, self.vocab, self.exact, terms)

    def check_exact(self, queries, k, where=None, tag=""):
        """Labels, counts and the 64 bits of every score against the model."""
        (lab, s32, cnt, s64), (ol, o32, oc, o64) = self.both("search_batch_sparse", SP, sparse_csr(queries), k, where)
        assert np.array_equal(cnt, oc), f"{tag}: counts"
        assert np.array_equal(lab, ol), f"{tag}: labels"
        assert np.array_equal(s64.view(np.int64), o64.view(np.int64)), f"{tag}: score64 bits"
        assert np.array_equal(s32.view(np.int32), o32.view(np.int32)), f"{tag}: float scores"
        return lab, s64, cnt


@pytest.fixture(scope="module")
def exact_pair():
    p = Pair(N, 64, exact=True)
    yield p
    p.close()


@pytest.fixture(scope="module")
def real_pair():
    p = Pair(N, 4096, exact=False, seed=1)
    yield p
    p.close()


# ---------------------------------------------------------------- exact weights: bit for bit, ties decided by the label
def test_the_corpus_holds_what_the_cases_need(exact_pair):
    rows, live = exact_pair.model.sparse_rows(SP), ~exact_pair.model._deleted
    lens = {len(r) for r, ok in zip(rows, live) if ok and r is not None}
    assert {0, 1, 15, 16, 17, 255} <= lens
    terms = {t for r, ok in zip(rows, live) if ok and r for t in r}
    assert {0, TERM_MAX} <= terms
    assert any(w < 0 for r in rows if r for w in r.values()) and any(r is None for r in rows)
    used, alive = exact_pair.eng.list_stats(SP)
    assert (used, alive) == exact_pair.model.list_stats(SP) and used > alive  # garbage of the rows overwritten by label
    assert exact_pair.eng.counts() == exact_pair.model.counts() and exact_pair.eng.counts()[1] > 100


@pytest.mark.parametrize("k", [1, 10, 64])
def test_exact_scores_bit_for_bit(exact_pair, k):
    p = exact_pair
    for nq in (1, 7, 8, 9, 17):
        queries = [p.query(int(p.rng.integers(1, 33))) for _ in range(nq)]
        queries[0][TERM_MAX] = -1.5
        queries[-1][0] = 2.0
        lab, s64, cnt = p.check_exact(queries, k, tag=f"k={k} nq={nq}")
        assert (cnt == k).all()
    if k == 10:  # ties are abundant at 64 terms of eighths: the label decides, and a zero is +0.0
        lab, s64, cnt = p.check_exact([{5: 1.0}], 64, tag="ties")
        assert (np.diff(s64[0]) == 0).sum() > 10 and not np.signbit(s64[s64 == 0]).any()


def test_real_weights_within_the_reordering_bound(real_pair):
    p = real_pair
    for nq, k in ((1, 10), (9, 1), (17, 64), (8, 10)):
        # every other query is long and drawn from the first 400 terms: it shares a hundred and more terms with the rows of
        # 255 nonzeros, so the order of the additions matters
        queries = [p.query(int(p.rng.integers(1, 65))) if i % 2 else p.query(int(p.rng.integers(100, 250)), np.arange(400))
                   for i in range(nq)]
        lab, s32, cnt, s64 = p.eng.search_batch_sparse(SP, sparse_csr(queries), k)
        scores, mass = dense_scores(queries, p.model.sparse_rows(SP))
        cand = p.model.candidates(SP)
        assert (cnt == min(k, int(cand.sum()))).all()
        for q in range(nq):  # no query is skipped
            got, s = lab[q, :cnt[q]], s64[q, :cnt[q]]
            assert cand[got].all() and np.unique(got).size == got.size
            bound = EPS * mass[q]
            print(f"nq={nq} k={k} q={q}: worst error {np.abs(s - scores[q, got]).max():.3e}, bound there "
                  f"{bound[got][np.abs(s - scores[q, got]).argmax()]:.3e}")
            assert (np.abs(s - scores[q, got]) <= bound[got]).all()
            order = np.lexsort((got, -s))
            assert np.array_equal(order, np.arange(got.size)), "sorted by (-score64, label)"
            # the model's k-th best row m is returned, or every returned row beat it by the GPU's own score of m, which
            # is within m's bound of the model's
            idx = np.flatnonzero(cand)
            kth = idx[np.lexsort((idx, -scores[q, idx]))][cnt[q] - 1]
            assert (s >= scores[q, kth] - bound[kth]).all()
            assert np.array_equal(s32[q, :cnt[q]], s.astype(np.float32))


# ---------------------------------------------------------------- tiles
def test_tile_splits_long_queries_and_an_empty_one(exact_pair):
    p = exact_pair
    wide = np.arange(0, 6000)
    # five queries of 300 terms: their union passes 1024 terms after the third, the tile splits early
    p.check_exact([p.query(300, wide) for _ in range(5)], 10, tag="300 terms each")
    # a full query beside one-term queries, and past it
    full = p.query(1024, wide)
    assert len(full) == 1024
    p.check_exact([{3: 1.0}, full, {0: -2.0}, {TERM_MAX: 0.5}, full, {63: 1.0}], 10, tag="1024 beside 1")
    # an empty query ranks the candidates by label, every score +0.0
    lab, s64, cnt = p.check_exact([{}, p.query(4), {}], 64, tag="empty")
    assert (s64[0] == 0).all() and not np.signbit(s64[0]).any() and (np.diff(lab[0]) > 0).all()
    assert np.array_equal(lab[0], np.flatnonzero(p.model.candidates(SP))[:64])


def test_more_queries_than_one_pass_takes(exact_pair):
    """A call is served in passes of 256 queries: 257 and 600 queries cross the boundary once and twice."""
    p = exact_pair
    queries = [p.query(int(p.rng.integers(0, 12))) for _ in range(600)]
    p.check_exact(queries[:257], 3, tag="257 queries")
    p.check_exact(queries, 10, prog([(W.GE, INT, 0, 0)]), tag="600 queries, where")


def test_a_pairs_score_does_not_depend_on_the_batch(real_pair):
    p = real_pair
    q = p.query(40)
    others = [p.query(int(p.rng.integers(1, 200))) for _ in range(20)]
    seen = {}

    def note(queries, at, k, where=None):
        lab, _, cnt, s64 = p.eng.search_batch_sparse(SP, sparse_csr(queries), k, where)
        for l, bits in zip(lab[at, :cnt[at]].tolist(), s64[at, :cnt[at]].view(np.int64).tolist()):
            assert seen.setdefault(l, bits) == bits, f"label {l}: {bits:#x} != {seen[l]:#x}"
        return cnt[at]

    assert note([q], 0, 64) == 64
    note([q], 0, 10)
    note(others[:3] + [q] + others[3:6], 3, 64)       # another place in its tile, other queries around it
    note(others[:8] + [q], 8, 64)                     # alone in the second tile
    note(others + [q], 20, 64)                        # the last of many
    note([q, q], 1, 64)
    note([q] + others[:2], 0, 64, prog([(W.GE, INT, 0, 0)]))
    note(others[5:9] + [q], 4, 30, prog([(W.LEN, SP, 1, 255)]))
    assert len(seen) > 64


def test_terms_that_alias_in_the_bitmap_score_exactly_zero():
    terms = [3, 100, 8191]
    rows = [{t + 2 ** m: exact_weight(np.random.default_rng(m)) for t in terms} for m in range(10, 31)]
    rows += [{3: 1.0, 3 + 2 ** 13: 5.0}, {2 ** 13: 1.0, 2 ** 14: 1.0}, {}]
    assert all(t < 2 ** 31 for r in rows for t in r)
    eng, model = HipScanEngine(D, "ip", device=0), SparseOracleEngine(D, "ip")
    try:
        for e in (eng, model):
            e.define_attr(SP, "sparse")
            e.append(np.ones((len(rows), D), np.float32))
            e.set_attr_sparse(SP, 0, sparse_csr(rows))
        q = sparse_csr([{t: 2.0 for t in terms}, {3: 1.0}])
        lab, _, cnt, s64 = eng.search_batch_sparse(SP, q, 64)
        ol, _, oc, o64 = model.search_batch_sparse(SP, q, 64)
        assert np.array_equal(lab, ol) and np.array_equal(cnt, oc) and np.array_equal(s64.view(np.int64), o64.view(np.int64))
        assert s64[0, 0] == 2.0 and lab[0, 0] == 21 and (s64[0, 1:cnt[0]].view(np.int64) == 0).all()
    finally:
        eng.close()


# ---------------------------------------------------------------- where
def test_where_programs(exact_pair):
    p = exact_pair
    queries = [p.query(int(p.rng.integers(1, 20))) for _ in range(9)]
    lit = np.array([0.25]).view(np.int64)[0]
    programs = {
        "int eq": prog([(W.EQ, INT, 3, 0)]),
        "float lt or int in": prog([(W.LT, FLT, int(lit), 0), (W.IN, INT, 0, 2), (W.OR, 0, 0, 0)], [0, 5]),
        "exists": prog([(W.EXISTS, SP, 0, 0)]),
        "not exists": prog([(W.EXISTS, SP, 0, 0), (W.NOT, 0, 0, 0)]),  # no candidate has no vector
        "size 15..17": prog([(W.LEN, SP, 15, 17)]),
        "empty": prog([(W.LEN, SP, 0, 0)]),
        "size and int": prog([(W.LEN, SP, 1, 255), (W.GE, INT, 2, 0), (W.AND, 0, 0, 0)]),
        "nothing": prog([(W.TRUE, 0, 0, 0), (W.NOT, 0, 0, 0)]),
        "one row": prog([(W.EQ, INT, UNIQUE, 0)]),
    }
    for tag, w in programs.items():
        for k in (1, 64):
            lab, s64, cnt = p.check_exact(queries, k, w, tag=f"{tag} k={k}")
        want = int((p.model.match(w) & p.model.candidates(SP)).sum())
        assert (cnt == min(64, want)).all(), tag
        if tag in ("nothing", "not exists"):
            assert want == 0 and (lab == -1).all() and np.isneginf(s64).all()
        if tag == "one row":
            assert want == 1 and (lab[:, 0] == ONE).all() and (lab[:, 1:] == -1).all()
        got, expect = p.both("where_count", w)
        assert got == expect, tag


# ---------------------------------------------------------------- small indexes
@pytest.mark.parametrize("n, k", [(1, 1), (1, 64), (3, 2), (3, 64), (5, 64)])
def test_fewer_candidates_than_k(n, k):
    p = Pair(n, 16, exact=True, seed=3, batches=1)
    try:
        lab, s64, cnt = p.check_exact([p.query(3), {}, p.query(16)], k, tag=f"n={n} k={k}")
        have = int(p.model.candidates(SP).sum())
        assert (cnt == min(k, have)).all() and (lab[:, min(k, have):] == -1).all()
    finally:
        p.close()


def test_an_empty_index_and_a_column_without_values_answer_padding():
    eng = HipScanEngine(D, "ip", device=0)
    try:
        eng.define_attr(SP, "sparse")
        q = sparse_csr([{1: 1.0}, {}])
        for state in ("empty", "no values", "all dead", "reset"):
            if state == "no values":
                eng.append(np.ones((300, D), np.float32))
            elif state == "all dead":
                eng.set_attr_sparse(SP, 0, sparse_csr([{1: 1.0}] * 300))
                assert eng.search_batch_sparse(SP, q, 5)[2].tolist() == [5, 5]
                eng.tombstone(np.arange(300))
            elif state == "reset":
                eng.reset()
            lab, s32, cnt, s64 = eng.search_batch_sparse(SP, q, 5)
            assert (lab == -1).all() and (cnt == 0).all() and np.isneginf(s64).all() and np.isneginf(s32).all(), state
    finally:
        eng.close()


# ---------------------------------------------------------------- life cycle
def test_life_cycle():
    p = Pair(700, 64, exact=True, seed=5)
    try:
        queries = [p.query(int(p.rng.integers(1, 24))) for _ in range(9)] + [{}]
        w = prog([(W.GE, INT, 1, 0)])

        def check(tag):
            p.check_exact(queries, 10, tag=tag)
            p.check_exact(queries, 64, w, tag=tag + " where")
            total = p.model.counts()[0]
            assert p.eng.counts() == p.model.counts(), tag
            got, want = p.both("get_attr_sparse", SP, 0, total)
            assert sparse_uncsr(got) == sparse_uncsr(want), tag  # absent (None) and empty ({}) told apart
            assert np.array_equal(got.present, want.present) and (got.present == 0).any() and got.terms.dtype == np.int32
            assert p.eng.list_stats(SP) == p.model.list_stats(SP), tag

        check("built")
        more = random_corpus(p.rng, 333, 64, True)
        block = p.rng.standard_normal((333, D), dtype=np.float32)
        for e in (p.eng, p.model):  # append (rows and pool regrow) -> search
            assert e.append(block) == 700
            e.set_attr_sparse(SP, 700, sparse_csr(more))
        check("appended")
        gone = p.rng.choice(1033, 150, replace=False)
        for e in (p.eng, p.model):
            e.tombstone(gone)
        check("tombstoned")
        used, live = p.eng.list_stats(SP)
        assert used > live
        old, want_old = p.both("compact")
        assert np.array_equal(old, want_old)
        assert p.eng.list_stats(SP)[0] == p.eng.list_stats(SP)[1] == live
        check("compacted")
        # the identity compaction sheds the garbage of an overwrite too
        labels = np.arange(0, 200, 3, dtype=np.int64)
        new = [random_vector(p.rng, 6, 64, True) for _ in labels]
        assert p.both("set_attr_sparse_at", SP, labels, sparse_csr(new)) == (labels.size, labels.size)
        used, live = p.eng.list_stats(SP)
        assert used > live
        old, want_old = p.both("compact")
        assert np.array_equal(old, want_old) and np.array_equal(old, np.arange(old.size))
        assert p.eng.list_stats(SP) == (live, live)
        check("identity compaction")
        # a partial read-back
        got, want = p.both("get_attr_sparse", SP, 100, 50)
        assert sparse_uncsr(got) == sparse_uncsr(want)
    finally:
        p.close()


def test_reset_then_append_then_search():
    p = Pair(300, 64, exact=True, seed=6)
    try:
        p.eng.reset()
        assert p.eng.list_stats(SP) == (0, 0)
        fresh = SparseOracleEngine(D, "ip")  # what is left after a reset: the definitions
        for a, kind in ((SP, "sparse"), (INT, "int64"), (FLT, "float64")):
            fresh.define_attr(a, kind)
        p.model = fresh
        rows = random_corpus(p.rng, 130, 64, True)
        for e in (p.eng, p.model):
            assert e.append(np.ones((130, D), np.float32)) == 0
            e.set_attr_sparse(SP, 0, sparse_csr(rows))
        p.check_exact([p.query(5), p.query(30), {}], 64, tag="after reset")
    finally:
        p.close()


# ---------------------------------------------------------------- refusals: status 1 (6 for k), then correct answers
def _raw_search(eng, offsets, terms, weights, k, attr=SP):
    lib = _native.load()
    offsets = np.asarray(offsets, np.int64)
    terms, weights = np.asarray(terms, np.int32), np.asarray(weights, np.float32)
    nq, kk = offsets.size - 1, max(k, 1)
    lab, s32, cnt = np.empty((nq, kk), np.int64), np.empty((nq, kk), np.float32), np.empty(nq, np.int32)
    return lib.mlvdb_search_batch_sparse(eng.handle, attr, offsets.ctypes.data, terms.ctypes.data, weights.ctypes.data, nq, k,
                                         None, lab.ctypes.data, s32.ctypes.data, cnt.ctypes.data, None)


def _raw_set(eng, first, offsets, terms, weights, present=None, attr=SP):
    lib = _native.load()
    offsets = np.asarray(offsets, np.int64)
    terms, weights = np.asarray(terms, np.int32), np.asarray(weights, np.float32)
    present = None if present is None else np.asarray(present, np.uint8)
    return lib.mlvdb_sparse_set(eng.handle, attr, first, offsets.size - 1, offsets.ctypes.data, terms.ctypes.data,
                                weights.ctypes.data, None if present is None else present.ctypes.data)


def test_refusals_leave_the_handle_as_it_was(exact_pair):
    p, eng = exact_pair, exact_pair.eng
    queries = [p.query(6), p.query(20)]
    before_stats = eng.list_stats(SP)
    one = sparse_csr([{1: 1.0}])
    ones = W.ListColumn(np.array([0, 1], np.int64), np.array([5], np.int64), np.array([1], np.uint8))
    refused = {
        # everything a scalar column is needed for
        "attr_set": lambda: eng.set_attr(SP, 0, np.zeros(1, np.int64)),
        "attr_get": lambda: eng.get_attr(SP, 0, 1),
        "attr_set_at": lambda: eng.set_attr_at(SP, np.array([0]), np.zeros(1, np.int64)),
        "attr_update_where": lambda: eng.update_where(prog([(W.TRUE, 0, 0, 0)]), [(SP, _native.SET_ASSIGN, 0)]),
        "facet_values": lambda: eng.facet_values(SP, 16),
        "where_ordered": lambda: eng.where_ordered(SP, 3),
        "distinct": lambda: eng.search_distinct(np.zeros((1, D), np.float32), 3, SP),
        "grouped": lambda: eng.search_grouped(np.zeros((1, D), np.float32), 3, 2, SP),
        "maxsim": lambda: eng.search_maxsim(np.zeros((1, D), np.float32), np.array([0, 1], np.int64), 3, SP),
        # the raw list entries and the list facet
        "attr_list_set": lambda: eng.set_attr_list(SP, 0, ones),
        "attr_list_set_at": lambda: eng.set_attr_list_at(SP, np.array([0]), ones),
        "attr_list_get": lambda: eng.get_attr_list(SP, 0, 1),
        "attr_list_update_where": lambda: eng.update_where_list(prog([(W.TRUE, 0, 0, 0)]), SP, [1]),
        "facet_list_values": lambda: eng.facet_list_values(SP, 16),
        # the sparse entries on other columns
        "sparse_set on int": lambda: eng.set_attr_sparse(INT, 0, one),
        "sparse_get on float": lambda: eng.get_attr_sparse(FLT, 0, 1),
        "search on int": lambda: eng.search_batch_sparse(INT, one, 3),
        "sparse_set_at twice": lambda: eng.set_attr_sparse_at(SP, np.array([1, 1]), sparse_csr([{1: 1.0}, {2: 1.0}])),
        "sparse_set_at outside": lambda: eng.set_attr_sparse_at(SP, np.array([N]), one),
        "sparse_set range": lambda: eng.set_attr_sparse(SP, N, one),
    }
    for op in (W.HAS, W.HAS_ANY, W.HAS_ALL, W.EQ, W.NE, W.LT, W.LE, W.GT, W.GE, W.IN):
        refused[f"where op {op}"] = lambda op=op: eng.where_count(prog([(op, SP, 0, 1)], [1]))
        refused[f"search where op {op}"] = lambda op=op: eng.search_batch_sparse(SP, one, 3, prog([(op, SP, 0, 1)], [1]))
    refused["LEN on int"] = lambda: eng.where_count(prog([(W.LEN, INT, 0, 1)]))
    for tag, call in refused.items():
        with pytest.raises(RuntimeError, match=r"failed \(1\)"):
            call()
        assert tag
    big = list(range(256))
    edges, bins, z = np.array([1, 2], np.int64), np.zeros(3, np.int64), C.c_int64(0)
    raw = {
        "facet_bins": lambda: _native.load().mlvdb_facet_bins(eng.handle, SP, None, edges.ctypes.data, 2, bins.ctypes.data,
                                                               C.byref(z), C.byref(z)),
        "decreasing offsets": lambda: _raw_set(eng, 0, [0, 2, 1], [1, 2], [1.0, 1.0]),
        "negative offset": lambda: _raw_set(eng, 0, [-1, 0], [1], [1.0]),
        "256 entries": lambda: _raw_set(eng, 0, [0, 256], big, [1.0] * 256),
        "negative term": lambda: _raw_set(eng, 0, [0, 2], [-1, 2], [1.0, 1.0]),
        "equal terms": lambda: _raw_set(eng, 0, [0, 2], [2, 2], [1.0, 1.0]),
        "descending terms": lambda: _raw_set(eng, 0, [0, 2], [3, 2], [1.0, 1.0]),
        "nan weight": lambda: _raw_set(eng, 0, [0, 1], [1], [np.nan]),
        "inf weight": lambda: _raw_set(eng, 0, [0, 1], [1], [np.inf]),
        "absent with entries": lambda: _raw_set(eng, 0, [0, 1], [1], [1.0], present=[0]),
        "query of 1025 terms": lambda: _raw_search(eng, [0, 1025], list(range(1025)), [1.0] * 1025, 3),
        "unsorted query": lambda: _raw_search(eng, [0, 2], [5, 4], [1.0, 1.0], 3),
        "nan query weight": lambda: _raw_search(eng, [0, 1], [5], [np.nan], 3),
        "inf query weight": lambda: _raw_search(eng, [0, 1], [5], [-np.inf], 3),
        "negative query term": lambda: _raw_search(eng, [0, 1], [-5], [1.0], 3),
        "offsets not from 0": lambda: _raw_search(eng, [1, 2], [5, 6], [1.0, 1.0], 3),
        "k = 0": lambda: _raw_search(eng, [0, 1], [5], [1.0], 0),
    }
    for tag, call in raw.items():
        assert call() == 1, tag
    assert _raw_search(eng, [0, 1], [5], [1.0], 65) == 6  # MLVDB_ERR_UNSUPPORTED
    assert _raw_search(eng, [0, 1], [5], [1.0], 64) == 0
    assert _raw_set(eng, 0, [0, 255], big[:255], [1.0] * 255, attr=INT) == 1
    # nothing was written, and the handle answers as before
    assert eng.list_stats(SP) == before_stats == p.model.list_stats(SP)
    got, want = p.both("get_attr_sparse", SP, 0, N)
    assert sparse_uncsr(got) == sparse_uncsr(want)
    p.check_exact(queries, 10, tag="after the refusals")
    p.check_exact(queries, 10, prog([(W.LEN, SP, 1, 40)]), tag="after the refusals, where")


# ---------------------------------------------------------------- the grid stride
def test_the_blocks_stride_over_a_large_index():
    """The grid is capped at 1,024 blocks of 16 rows per tile: 40,000 rows make every block walk its stride loop twice and
    some a third time.  Two or three nonzeros per row, exact weights, one tile."""
    n = 40_000
    rng = np.random.default_rng(11)
    terms = rng.integers(0, 50, (n, 3))
    weights = rng.integers(1, 33, (n, 3)) / 8.0
    rows = [dict(zip(t[:2 + i % 2], w[:2 + i % 2])) for i, (t, w) in enumerate(zip(terms.tolist(), weights.tolist()))]
    rows[n - 3] = {3: 100.0}  # the best row of the second query lies in the third sweep
    gone = rng.choice(n - 3, 2000, replace=False)
    eng, model = HipScanEngine(D, "ip", device=0), SparseOracleEngine(D, "ip")
    try:
        block = np.zeros((n, D), np.float32)
        block[:, 0] = 1.0
        for e in (eng, model):
            e.define_attr(SP, "sparse")
            e.append(block)
            e.set_attr_sparse(SP, 0, sparse_csr(rows))
            e.tombstone(gone)
        q = sparse_csr([{int(t): float(w) for t, w in zip(range(0, 50, 7), range(1, 9))}, {3: 1.0}, {}])
        lab, _, cnt, s64 = eng.search_batch_sparse(SP, q, 10)
        ol, _, oc, o64 = model.search_batch_sparse(SP, q, 10)
        assert np.array_equal(lab, ol) and np.array_equal(cnt, oc) and np.array_equal(s64.view(np.int64), o64.view(np.int64))
        assert lab[1, 0] == n - 3 > 16 * 1024 * 2 and s64[1, 0] == 100.0
        # 100 queries at k = 64: the partial lists' 64 MiB bound cuts the grid to 655 blocks, four sweeps per block
        many = sparse_csr([{int(t): float(w) / 8 for t, w in zip(rng.choice(50, 4, replace=False), rng.integers(1, 33, 4))}
                           for _ in range(100)])
        lab, _, cnt, s64 = eng.search_batch_sparse(SP, many, 64)
        ol, _, oc, o64 = model.search_batch_sparse(SP, many, 64)
        assert np.array_equal(lab, ol) and np.array_equal(cnt, oc) and np.array_equal(s64.view(np.int64), o64.view(np.int64))
    finally:
        eng.close()
