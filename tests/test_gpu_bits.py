"""Binary vector columns on the MI355X (include/mlvdb_bits.h), at the engine level through the C ABI: every call is made on
a ``HipScanEngine`` and on the model engine of tests/bits_helpers.py (codes as Python ints, distances from unpacked bits),
and the answers are compared bit for bit -- labels, counts, the 64 bits of every distance.  There is no tolerance here.
2,003 x 64 rows (no multiple of 4, 64 or 256) appended in three batches, about 10 % tombstoned, about 10 % without a code,
some rows overwritten by label, a few written at another width."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.bits_helpers import METRICS, BitsOracleEngine, near, random_codes
from tests.sparse_helpers import sparse_csr

pytestmark = pytest.mark.gpu

D = 64
BT, INT, FLT = 0, 1, 2  # the columns of every engine here
N = 2003
ONE = 7      # the one row whose int value is UNIQUE (kept live, holding the all-zero code)
UNIQUE = 99
ALL = np.uint64(2 ** 64 - 1)
# each lanes-per-row instantiation (1: 1-2 words, 2: 3-4, 4: 5-8, 8: 9-16, 16: 17-32, 16 through LDS: 33 and more), ragged
# last chunks (3, 5, 17, 33, 255 are odd; 33, 64 and 255 walk the 32-word loop twice, twice and eight times) and the limit
WIDTHS = (1, 2, 3, 4, 5, 8, 16, 17, 32, 33, 64, 255)


def prog(ops, table=()):
    return W.Program(np.array(ops, dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


def column(codes, present=None):
    codes = np.ascontiguousarray(codes, dtype=np.uint64)
    return W.BitsColumn(codes, np.ones(codes.shape[0], np.uint8) if present is None else np.asarray(present, np.uint8))


class Pair:
    """The HIP engine and the model, given the same calls."""

    def __init__(self, n, words, seed=0, batches=3, dead=0.1, absent=0.1):
        self.rng = rng = np.random.default_rng(seed + n + 1000 * words)
        self.words, self.n = words, n
        self.eng = HipScanEngine(D, "ip", device=0)
        self.model = BitsOracleEngine(D, "ip")
        for e in (self.eng, self.model):
            e.define_attr(BT, "bits")
            e.define_attr(INT, "int64")
            e.define_attr(FLT, "float64")
        rows = rng.standard_normal((n, D), dtype=np.float32)
        ints = rng.integers(-2, 6, n).astype(np.int64)
        ints[rng.random(n) < 0.1] = W.INT64_ABSENT
        flts = rng.uniform(-1, 1, n)
        flts[rng.random(n) < 0.1] = np.nan
        codes, self.base = random_codes(rng, n, words)
        present = (rng.random(n) >= absent).astype(np.uint8)
        # the nearest codes of `target` sit at the two ends of the index; row ONE holds the all-zero code
        self.target = rng.integers(0, 2 ** 64, size=words, dtype=np.uint64)
        keep = [0, n - 1] + ([ONE] if n > 8 else [])
        codes[0] = near(rng, self.target, 1)
        codes[n - 1] = self.target
        if n > 8:
            codes[ONE] = 0
            ints[ONE] = UNIQUE
        present[keep] = 1
        cuts = [0] + [n * (b + 1) // batches for b in range(batches)] if n >= batches else [0, n]
        for lo, hi in zip(cuts[:-1], cuts[1:]):  # the rows and the pool both regrow on the way
            for e in (self.eng, self.model):
                assert e.append(rows[lo:hi]) == lo
                e.bits_set(BT, lo, column(codes[lo:hi], present[lo:hi]))
                e.set_attr(INT, lo, ints[lo:hi])
                e.set_attr(FLT, lo, flts[lo:hi])
        gone = np.flatnonzero(rng.random(n) < dead) if n > 8 else np.zeros(0, np.int64)
        gone = np.setdiff1d(gone, keep)
        for e in (self.eng, self.model):
            e.tombstone(gone)
        if n > 8:
            # overwritten by label: the old codes stay behind in the pool as garbage (tombstoned rows are skipped)
            free = np.setdiff1d(np.arange(n), keep)
            labels = rng.choice(free, size=min(60, n // 4), replace=False).astype(np.int64)
            new, _ = random_codes(rng, labels.size, words)
            got, want = self.both("bits_set_at", BT, labels, column(new, [i % 9 != 0 for i in range(labels.size)]))
            assert got == want
            # a few rows of another width: they must never be candidates of a search of `words` words
            other = words + 1 if words < 255 else words - 1
            labels = rng.choice(free, size=min(20, n // 8), replace=False).astype(np.int64)
            odd = np.tile(self.target[:1], (labels.size, other))  # (they would be near `target` if they were read)
            got, want = self.both("bits_set_at", BT, labels, column(odd))
            assert got == want
            self.other = other

    def close(self):
        self.eng.close()

    def both(self, method, *args, **kw):
        return getattr(self.eng, method)(*args, **kw), getattr(self.model, method)(*args, **kw)

    def queries(self, nq):
        """nq codes: the target, the alphabet's codes (all-zero and all-ones first), codes near them and random ones."""
        rng, out = self.rng, []
        for i in range(nq):
            pick = i % 5
            if pick == 0:
                out.append(self.target if i == 0 else near(rng, self.target, int(rng.integers(1, min(9, 64 * self.words)))))
            elif pick == 1:
                out.append(self.base[(i // 5) % len(self.base)])
            elif pick == 2:
                out.append(near(rng, self.base[int(rng.integers(0, len(self.base)))], 2))
            else:
                out.append(rng.integers(0, 2 ** 64, size=self.words, dtype=np.uint64))
        return np.ascontiguousarray(np.stack(out), dtype=np.uint64)

    def check(self, queries, k, metric, where=None, tag=""):
        """Labels, counts and the 64 bits of every distance against the model."""
        (lab, d32, cnt, d64), (ol, o32, oc, o64) = self.both("search_bits", BT, queries, k, metric, where)
        tag = f"{tag} words={self.words} {metric} nq={len(queries)} k={k}"
        assert np.array_equal(cnt, oc), f"{tag}: counts"
        assert np.array_equal(lab, ol), f"{tag}: labels"
        assert np.array_equal(d64.view(np.int64), o64.view(np.int64)), f"{tag}: dist64 bits"
        assert np.array_equal(d32.view(np.int32), o32.view(np.int32)), f"{tag}: float distances"
        return lab, d64, cnt


@pytest.fixture(scope="module")
def pairs():
    """One pair per width, built when first asked for and kept for the module."""
    made = {}

    def get(words):
        if words not in made:
            made[words] = Pair(N, words)
        return made[words]

    yield get
    for p in made.values():
        p.close()


# ---------------------------------------------------------------- every width, batch shape, k and metric
def test_the_corpus_holds_what_the_cases_need(pairs):
    p = pairs(4)
    rows, live = p.model.bits_rows(BT), ~p.model._deleted
    widths = {len(r) for r, ok in zip(rows, live) if ok and r is not None}
    assert widths == {4, 5} and any(r is None for r, ok in zip(rows, live) if ok)
    assert live[0] and live[N - 1] and live[ONE] and rows[ONE] == (0, 0, 0, 0) and rows[N - 1] == tuple(p.target.tolist())
    used, alive = p.eng.list_stats(BT)
    assert (used, alive) == p.model.list_stats(BT) and used > alive  # garbage of the rows overwritten by label
    assert p.eng.counts() == p.model.counts() and p.eng.counts()[1] > 100
    # tie groups straddle the ranks: the rows that repeat a code of the alphabet are at one distance of any query
    lab, d64, cnt = p.check(p.queries(3), 64, "hamming", tag="ties")
    assert (np.diff(d64[1]) == 0).sum() > 30 and lab[0, 0] == N - 1 and d64[0, 0] == 0 and lab[0, 1] == 0 and d64[0, 1] == 1


@pytest.mark.parametrize("words", WIDTHS)
def test_every_width_against_the_model(pairs, words):
    p = pairs(words)
    shapes = [(1, 10), (15, 1), (16, 64), (17, 63), (33, 10)]  # full and ragged tiles; k at both ends
    for metric in METRICS:
        for nq, k in shapes:
            lab, d64, cnt = p.check(p.queries(nq), k, metric)
            assert (cnt == k).all()
            assert lab[0, 0] == N - 1 and d64[0, 0] == 0  # the planted code at the last row, then its neighbour at row 0
            if k > 1:
                assert lab[0, 1] == 0 and d64[0, 1] == (1.0 if metric == "hamming" else d64[0, 1]) and d64[0, 1] > 0
    # the rows of another width are candidates of a search of their own width only
    other = np.tile(p.target[:1], (1, p.other))
    lab, d64, cnt = p.check(other, 64, "hamming", tag="the other width")
    assert 0 < cnt[0] <= 20 and (d64[0, :cnt[0]] == 0).all()


@pytest.mark.parametrize("words", [2, 33])
def test_more_queries_than_one_pass_takes(pairs, words):
    """A call is served in passes of 256 queries: 257 queries cross the boundary once."""
    p = pairs(words)
    p.check(p.queries(257), 3, "hamming", tag="257 queries")
    p.check(p.queries(257), 10, "jaccard", prog([(W.GE, INT, 0, 0)]), tag="257 queries, where")


def test_k_64_with_40_candidates_pads_and_k_65_is_unsupported():
    rng = np.random.default_rng(40)
    codes, _ = random_codes(rng, 47, 3)
    present = np.ones(47, np.uint8)
    present[[1, 5, 9, 20, 33, 40, 46]] = 0
    eng, model = HipScanEngine(D, "ip", device=0), BitsOracleEngine(D, "ip")
    try:
        for e in (eng, model):
            e.define_attr(BT, "bits")
            e.append(np.ones((47, D), np.float32))
            e.bits_set(BT, 0, column(codes, present))
        q = np.ascontiguousarray(codes[[2, 3]])
        for metric in METRICS:
            lab, d32, cnt, d64 = eng.search_bits(BT, q, 64, metric)
            ol, o32, oc, o64 = model.search_bits(BT, q, 64, metric)
            assert cnt.tolist() == [40, 40] == oc.tolist() and np.array_equal(lab, ol)
            assert np.array_equal(d64.view(np.int64), o64.view(np.int64)) and np.array_equal(d32.view(np.int32), o32.view(np.int32))
            assert (lab[:, 40:] == -1).all() and np.isposinf(d64[:, 40:]).all() and np.isposinf(d32[:, 40:]).all()
            assert (lab[:, :40] >= 0).all() and np.isfinite(d64[:, :40]).all()
        # k = 65: MLVDB_ERR_UNSUPPORTED, and not one byte of the outputs is touched
        lib = _native.load()
        lab = np.full((2, 65), -7, np.int64)
        d32 = np.full((2, 65), -7.0, np.float32)
        d64 = np.full((2, 65), -7.0, np.float64)
        cnt = np.full(2, -7, np.int32)
        rc = lib.mlvdb_search_batch_bits(eng.handle, BT, q.ctypes.data, 2, 3, 0, 65, None, lab.ctypes.data, d32.ctypes.data,
                                         cnt.ctypes.data, d64.ctypes.data)
        assert rc == 6 and (lab == -7).all() and (d32 == -7).all() and (d64 == -7).all() and (cnt == -7).all()
        assert eng.search_bits(BT, q, 64, "hamming")[2].tolist() == [40, 40]
    finally:
        eng.close()


# ---------------------------------------------------------------- the metrics' corners
def test_jaccard_of_the_all_zero_query(pairs):
    p = pairs(3)
    zero = np.zeros((1, 3), np.uint64)
    half = prog([(W.GE, INT, 2, 0)])  # about half of the rows, row ONE among them: fewer all-zero rows than k
    lab, d64, cnt = p.check(zero, 64, "jaccard", half, tag="zero query")
    rows, cand = p.model.bits_rows(BT), p.model.candidates(BT, half, 3)
    zeros = [i for i in np.flatnonzero(cand).tolist() if rows[i] == (0, 0, 0)]
    assert 2 <= len(zeros) < 64 and ONE in zeros and cnt[0] == 64
    # against all-zero rows the distance is 0 and the labels decide; against every other row it is exactly 1
    assert lab[0, :len(zeros)].tolist() == zeros and (d64[0, :len(zeros)] == 0).all() and not np.signbit(d64[0, :len(zeros)]).any()
    assert (d64[0, len(zeros):] == 1).all() and (np.diff(lab[0, len(zeros):]) > 0).all()
    p.check(zero, 64, "jaccard", tag="zero query, every row")
    # where the zero rows are filtered out only distance 1 is left
    every = [i for i in np.flatnonzero(p.model.candidates(BT, None, 3)).tolist() if rows[i] == (0, 0, 0)]
    some = [int(c) for c in range(-2, 6) if not any(p.model._cols[INT][i] == c for i in every)]
    if some:
        lab, d64, cnt = p.check(zero, 10, "jaccard", prog([(W.EQ, INT, some[0], 0)]), tag="zero query, no zero row")
        assert (d64[0, :cnt[0]] == 1).all()


def test_all_ones_against_its_complement_is_16320(pairs):
    p = pairs(255)
    ones = np.full((1, 255), ALL, np.uint64)
    w = prog([(W.EQ, INT, UNIQUE, 0)])  # the one row that holds the all-zero code
    lab, d64, cnt = p.check(ones, 5, "hamming", w, tag="complement")
    assert cnt[0] == 1 and lab[0, 0] == ONE and d64[0, 0] == 16320.0 and (lab[0, 1:] == -1).all()
    lab, d64, cnt = p.check(ones, 5, "jaccard", w, tag="complement")
    assert d64[0, 0] == 1.0
    lab, d64, cnt = p.check(np.concatenate([ones, ~p.target[None, :], p.target[None, :]]), 64, "hamming", tag="far and near")
    assert d64[2, 0] == 0 and lab[2, 0] == N - 1


def test_a_pairs_distance_does_not_depend_on_the_batch(pairs):
    for words in (4, 40):
        p = pairs(words)
        q = near(p.rng, p.base[3], 3)
        others = p.queries(40)
        for metric in METRICS:
            seen = {}

            def note(queries, at, k, where=None):
                lab, _, cnt, d64 = p.eng.search_bits(BT, np.ascontiguousarray(queries), k, metric, where)
                for l, bits in zip(lab[at, :cnt[at]].tolist(), d64[at, :cnt[at]].view(np.int64).tolist()):
                    assert seen.setdefault(l, bits) == bits, f"label {l}: {bits:#x} != {seen[l]:#x}"
                return cnt[at]

            assert note(q[None, :], 0, 64) == 64
            note(q[None, :], 0, 10)
            note(np.concatenate([others[:3], q[None, :], others[3:6]]), 3, 64)  # another place in its tile
            note(np.concatenate([others[:16], q[None, :]]), 16, 64)             # alone in the second tile
            note(np.concatenate([others, q[None, :]]), 40, 64)                  # the last of many
            note(np.stack([q, q]), 1, 64)
            note(np.concatenate([q[None, :], others[:2]]), 0, 64, prog([(W.GE, INT, 0, 0)]))
            note(np.concatenate([others[5:9], q[None, :]]), 4, 30, prog([(W.EXISTS, BT, 0, 0)]))
            assert len(seen) >= 64


# ---------------------------------------------------------------- where
def test_where_programs(pairs):
    p = pairs(5)
    queries = p.queries(9)
    lit = np.array([0.25]).view(np.int64)[0]
    programs = {
        "int eq": prog([(W.EQ, INT, 3, 0)]),
        "float lt or int in": prog([(W.LT, FLT, int(lit), 0), (W.IN, INT, 0, 2), (W.OR, 0, 0, 0)], [0, 5]),
        "exists": prog([(W.EXISTS, BT, 0, 0)]),
        "not exists": prog([(W.EXISTS, BT, 0, 0), (W.NOT, 0, 0, 0)]),  # no candidate has no code
        "exists and int": prog([(W.EXISTS, BT, 0, 0), (W.GE, INT, 2, 0), (W.AND, 0, 0, 0)]),
        "nothing": prog([(W.TRUE, 0, 0, 0), (W.NOT, 0, 0, 0)]),
        "one row": prog([(W.EQ, INT, UNIQUE, 0)]),
    }
    for tag, w in programs.items():
        for k, metric in ((1, "hamming"), (64, "jaccard"), (10, "hamming")):
            lab, d64, cnt = p.check(queries, k, metric, w, tag=tag)
        want = int((p.model.match(w) & p.model.candidates(BT, None, 5)).sum())
        assert (cnt == min(10, want)).all(), tag
        if tag in ("nothing", "not exists"):
            assert want == 0 and (lab == -1).all() and np.isposinf(d64).all()
        if tag == "one row":
            assert want == 1 and (lab[:, 0] == ONE).all() and (lab[:, 1:] == -1).all()
        got, expect = p.both("where_count", w)
        assert got == expect, tag


def test_an_empty_index_and_a_column_without_values_answer_padding():
    eng = HipScanEngine(D, "ip", device=0)
    try:
        eng.define_attr(BT, "bits")
        q = np.array([[1, 2], [0, 0]], np.uint64)
        for state in ("empty", "no values", "all dead", "reset"):
            if state == "no values":
                eng.append(np.ones((300, D), np.float32))
            elif state == "all dead":
                eng.bits_set(BT, 0, column(np.ones((300, 2), np.uint64)))
                assert eng.search_bits(BT, q, 5, "jaccard")[2].tolist() == [5, 5]
                eng.tombstone(np.arange(300))
            elif state == "reset":
                eng.reset()
            for metric in METRICS:
                lab, d32, cnt, d64 = eng.search_bits(BT, q, 5, metric)
                assert (lab == -1).all() and (cnt == 0).all() and np.isposinf(d64).all() and np.isposinf(d32).all(), state
    finally:
        eng.close()


# ---------------------------------------------------------------- the grid stride
def test_the_blocks_stride_over_a_large_index():
    """A pass spreads 512 blocks over its tiles, and a block of the 16-lanes-per-row kernels takes 16 rows per step: 40,000
    rows of 33-word codes make every block of a one-tile call walk its stride loop four or five times (the full grid: 512
    blocks), and with 128 queries the grid is cut to 64 blocks per tile, which walk it 39 or 40 times.  (The 64 MiB bound
    of the partial lists cannot be what cuts the grid at k <= 64: DESIGN 11.17, deviations.)"""
    p = Pair(40_000, 33, seed=11, batches=2)
    try:
        for metric in METRICS:
            lab, d64, cnt = p.check(p.queries(3), 10, metric, tag="full grid")
            assert lab[0, 0] == 39_999 and lab[0, 1] == 0
        lab, d64, cnt = p.check(p.queries(128), 64, "hamming", tag="cut grid")
        assert (cnt == 64).all() and lab[0, 0] == 39_999
        p.check(p.queries(17), 64, "jaccard", prog([(W.GE, INT, 1, 0)]), tag="where")
    finally:
        p.close()


# ---------------------------------------------------------------- life cycle
def _raw_get(eng, first, n, capacity, attr=BT):
    widths = np.full(max(n, 1), -7, np.int32)
    codes = np.full(max(capacity, 1), 7, np.uint64)
    needed = C.c_int64(-1)
    rc = _native.load().mlvdb_bits_get(eng.handle, attr, first, n, widths.ctypes.data, codes.ctypes.data, capacity,
                                       C.byref(needed))
    return rc, widths[:n], codes[:capacity], needed.value


def test_life_cycle():
    p = Pair(700, 6, seed=5)
    try:
        queries = p.queries(18)
        w = prog([(W.GE, INT, 1, 0)])

        def check(tag, words=6, qs=queries):
            p.check(qs, 10, "hamming", tag=tag)
            p.check(qs, 64, "jaccard", w, tag=tag + " where")
            total = p.model.counts()[0]
            assert p.eng.counts() == p.model.counts(), tag
            (gw, gc), (ww, wc) = p.both("bits_get", BT, 0, total)
            assert np.array_equal(gw, ww) and np.array_equal(gc, wc) and gw.dtype == np.int32 and gc.dtype == np.uint64, tag
            assert (gw == 0).any() and (gw == words).any()
            assert p.eng.list_stats(BT) == p.model.list_stats(BT), tag

        check("built")
        more, _ = random_codes(p.rng, 333, 6)
        block = p.rng.standard_normal((333, D), dtype=np.float32)
        held = p.rng.random(333) > 0.1
        for e in (p.eng, p.model):  # append (rows and pool regrow) -> set -> search
            assert e.append(block) == 700
            e.bits_set(BT, 700, column(more, held))
        check("appended")
        gone = p.rng.choice(np.arange(1, 1033), 150, replace=False)
        for e in (p.eng, p.model):
            e.tombstone(gone)
        check("tombstoned")
        used, live = p.eng.list_stats(BT)
        assert used > live
        old, want_old = p.both("compact")
        assert np.array_equal(old, want_old)
        assert p.eng.list_stats(BT)[0] == p.eng.list_stats(BT)[1] == live
        check("compacted")
        # the identity compaction sheds the garbage of an overwrite too
        labels = np.arange(0, 200, 3, dtype=np.int64)
        new, _ = random_codes(p.rng, labels.size, 6)
        assert p.both("bits_set_at", BT, labels, column(new)) == (labels.size, labels.size)
        used, live = p.eng.list_stats(BT)
        assert used > live
        old, want_old = p.both("compact")
        assert np.array_equal(old, want_old) and np.array_equal(old, np.arange(old.size))
        assert p.eng.list_stats(BT) == (live, live)
        check("identity compaction")
        # a partial read-back, and the protocol of a buffer that is too small: the need is reported, nothing else is written
        (gw, gc), (ww, wc) = p.both("bits_get", BT, 100, 50)
        assert np.array_equal(gw, ww) and np.array_equal(gc, wc) and gc.size == int(gw.sum()) > 0
        rc, widths, codes, needed = _raw_get(p.eng, 100, 50, gc.size - 1)
        assert rc == 0 and needed == gc.size and (widths == -7).all() and (codes == 7).all()
        rc, widths, codes, needed = _raw_get(p.eng, 100, 50, 0)
        assert rc == 0 and needed == gc.size and (widths == -7).all()
        rc, widths, codes, needed = _raw_get(p.eng, 100, 50, gc.size + 3)
        assert rc == 0 and needed == gc.size and np.array_equal(widths, gw) and np.array_equal(codes[:gc.size], gc) and \
            (codes[gc.size:] == 7).all()
        rc, widths, codes, needed = _raw_get(p.eng, 100, 0, 0)
        assert rc == 0 and needed == 0
        # reset: the definitions stay, the rows and the pool go; rows of a new width come in
        p.eng.reset()
        assert p.eng.list_stats(BT) == (0, 0)
        fresh = BitsOracleEngine(D, "ip")
        for a, kind in ((BT, "bits"), (INT, "int64"), (FLT, "float64")):
            fresh.define_attr(a, kind)
        p.model = fresh
        wide, base = random_codes(p.rng, 130, 9)
        ints = p.rng.integers(0, 4, 130).astype(np.int64)
        for e in (p.eng, p.model):
            assert e.append(np.ones((130, D), np.float32)) == 0
            e.bits_set(BT, 0, column(wide, np.arange(130) % 10 != 3))
            e.set_attr(INT, 0, ints)
        check("after reset", words=9, qs=np.ascontiguousarray(np.concatenate([base[:4], wide[5:9]])))
        lab, d32, cnt, d64 = p.eng.search_bits(BT, queries, 5, "hamming")  # the old width finds nothing now
        assert (cnt == 0).all() and (lab == -1).all()
    finally:
        p.close()


# ---------------------------------------------------------------- refusals: status 1 (6 for k), then correct answers
def _raw_search(eng, nq, words, metric, k, attr=BT, queries=True, labels=True, where=None):
    lib = _native.load()
    q = np.zeros((max(nq, 1), max(words, 1)), np.uint64)
    kk = max(k, 1)
    lab, d32, cnt = np.empty((max(nq, 1), kk), np.int64), np.empty((max(nq, 1), kk), np.float32), np.empty(max(nq, 1), np.int32)
    return lib.mlvdb_search_batch_bits(eng.handle, attr, q.ctypes.data if queries else None, nq, words, metric, k, where,
                                       lab.ctypes.data if labels else None, d32.ctypes.data, cnt.ctypes.data, None)


def _raw_set(eng, first, n, words, attr=BT, codes=True):
    buf = np.zeros((max(n, 1), max(words, 1)), np.uint64)
    return _native.load().mlvdb_bits_set(eng.handle, attr, first, n, words, buf.ctypes.data if codes else None, None)


def _raw_set_at(eng, labels, words, attr=BT, codes=True, updated=True):
    labels = np.asarray(labels, np.int64)
    buf = np.zeros((max(labels.size, 1), max(words, 1)), np.uint64)
    z = C.c_int64(-1)
    return _native.load().mlvdb_bits_set_at(eng.handle, attr, labels.ctypes.data, labels.size, words,
                                            buf.ctypes.data if codes else None, None, C.byref(z) if updated else None)


def test_refusals_leave_the_handle_as_it_was(pairs):
    p = pairs(4)
    eng = p.eng
    queries = p.queries(6)
    before_stats = eng.list_stats(BT)
    one = column(np.ones((1, 4), np.uint64))
    vec = sparse_csr([{1: 1.0}])
    ones = W.ListColumn(np.array([0, 1], np.int64), np.array([5], np.int64), np.array([1], np.uint8))
    zero = np.zeros((1, D), np.float32)
    refused = {
        # everything a scalar column is needed for
        "attr_set": lambda: eng.set_attr(BT, 0, np.zeros(1, np.int64)),
        "attr_get": lambda: eng.get_attr(BT, 0, 1),
        "attr_set_at": lambda: eng.set_attr_at(BT, np.array([0]), np.zeros(1, np.int64)),
        "attr_update_where": lambda: eng.update_where(prog([(W.TRUE, 0, 0, 0)]), [(BT, _native.SET_ASSIGN, 0)]),
        "facet_values": lambda: eng.facet_values(BT, 16),
        "attr_stats": lambda: eng.attr_stats(BT),
        "attr_stats by": lambda: eng.attr_stats(INT, by=BT, max_groups=8),
        "where_ordered": lambda: eng.where_ordered(BT, 3),
        "geo_nearest": lambda: eng.geo_nearest(BT, 0, 3),
        "distinct": lambda: eng.search_distinct(zero, 3, BT),
        "grouped": lambda: eng.search_grouped(zero, 3, 2, BT),
        "maxsim": lambda: eng.search_maxsim(zero, np.array([0, 1], np.int64), 3, BT),
        # the raw list entries and the list facet
        "attr_list_set": lambda: eng.set_attr_list(BT, 0, ones),
        "attr_list_set_at": lambda: eng.set_attr_list_at(BT, np.array([0]), ones),
        "attr_list_get": lambda: eng.get_attr_list(BT, 0, 1),
        "attr_list_update_where": lambda: eng.update_where_list(prog([(W.TRUE, 0, 0, 0)]), BT, [1]),
        "facet_list_values": lambda: eng.facet_list_values(BT, 16),
        # the sparse entries
        "sparse_set": lambda: eng.set_attr_sparse(BT, 0, vec),
        "sparse_set_at": lambda: eng.set_attr_sparse_at(BT, np.array([0]), vec),
        "sparse_get": lambda: eng.get_attr_sparse(BT, 0, 1),
        "search_batch_sparse": lambda: eng.search_batch_sparse(BT, vec, 3),
        "hybrid": lambda: eng.search_hybrid(zero, BT, vec, 3, 5, 5),
        # the bits entries on other columns (wrong type), and their own arguments
        "bits_set on int": lambda: eng.bits_set(INT, 0, one),
        "bits_set_at on int": lambda: eng.bits_set_at(INT, np.array([0]), one),
        "bits_get on float": lambda: eng.bits_get(FLT, 0, 1),
        "search on int": lambda: eng.search_bits(INT, np.ones((1, 4), np.uint64), 3),
        "bits_set_at twice": lambda: eng.bits_set_at(BT, np.array([1, 1]), column(np.ones((2, 4), np.uint64))),
        "bits_set_at outside": lambda: eng.bits_set_at(BT, np.array([N]), one),
        "bits_set_at negative": lambda: eng.bits_set_at(BT, np.array([-1]), one),
        "bits_set range": lambda: eng.bits_set(BT, N, one),
        "bits_get range": lambda: eng.bits_get(BT, N - 1, 2),
    }
    for op in (W.HAS, W.HAS_ANY, W.HAS_ALL, W.LEN, W.EQ, W.NE, W.LT, W.LE, W.GT, W.GE, W.IN):
        refused[f"where op {op}"] = lambda op=op: eng.where_count(prog([(op, BT, 0, 1)], [1]))
        refused[f"search where op {op}"] = lambda op=op: eng.search_bits(BT, queries, 3, "hamming", prog([(op, BT, 0, 1)], [1]))
    for tag, call in refused.items():
        with pytest.raises(RuntimeError, match=r"failed \(1\)"):
            call()
        assert tag
    edges, bins, z = np.array([1, 2], np.int64), np.zeros(3, np.int64), C.c_int64(0)
    raw = {
        "facet_bins": lambda: _native.load().mlvdb_facet_bins(eng.handle, BT, None, edges.ctypes.data, 2, bins.ctypes.data,
                                                               C.byref(z), C.byref(z)),
        "words 0": lambda: _raw_search(eng, 1, 0, 0, 3),
        "words 256": lambda: _raw_search(eng, 1, 256, 0, 3),
        "metric 2": lambda: _raw_search(eng, 1, 4, 2, 3),
        "metric -1": lambda: _raw_search(eng, 1, 4, -1, 3),
        "k = 0": lambda: _raw_search(eng, 1, 4, 0, 0),
        "nq = -1": lambda: _raw_search(eng, -1, 4, 0, 3),
        "null queries": lambda: _raw_search(eng, 1, 4, 0, 3, queries=False),
        "null labels": lambda: _raw_search(eng, 1, 4, 0, 3, labels=False),
        "set words 0": lambda: _raw_set(eng, 0, 1, 0),
        "set words 256": lambda: _raw_set(eng, 0, 1, 256),
        "set null codes": lambda: _raw_set(eng, 0, 1, 4, codes=False),
        "set n = -1": lambda: _raw_set(eng, 0, -1, 4),
        "set_at words 0": lambda: _raw_set_at(eng, [0], 0),
        "set_at words 256": lambda: _raw_set_at(eng, [0], 256),
        "set_at null codes": lambda: _raw_set_at(eng, [0], 4, codes=False),
        "set_at null counter": lambda: _raw_set_at(eng, [0], 4, updated=False),
        "get null needed": lambda: _native.load().mlvdb_bits_get(eng.handle, BT, 0, 1, None, None, 0, None),
        "get negative capacity": lambda: _raw_get(eng, 0, 1, -1)[0],
    }
    for tag, call in raw.items():
        assert call() == 1, tag
    assert _raw_search(eng, 1, 4, 0, 65) == 6  # MLVDB_ERR_UNSUPPORTED
    assert _raw_search(eng, 1, 4, 1, 64) == 0 and _raw_search(eng, 0, 4, 0, 3, queries=False, labels=False) == 0
    assert _raw_search(eng, 1, 255, 0, 3) == 0 and _raw_search(eng, 1, 1, 1, 3) == 0
    # nothing was written, and the handle answers as before
    assert eng.list_stats(BT) == before_stats == p.model.list_stats(BT)
    (gw, gc), (ww, wc) = p.both("bits_get", BT, 0, N)
    assert np.array_equal(gw, ww) and np.array_equal(gc, wc)
    for metric in METRICS:
        p.check(queries, 10, metric, tag="after the refusals")
        p.check(queries, 10, metric, prog([(W.EXISTS, BT, 0, 0), (W.LE, INT, 3, 0), (W.AND, 0, 0, 0)]), tag="after, where")
