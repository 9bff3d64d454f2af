"""List-valued attribute columns on the MI355X (include/mlvdb_list.h), at the engine level through the C ABI: every call is
made on a ``HipScanEngine`` and on the model engine of tests/tags_helpers.py (lists as Python sets), and the answers are
compared.  2,000 x 64 rows (no multiple of 64 or 256) appended in three batches, about 10 % tombstoned."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import FacetOverflow, HipScanEngine
from oracle import exact_scan
from tests.tags_helpers import (INT64_MAX, INT64_MIN, TagsOracleEngine, csr, py_match, random_list_program,
                                random_tag_metadata, uncsr)

pytestmark = pytest.mark.gpu

D = 64
LIST, INT, FLT = 0, 1, 2  # the columns of every engine here
RARE, COMMON = 424242, 2
LONG = list(range(1000, 1255))  # a list of 255 elements
ELEMENTS = [INT64_MIN + 1, -5, 0, 1, COMMON, 3, 7, 100, INT64_MAX]


def prog(ops, table=()):
    return W.Program(np.array(ops, dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


def random_lists(rng, n):
    """Rows with no list, an empty one, one element, a few, and 255; COMMON in most rows, RARE in about one of a hundred."""
    out = []
    for i in range(n):
        r = rng.random()
        if r < 0.1:
            out.append(None)
        elif r < 0.2:
            out.append([])
        elif r < 0.3:
            out.append([int(rng.choice(ELEMENTS))])
        else:
            row = set(int(x) for x in rng.choice(ELEMENTS, int(rng.integers(1, 7))))
            if rng.random() < 0.7:
                row.add(COMMON)
            out.append(sorted(row))
        if out[-1] is not None and rng.random() < 0.01:
            out[-1] = sorted(set(out[-1]) | {RARE})
    for at in (3, n // 2, n - 1):
        if n > 8:
            out[at] = LONG if at != n // 2 else LONG[:-1] + [INT64_MAX]
    if n > 8:
        out[5] = [RARE]
    return out


class Pair:
    """The HIP engine and the model, given the same calls."""

    def __init__(self, space, n, seed=0, batches=3):
        self.rng = rng = np.random.default_rng(seed + n)
        self.rows = rng.standard_normal((n, D), dtype=np.float32)
        self.eng = HipScanEngine(D, space, device=0)
        self.model = TagsOracleEngine(D, space)
        self.space, self.n = space, n
        for e in (self.eng, self.model):
            e.define_attr(LIST, "int64_list")
            e.define_attr(INT, "int64")
            e.define_attr(FLT, "float64")
        ints = rng.integers(-2, 6, n).astype(np.int64)
        ints[rng.random(n) < 0.1] = W.INT64_ABSENT
        flts = rng.uniform(-1, 1, n)
        flts[rng.random(n) < 0.1] = np.nan
        lists = random_lists(rng, n)
        cuts = [0] + [n * (b + 1) // batches for b in range(batches)] if n >= batches else [0, n]
        for lo, hi in zip(cuts[:-1], cuts[1:]):  # the rows and the pool both regrow on the way
            for e in (self.eng, self.model):
                assert e.append(self.rows[lo:hi]) == lo
                e.set_attr_list(LIST, lo, csr(lists[lo:hi]))
                e.set_attr(INT, lo, ints[lo:hi])
                e.set_attr(FLT, lo, flts[lo:hi])
        dead = np.flatnonzero(rng.random(n) < 0.1) if n > 8 else np.zeros(0, np.int64)
        for e in (self.eng, self.model):
            e.tombstone(dead)
        self.qs = rng.standard_normal((6, D), dtype=np.float32)

    def close(self):
        self.eng.close()

    def both(self, method, *args):
        got, want = getattr(self.eng, method)(*args), getattr(self.model, method)(*args)
        return got, want

    def check_state(self, tag=""):
        """Every column and the counters against the model."""
        total = self.model.counts()[0]
        assert self.eng.counts() == self.model.counts(), tag
        if total:
            assert uncsr(self.eng.get_attr_list(LIST, 0, total)) == uncsr(self.model.get_attr_list(LIST, 0, total)), tag
            assert np.array_equal(self.eng.get_attr(INT, 0, total), self.model.get_attr(INT, 0, total)), tag
            assert np.array_equal(self.eng.get_attr(FLT, 0, total, np.float64).view(np.int64),
                                  self.model.get_attr(FLT, 0, total, np.float64).view(np.int64)), tag
        assert self.eng.list_stats(LIST) == self.model.list_stats(LIST), tag

    def check_program(self, p, tag, search=True):
        got, want = self.both("where_count", p)
        assert got == want, f"{tag}: count {got}, model {want}"
        got, want = self.both("where_labels", p)
        assert np.array_equal(got, want), tag
        matches = int(want.size)
        if not search or self.model.counts()[0] == 0:
            return matches
        k = 10
        (lab, dist, cnt, d64), (ol, od, oc, _) = self.both("search64", self.qs, k, None, p)
        assert np.array_equal(lab, ol) and np.array_equal(cnt, oc), f"{tag}: kNN ids"
        assert np.allclose(dist, od, atol=1e-5, rtol=0), f"{tag}: kNN distances"
        got = self.eng.range(self.qs[:3], self.radius, 256, False, p)
        want = self.model.range(self.qs[:3], self.radius, 256, False, p)
        for qi, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g[0], w[0]), f"{tag}: range ids of query {qi}"
            assert np.allclose(g[1], w[1], atol=1e-5, rtol=0), f"{tag}: range distances of query {qi}"
        return matches

    @property
    def radius(self):
        if not hasattr(self, "_radius"):
            dd = np.sort(exact_scan.exact_distances(self.qs[:3], self.rows, self.space), axis=1)
            self._radius = float(dd[:, min(120, self.n - 1)].mean())
        return self._radius


def fixed_programs():
    """(name, program): every list op alone and mixed with the scalar columns; set ranges of size 1, 2 and 300, one with no
    member anywhere, literals at both ends of int64."""
    big = list(range(1000, 1300))  # 300 values: the 255 of LONG and 45 more
    none = [555, 556, 557]       # in no list
    table = [RARE] + [COMMON, INT64_MAX] + big + none + LONG + [INT64_MIN + 1, INT64_MAX]
    o_rare, o_two, o_big, o_none, o_long, o_ends = 0, 1, 3, 303, 306, 561
    out = [
        ("has common", prog([(W.HAS, LIST, COMMON, 0)])),
        ("has rare", prog([(W.HAS, LIST, RARE, 0)])),
        ("has max", prog([(W.HAS, LIST, INT64_MAX, 0)])),
        ("has min+1", prog([(W.HAS, LIST, INT64_MIN + 1, 0)])),
        ("has min", prog([(W.HAS, LIST, INT64_MIN, 0)])),
        ("has last of long", prog([(W.HAS, LIST, 1254, 0)])),
        ("has nothing", prog([(W.HAS, LIST, 555, 0)])),
        ("any 1", prog([(W.HAS_ANY, LIST, o_rare, 1)], table)),
        ("any 2", prog([(W.HAS_ANY, LIST, o_two, 2)], table)),
        ("any 300", prog([(W.HAS_ANY, LIST, o_big, 300)], table)),
        ("any none present", prog([(W.HAS_ANY, LIST, o_none, 3)], table)),
        ("any empty range", prog([(W.HAS_ANY, LIST, o_none, 0)], table)),
        ("any ends", prog([(W.HAS_ANY, LIST, o_ends, 2)], table)),
        ("all 1", prog([(W.HAS_ALL, LIST, o_two, 1)], table)),
        ("all 2", prog([(W.HAS_ALL, LIST, o_two, 2)], table)),
        ("all 255", prog([(W.HAS_ALL, LIST, o_long, 255)], table)),
        ("all 254", prog([(W.HAS_ALL, LIST, o_long, 254)], table)),
        ("all 300", prog([(W.HAS_ALL, LIST, o_big, 300)], table)),
        ("all none present", prog([(W.HAS_ALL, LIST, o_none, 2)], table)),
        ("all ends", prog([(W.HAS_ALL, LIST, o_ends, 2)], table)),
        ("len 0", prog([(W.LEN, LIST, 0, 0)])),
        ("len 1", prog([(W.LEN, LIST, 1, 1)])),
        ("len 255", prog([(W.LEN, LIST, 255, 255)])),
        ("len any", prog([(W.LEN, LIST, 0, 255)])),
        ("len 2..5", prog([(W.LEN, LIST, 2, 5)])),
        ("len below", prog([(W.LEN, LIST, -3, 1)])),
        ("len inverted", prog([(W.LEN, LIST, 5, 2)])),
        ("len huge", prog([(W.LEN, LIST, 256, INT64_MAX)])),
        ("exists", prog([(W.EXISTS, LIST, 0, 0)])),
        ("not exists", prog([(W.EXISTS, LIST, 0, 0), (W.NOT, 0, 0, 0)])),
        ("not has", prog([(W.HAS, LIST, COMMON, 0), (W.NOT, 0, 0, 0)])),
        ("has and int", prog([(W.HAS, LIST, COMMON, 0), (W.GE, INT, 2, 0), (W.AND, 0, 0, 0)])),
        ("any or float", prog([(W.HAS_ANY, LIST, o_big, 300), (W.LT, FLT, W.float_bits(-0.5), 0), (W.OR, 0, 0, 0)], table)),
        ("not all and in", prog([(W.HAS_ALL, LIST, o_two, 2), (W.NOT, 0, 0, 0), (W.IN, INT, o_two, 1), (W.AND, 0, 0, 0)], table)),
        ("len and not float or int", prog([(W.LEN, LIST, 1, 3), (W.EXISTS, FLT, 0, 0), (W.NOT, 0, 0, 0), (W.AND, 0, 0, 0),
                                           (W.EQ, INT, 1, 0), (W.OR, 0, 0, 0)])),
    ]
    return out


# ---------------------------------------------------------------- 1. parity of the ops
@pytest.mark.parametrize("space, n", [("cosine", 2000), ("l2", 2000), ("l2", 300), ("cosine", 1)])
def test_list_ops_answer_as_the_model(space, n):
    pair = Pair(space, n)
    try:
        pair.check_state("ingest")
        sizes = {name: pair.check_program(p, f"{space}_{n} {name}") for name, p in fixed_programs()}
        if n == 2000:  # the data reaches what the programs are about
            assert sizes["has rare"] > 0 and sizes["all 255"] >= 1 and sizes["all 254"] > sizes["all 255"]
            assert sizes["len 0"] > 0 and sizes["len 1"] > 0 and sizes["len 255"] == sizes["all 254"]
            assert sizes["has nothing"] == sizes["any none present"] == sizes["all 300"] == sizes["has min"] == 0
            assert sizes["has max"] > 0 and sizes["has min+1"] > 0 and sizes["any 300"] == sizes["len 255"]
        rng = np.random.default_rng(77)
        matched = 0
        for i in range(100 if n == 2000 else 25):
            p = random_list_program(rng, LIST, INT, FLT, ELEMENTS + [RARE, 1000, 1254])
            matched += pair.check_program(p, f"{space}_{n} random {i}: {p.ops.tolist()} {p.set.tolist()}", search=i % 4 == 0) > 0
        assert matched > (10 if n > 1 else 0)
    finally:
        pair.close()


# ---------------------------------------------------------------- 2. per-query filters
@pytest.mark.parametrize("space", ["cosine", "l2"])
def test_per_query_filters_mix_list_and_scalar_programs(space):
    pair = Pair(space, 2000, seed=2)
    try:
        fixed = dict(fixed_programs())
        programs = [fixed["has rare"], fixed["has common"], fixed["any 300"], fixed["all 2"], fixed["len 2..5"],
                    fixed["has and int"], fixed["not all and in"], prog([(W.GE, INT, 1, 0)]),
                    prog([(W.LT, FLT, W.float_bits(0.0), 0)]), fixed["has nothing"]]
        nq = 24
        of = np.array([(i % (len(programs) + 1)) - 1 for i in range(nq)], np.int32)  # None and every program in turn
        qs = pair.rng.standard_normal((nq, D), dtype=np.float32)
        k = 10
        lab, dist, cnt, d64, routes = pair.eng.search_each(qs, k, programs, of, want64=True, return_routes=True)
        assert routes[0] == _native.ROUTE_GATHER and routes[1] == _native.ROUTE_SCAN and routes[9] == _native.ROUTE_NONE, routes
        hits = pair.eng.range_each(qs, pair.radius, 256, programs, of)
        for i, p in enumerate(of.tolist()):
            where = None if p < 0 else programs[p]
            sl, sd, sc, s64 = pair.eng.search64(qs[i:i + 1], k, where=where)
            assert np.array_equal(lab[i], sl[0]) and cnt[i] == sc[0], f"query {i} program {p}"
            assert np.array_equal(d64[i].view(np.int64), s64[0].view(np.int64)), f"query {i} program {p}"
            ol, od, oc, _ = pair.model.search64(qs[i:i + 1], k, where=where)
            assert np.array_equal(lab[i], ol[0]) and cnt[i] == oc[0], f"query {i} program {p}: the model"
            assert np.allclose(dist[i], od[0], atol=1e-5, rtol=0)
            one = pair.eng.range(qs[i:i + 1], pair.radius, 256, False, where)[0]
            want = pair.model.range(qs[i:i + 1], pair.radius, 256, False, where)[0]
            assert np.array_equal(hits[i][0], one[0]) and np.array_equal(hits[i][1], one[1]), f"range query {i} program {p}"
            assert np.array_equal(hits[i][0], want[0]) and np.allclose(hits[i][1], want[1], atol=1e-5, rtol=0)
        assert pair.eng.count_each(programs).tolist() == [pair.model.where_count(p) for p in programs]
    finally:
        pair.close()


# ---------------------------------------------------------------- 3. refusals are status codes
def test_refusals_are_status_codes_and_the_handle_lives_on():
    pair = Pair("cosine", 300, seed=3)
    eng = pair.eng
    try:
        before = eng.where_count(prog([(W.HAS, LIST, COMMON, 0)]))
        bad_programs = [
            prog([(W.EQ, LIST, 1, 0)]), prog([(W.NE, LIST, 1, 0)]), prog([(W.LT, LIST, 1, 0)]), prog([(W.LE, LIST, 1, 0)]),
            prog([(W.GT, LIST, 1, 0)]), prog([(W.GE, LIST, 1, 0)]), prog([(W.IN, LIST, 0, 1)], [1]),
            prog([(W.HAS, INT, 1, 0)]), prog([(W.HAS_ANY, INT, 0, 1)], [1]), prog([(W.HAS_ALL, FLT, 0, 1)], [1]),
            prog([(W.LEN, INT, 0, 1)]), prog([(W.LEN, FLT, 0, 1)]),
            prog([(W.HAS, 7, 1, 0)]),                         # undefined attribute
            prog([(W.HAS_ALL, LIST, 0, 0)], [1]),             # empty range
            prog([(W.HAS_ALL, LIST, 0, 2)], [1, 1]),          # not strictly ascending
            prog([(W.HAS_ALL, LIST, 0, 2)], [2, 1]),
            prog([(W.HAS_ANY, LIST, 0, 2)], [2, 1]),          # unsorted
            prog([(W.HAS_ANY, LIST, 1, 2)], [1, 2]),          # outside the table
            prog([(W.HAS_ANY, LIST, -1, 1)], [1, 2]),
            prog([(W.HAS_ALL, LIST, 0, 2 ** 31)], [1, 2]),
            prog([(16, LIST, 0, 0)]), prog([(42, 0, 0, 0)]),  # unknown ops
        ]
        for i, p in enumerate(bad_programs):
            for call in (lambda: eng.where_count(p), lambda: eng.search(pair.qs, 3, where=p),
                         lambda: eng.count_each([p]), lambda: eng.update_where_list(p, LIST, [1]),
                         lambda: eng.facet_list_values(LIST, 16, where=p), lambda: eng.tombstone_where(p)):
                with pytest.raises(RuntimeError, match=r"\(1\)"):
                    call()
        one = np.array([5], np.int64)

        def lists(offsets, values, present=None):
            n = len(offsets) - 1
            return W.ListColumn(np.array(offsets, np.int64), np.array(values, np.int64),
                                np.ones(n, np.uint8) if present is None else np.array(present, np.uint8))
        bad_lists = [lists([0, 2, 1], [1, 2]), lists([0, 256], list(range(256))), lists([0, 2], [2, 1]), lists([0, 2], [1, 1]),
                     lists([0, 1], [INT64_MIN]), lists([-1, 1], [1, 2]), lists([0, 1], [1], [0])]
        bad_writes = [
            lambda: eng.set_attr(LIST, 0, one), lambda: eng.get_attr(LIST, 0, 1), lambda: eng.set_attr_at(LIST, one, one),
            lambda: eng.update_where(prog([(W.TRUE, 0, 0, 0)]), [(LIST, _native.SET_ASSIGN, 7)]),
            lambda: eng.update_where(prog([(W.TRUE, 0, 0, 0)]), [(INT, _native.SET_ASSIGN, 7), (LIST, _native.SET_ADD, 1)]),
            lambda: eng.set_attr_list(INT, 0, lists([0, 1], [1])), lambda: eng.set_attr_list(9, 0, lists([0, 1], [1])),
            lambda: eng.set_attr_list(LIST, 300, lists([0, 1], [1])), lambda: eng.get_attr_list(INT, 0, 1),
            lambda: eng.get_attr_list(LIST, 299, 2), lambda: eng.list_stats(FLT),
            lambda: eng.set_attr_list_at(LIST, np.array([1, 1]), lists([0, 1, 2], [1, 2])),
            lambda: eng.set_attr_list_at(LIST, np.array([300]), lists([0, 1], [1])),
            lambda: eng.set_attr_list_at(INT, np.array([1]), lists([0, 1], [1])),
            lambda: eng.update_where_list(prog([(W.TRUE, 0, 0, 0)]), INT, [1]),
            lambda: eng.update_where_list(prog([(W.TRUE, 0, 0, 0)]), LIST, [2, 1]),
            lambda: eng.update_where_list(prog([(W.TRUE, 0, 0, 0)]), LIST, list(range(256))),
            lambda: eng.update_where_list(prog([(W.TRUE, 0, 0, 0)]), LIST, [INT64_MIN]),
            lambda: eng.facet_list_values(INT, 16), lambda: eng.facet_list_values(LIST, 0),
        ]
        bad_writes += [lambda c=c: eng.set_attr_list(LIST, 0, c) for c in bad_lists]
        bad_writes += [lambda c=c: eng.set_attr_list_at(LIST, np.arange(len(c), dtype=np.int64), c) for c in bad_lists]
        # every entry that needs a scalar column, given the list column
        tokens, offsets = pair.qs[:4], np.array([0, 2, 4], np.int64)
        edges = np.array([1, 2], np.int64)
        z = C.c_int64(0)
        counts = (C.c_int64 * 4)()
        scalar_only = [
            lambda: eng.search_distinct(pair.qs, 3, LIST), lambda: eng.search_grouped(pair.qs, 3, 2, LIST),
            lambda: eng.search_maxsim(tokens, offsets, 3, LIST), lambda: eng.where_ordered(LIST, 5),
            lambda: eng.facet_values(LIST, 16),
            lambda: eng._check(eng._lib.mlvdb_facet_bins(eng.handle, LIST, None, edges.ctypes.data, 2, counts, C.byref(z),
                                                         C.byref(z)), "facet_bins"),
        ]
        for i, call in enumerate(bad_writes + scalar_only):
            with pytest.raises(RuntimeError, match=r"\(1\)"):
                call()
            assert eng.where_count(prog([(W.HAS, LIST, COMMON, 0)])) == before, i  # nothing was written; the handle answers
        pair.check_state("after the refusals")
    finally:
        pair.close()


# ---------------------------------------------------------------- 4. writes
def test_writes_by_label_and_by_filter_follow_the_model():
    pair = Pair("l2", 2000, seed=4)
    rng = pair.rng
    programs = [p for _, p in fixed_programs()]
    try:
        dead = np.flatnonzero(pair.model._deleted)
        live = np.flatnonzero(~pair.model._deleted)
        labels = np.concatenate([rng.choice(live, 300, replace=False), dead[:40]])
        rng.shuffle(labels)
        new = random_lists(rng, labels.size)
        got, want = pair.both("set_attr_list_at", LIST, labels, csr(new))
        assert got == want == 300  # the tombstoned labels are skipped
        pair.check_state("set_at")
        # assign where the predicate reads the column it assigns: rows holding COMMON get [RARE, 9]
        where = prog([(W.HAS, LIST, COMMON, 0)])
        got, want = pair.both("update_where_list", where, LIST, np.array([9, RARE], np.int64))
        assert got == want > 500
        pair.check_state("update_where assign")
        assert pair.eng.where_count(where) == 0 and pair.eng.where_count(prog([(W.HAS, LIST, 9, 0)])) == got
        # clear where the list is empty or long; an empty list for the rows that had none
        where = prog([(W.LEN, LIST, 0, 0), (W.LEN, LIST, 255, 255), (W.OR, 0, 0, 0)])
        got, want = pair.both("update_where_list", where, LIST, None)
        assert got == want > 50
        got, want = pair.both("update_where_list", prog([(W.EXISTS, LIST, 0, 0), (W.NOT, 0, 0, 0), (W.GE, INT, 0, 0),
                                                         (W.AND, 0, 0, 0)]), LIST, np.zeros(0, np.int64))
        assert got == want > 50
        pair.check_state("update_where clear / empty")
        for i, p in enumerate(programs):
            pair.check_program(p, f"after the updates, program {i}", search=False)
        # delete by a list program
        where = prog([(W.HAS, LIST, RARE, 0), (W.LT, FLT, W.float_bits(0.0), 0), (W.AND, 0, 0, 0)])
        got, want = pair.both("tombstone_where", where)
        assert np.array_equal(got, want) and got.size > 100
        pair.check_state("tombstone_where")
        for i, p in enumerate(programs):
            pair.check_program(p, f"after the delete, program {i}", search=i % 5 == 0)
    finally:
        pair.close()


# ---------------------------------------------------------------- 5. compact and reset
@pytest.mark.parametrize("tombstones", [True, False])
def test_compact_repacks_the_pool_and_reset_empties_it(tombstones):
    pair = Pair("cosine", 2000 if tombstones else 300, seed=5)
    rng = pair.rng
    try:
        if not tombstones:  # drop the tombstones first: the compaction under test is then the identity, which repacks too
            got, want = pair.both("compact")
            assert np.array_equal(got, want)
            pair.rows = pair.rows[want]
        n = pair.model.counts()[0]
        for _ in range(2):  # half the lists overwritten twice: their old values stay behind in the pool
            labels = rng.choice(n, n // 2, replace=False)
            pair.both("set_attr_list_at", LIST, labels, csr(random_lists(rng, labels.size)))
        pair.both("update_where_list", prog([(W.HAS, LIST, 7, 0)]), LIST, np.array([1, 7, 8], np.int64))  # one shared range
        used, live = pair.eng.list_stats(LIST)
        assert (used, live) == pair.model.list_stats(LIST) and used > live > 0
        got, want = pair.both("compact")
        assert np.array_equal(got, want)
        used, live = pair.eng.list_stats(LIST)
        assert used == live == pair.model.list_stats(LIST)[1] == \
            sum(len(r) for r in pair.model._lists[LIST] if r is not None)
        pair.check_state("compacted")
        pair.rows = pair.rows[want]
        for name, p in fixed_programs():
            pair.check_program(p, f"compacted: {name}", search=name in ("has common", "any 300", "len 2..5", "has and int"))
        # rows appended after a compaction, and a second compaction with nothing to reclaim
        more = csr(random_lists(rng, 10))
        for e in (pair.eng, pair.model):
            first = e.append(pair.rows[:10])
            e.set_attr_list(LIST, first, more)
            e.compact()
        assert pair.eng.list_stats(LIST) == pair.model.list_stats(LIST)
        pair.check_state("compacted again")
        pair.eng.reset()
        assert pair.eng.list_stats(LIST) == (0, 0) and pair.eng.counts() == (0, 0)
        assert pair.eng.where_count(prog([(W.EXISTS, LIST, 0, 0)])) == 0
        fresh = TagsOracleEngine(D, "cosine")  # the definitions remain: no define_attr on the reset engine
        for a, kind in ((LIST, "int64_list"), (INT, "int64"), (FLT, "float64")):
            fresh.define_attr(a, kind)
        lists = random_lists(rng, 100)
        for e in (pair.eng, fresh):
            assert e.append(pair.rows[:100]) == 0
            e.set_attr_list(LIST, 0, csr(lists))
        pair.model = fresh
        pair.check_state("after the reset")
        assert pair.eng.where_count(prog([(W.HAS, LIST, COMMON, 0)])) == fresh.where_count(prog([(W.HAS, LIST, COMMON, 0)])) > 0
    finally:
        pair.close()


# ---------------------------------------------------------------- 6. list facets
def test_list_facets_count_rows_per_value():
    pair = Pair("cosine", 2000, seed=6)
    try:
        live = ~pair.model._deleted
        for name, where in [("all rows", None)] + [(n, p) for n, p in fixed_programs()
                                                   if n in ("has common", "len 2..5", "has and int", "has nothing", "not exists")]:
            mask = live if where is None else pair.model.match(where)
            counts = Counter(v for i in np.flatnonzero(mask).tolist() for v in pair.model._lists[LIST][i] or ())
            values, got, matched, absent = pair.eng.facet_list_values(LIST, 4096, where=where)
            assert values.tolist() == sorted(counts) and got.tolist() == [counts[v] for v in sorted(counts)], name
            assert matched == int(mask.sum()), name
            assert absent == sum(not pair.model._lists[LIST][i] for i in np.flatnonzero(mask).tolist()), name
        distinct = len(Counter(v for i in np.flatnonzero(live).tolist() for v in pair.model._lists[LIST][i] or ()))
        assert distinct > 255
        assert pair.eng.facet_list_values(LIST, distinct)[0].size == distinct  # exactly enough
        with pytest.raises(FacetOverflow):
            pair.eng.facet_list_values(LIST, distinct - 1)
    finally:
        pair.close()


def test_the_second_sweep_of_a_capped_grid_counts_and_facets():
    """where_eval_kernel and facet_list_values_kernel cover 1,048,576 rows per sweep of their grid: 1,100,000 rows make the
    stride loop run again."""
    n, d = 1_100_000, 4
    rng = np.random.default_rng(9)
    eng = HipScanEngine(d, "l2", device=0)
    try:
        eng.append(rng.standard_normal((n, d), dtype=np.float32))
        eng.define_attr(LIST, "int64_list")
        i = np.arange(n, dtype=np.int64)
        first, second = i % 7, 7 + i % 5  # two elements per row, ascending
        values = np.stack([first, second], axis=1).ravel()
        eng.set_attr_list(LIST, 0, W.ListColumn(2 * np.arange(n + 1, dtype=np.int64), values, np.ones(n, np.uint8)))
        dead = np.arange(0, n, 11, dtype=np.int64)
        eng.tombstone(dead)
        live = np.ones(n, bool)
        live[dead] = False
        assert eng.where_count(prog([(W.HAS, LIST, 3, 0)])) == int((live & (first == 3)).sum())
        assert eng.where_count(prog([(W.HAS_ALL, LIST, 0, 2)], [3, 9])) == int((live & (first == 3) & (second == 9)).sum())
        tail = prog([(W.HAS, LIST, 11, 0)])
        assert np.array_equal(eng.where_labels(tail)[-5:], np.flatnonzero(live & (second == 11))[-5:])
        got_values, got_counts, matched, absent = eng.facet_list_values(LIST, 64)
        want = np.bincount(first[live], minlength=12) + np.bincount(second[live], minlength=12)
        assert got_values.tolist() == list(range(12)) and got_counts.tolist() == want.tolist()
        assert matched == int(live.sum()) and absent == 0
        assert eng.list_stats(LIST) == (2 * n, 2 * int(live.sum()))
    finally:
        eng.close()


# ---------------------------------------------------------------- 7. through Index on the real engine
def test_index_with_tags_on_the_device(tmp_path):
    rng = np.random.default_rng(12)
    schema = {"tags": "str[]", "year": "int"}
    metas = [{k: v for k, v in m.items() if k in ("tags", "year")} for m in random_tag_metadata(rng, 600)]
    vectors = [Vector(values=rng.standard_normal(32).astype(np.float32).tolist(), metadata=m) for m in metas]
    index = Index(space="cosine", attributes=schema)
    try:
        for lo in (0, 200, 400):
            index.add(vectors[lo:lo + 200], "ns")
        model = {v.id: dict(m) for v, m in zip(vectors, metas)}
        order = [v.id for v in vectors]

        def matching(where):
            return [i for i in order if i in model and py_match(where, model[i], schema)]

        def check(tag):
            for where in ({"tags": "jazz"}, {"tags": {"$all": ["jazz", "live"]}}, {"tags": {"$nin": ["mono", "zydeco"]}},
                          {"tags": {"$size": {"$gte": 2}}, "year": {"$lt": 1960}}, {"tags": {"$exists": False}},
                          {"$or": [{"tags": {"$size": 0}}, {"tags": {"$in": ["vinyl", "fresh"]}}]}):
                want = matching(where)
                assert index.count("ns", where) == len(want), (tag, where)
                assert index.query_by_metadata("ns", where) == want, (tag, where)
            counts = Counter(e for m in model.values() for e in set(m.get("tags") or ()))
            got = index.facets("ns", "tags", order="value")
            assert got["values"] == sorted(counts.items()) and got["matched"] == len(model), tag
            assert got["absent"] == sum(not m.get("tags") for m in model.values()), tag

        check("ingest")
        where = {"tags": "jazz", "year": {"$gte": 1955}}
        allowed = matching(where)
        q = np.stack([np.asarray(vectors[i].values, np.float32) for i in (3, 77, 401)])
        hits = index.search_many(q, 5, "ns", "cosine", where=where)
        rows = np.stack([np.asarray(v.values, np.float32) for v in vectors])
        deleted = np.array([v.id not in set(allowed) for v in vectors])
        ol, _, oc = exact_scan.knn(q, rows, 5, "cosine", deleted=deleted)
        assert [[order[j] for j in r[:c]] for r, c in zip(ol, oc)] == [r[:c].tolist() for r, c in zip(hits.ids(), hits.counts)]
        assert index.update_attributes(order[:50], [{"tags": ["fresh", "jazz"]}, {"tags": None}] * 25, "ns") == 50
        for j, i in enumerate(order[:50]):
            model[i]["tags"] = ["fresh", "jazz"] if j % 2 == 0 else None
        check("update_attributes")
        n = len(matching({"tags": "fresh"}))
        assert index.update_where("ns", {"tags": "fresh"}, {"tags": ["stale", "mono"]}) == n == 25
        for i in matching({"tags": "fresh"}):
            model[i]["tags"] = ["stale", "mono"]
        check("update_where")
        gone = matching({"tags": {"$all": ["blues"]}, "year": {"$lt": 1962}})
        assert index.remove_where("ns", {"tags": {"$all": ["blues"]}, "year": {"$lt": 1962}}, return_ids=True) == gone
        assert len(gone) > 10
        for i in gone:
            del model[i]
        check("remove_where")
        index.save_index(str(tmp_path))
        assert '"mlvdb-index-v3"' in (tmp_path / "index.json").read_text()
        loaded = Index(space="cosine")
        try:
            assert loaded.load_index(str(tmp_path)) and loaded.attributes == schema
            index, kept = loaded, index
            check("loaded")
            assert index.compact("ns")
            order = [i for i in order if i in model]
            check("loaded and compacted")
            used, live = index._ns["ns"].engine.list_stats(0)
            assert used == live == sum(len(set(m.get("tags") or ())) for m in model.values())
        finally:
            loaded.close()
            index = kept
    finally:
        index.close()
