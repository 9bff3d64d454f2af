"""Facet counts and histograms on the MI355X (include/mlvdb_facet.h) against NumPy: np.unique / np.searchsorted over the
live matching rows (tests/facet_helpers.py).  Every comparison is exact equality of integers.  Rows are 4 floats wide, so the
row store is negligible; the shapes are the smallest at which the kernels take another path: wave and block edges, one size
past a whole pass of the grid, cardinalities around the wave, the block table and the global table, and keys built with
the mirrored hash to share a probe chain."""
from collections import Counter

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import FacetOverflow, HipScanEngine
from mlvectordb_amd.vector import Vector
from tests import facet_helpers as F
from tests.conftest import dump_mismatch
from tests.where_helpers import (FLOAT_POOL, INT_POOL, SCHEMA, eval_program, hostile_columns, program_depth, py_match,
                                 random_filter, random_metadata, random_raw_program)

pytestmark = pytest.mark.gpu

NOTHING = W.Program(np.array([(W.TRUE, 0, 0, 0), (W.NOT, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
EVERYTHING = W.Program(np.array([(W.TRUE, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))


def _engine(cols, n=None, tomb=None):
    """An index of n rows of 4 floats with the columns `cols` (attr -> int64 / float64 array of n values)."""
    n = len(next(iter(cols.values()))) if n is None else n
    eng = HipScanEngine(4, "l2", device=0)
    if n:
        eng.append(np.ones((n, 4), dtype=np.float32))
    for a, col in cols.items():
        eng.define_attr(a, col.dtype.name)
        if n:
            eng.set_attr(a, 0, col)
    if tomb is not None and tomb.any():
        eng.tombstone(np.flatnonzero(tomb))
    return eng


def _check_values(eng, attr, col, live, max_values, program=None, cols=None, tag="values"):
    """facet_values twice (bit-identical) against the oracle; matched against where_count of the same program."""
    mask = live if program is None else live & eval_program(program, cols, col.size)
    want = F.values_oracle(col, mask)
    got = eng.facet_values(attr, max_values, where=program)
    again = eng.facet_values(attr, max_values, where=program)
    ok = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    if not ok:
        dump_mismatch(f"facet_{tag}", got_values=got[0], got_counts=got[1], want_values=want[0], want_counts=want[1],
                      scalars=np.array(got[2:] + want[2:]))
    assert got[2:] == want[2:], f"{tag}: (matched, absent) {got[2:]}, NumPy {want[2:]}"
    assert np.array_equal(got[0], want[0]), f"{tag}: {got[0].size} values, NumPy {want[0].size}"
    assert np.array_equal(got[1], want[1]), f"{tag}: counts differ"
    assert got[0].dtype == got[1].dtype == np.int64 and int(got[1].sum()) + got[3] == got[2]
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]) and got[2:] == again[2:], f"{tag}: two calls"
    if program is not None:
        assert got[2] == eng.where_count(program), f"{tag}: matched != where_count"
    return got


def _check_bins(eng, attr, col, edges, live, program=None, cols=None, tag="bins"):
    mask = live if program is None else live & eval_program(program, cols, col.size)
    want = F.bins_oracle(col, edges, mask)
    got = eng.facet_bins(attr, edges, where=program)
    again = eng.facet_bins(attr, edges, where=program)
    if not (np.array_equal(got[0], want[0]) and got[1:] == want[1:]):
        dump_mismatch(f"facet_{tag}", got=got[0], want=want[0], edges=edges, scalars=np.array(got[1:] + want[1:]))
    assert got[1:] == want[1:], f"{tag}: (matched, absent) {got[1:]}, NumPy {want[1:]}"
    assert np.array_equal(got[0], want[0]), f"{tag}: bins differ at {np.flatnonzero(got[0] != want[0])[:8]}"
    assert got[0].dtype == np.int64 and got[0].size == edges.size + 1 and int(got[0].sum()) + got[2] == got[1]
    assert np.array_equal(got[0], again[0]) and got[1:] == again[1:], f"{tag}: two calls"
    if program is not None:
        assert got[1] == eng.where_count(program), f"{tag}: matched != where_count"
    return got


def _with_absent(rng, col, share=0.1):
    col = col.copy()
    col[rng.random(col.size) < share] = F.ABSENT
    return col


# ---------------------------------------------------------------- row counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 40_000, F.GRID_ROWS + 300])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    ints = _with_absent(rng, rng.integers(-3, 9, n).astype(np.int64))
    if n > F.GRID_ROWS:
        ints[F.GRID_ROWS:] = 1000 + np.arange(n - F.GRID_ROWS)  # the rows of the second pass hold values of their own
    floats = rng.integers(-3, 9, n).astype(np.float64) / 2
    floats[rng.random(n) < 0.1] = np.nan
    tomb = rng.random(n) < 0.1
    eng = _engine({0: ints, 1: floats}, n, tomb)
    try:
        got = _check_values(eng, 0, ints, ~tomb, 512, tag=f"rows_{n}")
        if n == 0:
            assert got[0].size == 0 and got[2:] == (0, 0)
        _check_bins(eng, 0, ints, np.array([-2, 0, 1, 5, 1100], np.int64), ~tomb, tag=f"rows_{n}_i")
        _check_bins(eng, 1, floats, np.array([-1.0, 0.0, 0.5, 3.5]), ~tomb, tag=f"rows_{n}_f")
        if n:
            sel = W.Program(np.array([(W.GE, 0, 2, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
            _check_values(eng, 0, ints, ~tomb, 512, sel, {0: ints, 1: floats}, tag=f"rows_{n}_where")
    finally:
        eng.close()


# ---------------------------------------------------------------- cardinality
N_CARD = 40_000


def _card_column(rng, card):
    if card == "unique":
        return rng.permutation(N_CARD).astype(np.int64) * 7 - 100_000
    if card == "skewed":  # one value on 90 % of the rows, the rest unique
        col = 10_000_000 + np.arange(N_CARD, dtype=np.int64)
        col[rng.random(N_CARD) < 0.9] = 42
        return col
    values = rng.choice(np.arange(-(10 ** 6), 10 ** 6), card, replace=False).astype(np.int64)
    col = values[rng.integers(0, card, N_CARD)]
    col[:card] = values  # every value at least once
    return col[rng.permutation(N_CARD)]


@pytest.mark.parametrize("card", [1, 2, 6, 64, 65, F.LDS_SLOTS - 1, F.LDS_SLOTS, F.LDS_SLOTS + 1, "unique", "skewed"])
def test_cardinalities(card):
    rng = np.random.default_rng(card if isinstance(card, int) else len(card))
    col = _card_column(rng, card)
    distinct = np.unique(col).size
    assert distinct == (card if isinstance(card, int) else distinct)
    eng = _engine({0: col})
    try:
        live = np.ones(N_CARD, bool)
        got = _check_values(eng, 0, col, live, 65536, tag=f"card_{card}")
        assert got[0].size == distinct and got[3] == 0
        _check_values(eng, 0, col, live, distinct, tag=f"card_{card}_tight")  # exactly max_values distinct values
        sel = W.Program(np.array([(W.GT, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
        _check_values(eng, 0, col, live, 65536, sel, {0: col}, tag=f"card_{card}_where")
    finally:
        eng.close()


# ---------------------------------------------------------------- values and probe chains
def test_extreme_values():
    rng = np.random.default_rng(1)
    col = rng.choice(np.array([F.ABSENT + 1, F.INT64_MAX, -1, 0, F.ABSENT], np.int64), 3000)
    eng = _engine({0: col})
    try:
        got = _check_values(eng, 0, col, np.ones(3000, bool), 4, tag="extremes")
        assert got[0].tolist() == [F.ABSENT + 1, -1, 0, F.INT64_MAX]
    finally:
        eng.close()


def test_keys_sharing_one_probe_chain():
    """20 keys with the same first slot in the block table (probe bound 8): within one block -- rows 0..255 -- the chain is
    longer than the bound, so the later keys go straight to the global table; they share the first slot of the 64-slot global
    table of max_values = 32 too.  Then 40 keys that share one slot of the 128-slot global table of max_values = 64."""
    rng = np.random.default_rng(2)
    lds_chain = F.colliding_keys(F.LDS_SLOTS, 20, slot=4095)  # (the chain wraps round the end of the table)
    assert set((F.facet_hash(lds_chain) & np.uint64(63)).tolist()) == {63}
    glob_chain = F.colliding_keys(128, 40, slot=127, start=10 ** 9)
    assert np.unique(F.facet_hash(glob_chain) & np.uint64(F.LDS_SLOTS - 1)).size > 8
    for chain, max_values in ((lds_chain, 32), (glob_chain, 64), (np.concatenate([lds_chain, glob_chain]), 65536)):
        col = chain[rng.integers(0, chain.size, 2000)]
        col[:chain.size] = chain  # all of them inside the first block
        col[rng.random(2000) < 0.05] = F.ABSENT
        eng = _engine({0: col})
        try:
            got = _check_values(eng, 0, col, np.ones(2000, bool), max_values, tag=f"chain_{max_values}")
            assert got[0].size == chain.size
        finally:
            eng.close()


# ---------------------------------------------------------------- overflow
def test_overflow_and_max_values_limits():
    rng = np.random.default_rng(3)
    n = 5000
    col = _with_absent(rng, rng.integers(0, 100, n).astype(np.int64))
    col[:100] = np.arange(100)
    tomb = rng.random(n) < 0.2
    tomb[:100] = False
    eng = _engine({0: col, 1: np.zeros(n)}, n, tomb)
    try:
        want = F.values_oracle(col, ~tomb)
        assert want[0].size == 100
        _check_values(eng, 0, col, ~tomb, 100, tag="overflow_exact")
        for max_values in (99, 50, 1):
            with pytest.raises(FacetOverflow) as err:
                eng.facet_values(0, max_values)
            assert (err.value.matched, err.value.absent) == want[2:] and err.value.n_values > max_values
        one = W.Program(np.array([(W.EQ, 0, 7, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
        two = W.Program(np.array([(W.IN, 0, 0, 2)], W.OP_DTYPE), np.array([7, 8], np.int64))
        got = _check_values(eng, 0, col, ~tomb, 1, one, {0: col}, tag="overflow_one")
        assert got[0].tolist() == [7]
        with pytest.raises(FacetOverflow) as err:
            eng.facet_values(0, 1, where=two)
        assert err.value.matched == int((~tomb & np.isin(col, [7, 8])).sum()) == eng.where_count(two) and err.value.absent == 0
        _check_values(eng, 0, col, ~tomb, F.MAX_VALUES, tag="overflow_largest")
        for bad in (F.MAX_VALUES + 1, 0, -1):
            with pytest.raises(RuntimeError, match=r"failed \(1\).*max_values"):
                eng.facet_values(0, bad)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*int64 column"):
            eng.facet_values(1, 10)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*not defined"):
            eng.facet_values(2, 10)
    finally:
        eng.close()


# ---------------------------------------------------------------- liveness
def test_liveness_tombstones_compaction_and_default_absence():
    rng = np.random.default_rng(4)
    n = 3000
    col = _with_absent(rng, rng.integers(0, 300, n).astype(np.int64))
    fcol = rng.standard_normal(n)
    edges_i, edges_f = np.array([50, 100, 250], np.int64), np.array([-1.0, 0.0, 1.0])
    for share in (0.0, 0.3, 1.0):
        tomb = rng.random(n) < share if share < 1 else np.ones(n, bool)
        eng = _engine({0: col, 3: fcol}, n, tomb)
        try:
            got = _check_values(eng, 0, col, ~tomb, 512, tag=f"live_{share}")
            _check_bins(eng, 0, col, edges_i, ~tomb, tag=f"live_{share}_i")
            _check_bins(eng, 3, fcol, edges_f, ~tomb, tag=f"live_{share}_f")
            if share == 1.0:
                assert got[0].size == 0 and got[2:] == (0, 0)
            old = eng.compact()
            assert np.array_equal(old, np.flatnonzero(~tomb))
            c, f, live = col[old], fcol[old], np.ones(old.size, bool)
            _check_values(eng, 0, c, live, 512, tag=f"compact_{share}")
            _check_bins(eng, 3, f, edges_f, live, tag=f"compact_{share}_f")
            # rows appended after the values were set hold no value
            eng.append(np.ones((70, 4), dtype=np.float32))
            c = np.concatenate([c, np.full(70, F.ABSENT)])
            f = np.concatenate([f, np.full(70, np.nan)])
            live = np.ones(c.size, bool)
            got = _check_values(eng, 0, c, live, 512, tag=f"appended_{share}")
            assert got[3] >= 70
            _check_bins(eng, 3, f, edges_f, live, tag=f"appended_{share}_f")
        finally:
            eng.close()
    eng = _engine({0: np.full(500, F.ABSENT), 1: np.full(500, np.nan)})
    try:
        got = _check_values(eng, 0, np.full(500, F.ABSENT), np.ones(500, bool), 8, tag="all_absent")
        assert got[0].size == 0 and got[2:] == (500, 500)
        got = _check_bins(eng, 1, np.full(500, np.nan), edges_f, np.ones(500, bool), tag="all_absent_f")
        assert got[0].sum() == 0 and got[1:] == (500, 500)
    finally:
        eng.close()


# ---------------------------------------------------------------- filters
def test_raw_programs_over_hostile_columns():
    rng = np.random.default_rng(5)
    n = 5000
    kinds = {0: "int64", 1: "float64", 2: "int64", 3: "float64"}
    cols = hostile_columns(rng, n, kinds)
    tomb = rng.random(n) < 0.1
    eng = _engine(cols, n, tomb)
    programs = [NOTHING, EVERYTHING]
    for j in range(40):
        size = 64 if j < 2 or rng.random() < 0.15 else int(rng.integers(1, 24))
        programs.append(random_raw_program(rng, kinds, size, deep=(j == 0)))
    assert program_depth(programs[2]) == W.MAX_DEPTH and programs[2].ops.size == programs[3].ops.size == W.MAX_OPS
    edges_i = np.array([F.ABSENT + 2, 0, 2, 3, F.INT64_MAX], np.int64)
    edges_f = np.array([-1.0, 0.0, 1.0, 1.5])
    try:
        matched = []
        for j, p in enumerate([None] + programs):
            got = _check_values(eng, 0, cols[0], ~tomb, 64, p, cols, tag=f"prog_{j}")
            _check_bins(eng, 2, cols[2], edges_i, ~tomb, p, cols, tag=f"prog_{j}_i")
            _check_bins(eng, 1, cols[1], edges_f, ~tomb, p, cols, tag=f"prog_{j}_f")
            matched.append(got[2])
        assert matched[0] == matched[2] == int((~tomb).sum()) and matched[1] == 0
        assert any(0 < m < matched[0] for m in matched[3:])
    finally:
        eng.close()


# ---------------------------------------------------------------- bins
@pytest.mark.parametrize("n_edges", [1, 2, 63, 64, 65, F.MAX_EDGES])
def test_bin_edge_counts(n_edges):
    rng = np.random.default_rng(n_edges)
    n = 20_000
    edges_i = np.sort(rng.choice(np.arange(-50_000, 50_000), n_edges, replace=False)).astype(np.int64)
    ints = rng.integers(-60_000, 60_000, n).astype(np.int64)
    ints[: min(n, n_edges)] = edges_i[:n]  # values equal to edges
    ints = _with_absent(rng, ints, 0.05)
    edges_f = edges_i / 8.0
    floats = rng.integers(-60_000, 60_000, n) / 8.0
    floats[: min(n, n_edges)] = edges_f[:n]
    floats[rng.random(n) < 0.05] = np.nan
    tomb = rng.random(n) < 0.1
    eng = _engine({0: ints, 1: floats}, n, tomb)
    try:
        got = _check_bins(eng, 0, ints, edges_i, ~tomb, tag=f"edges_{n_edges}_i")
        assert got[0][0] > 0 and got[0][-1] > 0
        _check_bins(eng, 1, floats, edges_f, ~tomb, tag=f"edges_{n_edges}_f")
        sel = W.Program(np.array([(W.LT, 1, W.float_bits(100.0), 0)], W.OP_DTYPE), np.zeros(0, np.int64))
        _check_bins(eng, 0, ints, edges_i, ~tomb, sel, {0: ints, 1: floats}, tag=f"edges_{n_edges}_where")
    finally:
        eng.close()


def test_bins_at_the_ends_of_both_types():
    rng = np.random.default_rng(6)
    n = 4000
    ints, floats = rng.choice(INT_POOL, n), rng.choice(FLOAT_POOL, n)
    live = np.ones(n, bool)
    eng = _engine({0: ints, 1: floats})
    try:
        # integer comparisons, never through double: INT64_MAX - 1 and INT64_MAX lie on different sides of INT64_MAX
        got = _check_bins(eng, 0, ints, np.array([F.INT64_MAX], np.int64), live, tag="ends_max")
        assert got[0][1] == int((ints == F.INT64_MAX).sum()) > 0 and int((ints == F.INT64_MAX - 1).sum()) > 0
        got = _check_bins(eng, 0, ints, np.array([F.ABSENT + 1], np.int64), live, tag="ends_min")
        assert got[0][0] == 0 and got[2] == int((ints == F.ABSENT).sum()) > 0
        _check_bins(eng, 0, ints, np.array([F.ABSENT + 1, F.ABSENT + 2, -1, 0, 1, 2, 3, 7, F.INT64_MAX - 1, F.INT64_MAX], np.int64),
                    live, tag="ends_pool")
        edges = np.array([-np.inf, -1.0, 0.0, 5e-324, 1.0, np.nextafter(1.0, np.inf), np.inf])
        got = _check_bins(eng, 1, floats, edges, live, tag="ends_float")
        assert got[2] == int(np.isnan(floats).sum()) > 0 and got[0][0] == 0
        assert got[0][-1] == int((floats == np.inf).sum()) > 0 and got[0][1] >= int((floats == -np.inf).sum()) > 0
        assert got[0][3] == int((floats == 0.0).sum()) and int((np.signbit(floats) & (floats == 0.0)).sum()) > 0  # -0.0 == 0.0
    finally:
        eng.close()


def test_refused_edges():
    n = 100
    eng = _engine({0: np.arange(n, dtype=np.int64), 1: np.arange(n, dtype=np.float64)})
    try:
        bad_i = [np.array([3, 2]), np.array([1, 2, 2]), np.array([F.ABSENT]), np.array([F.ABSENT, 0]), np.zeros(0),
                 np.arange(F.MAX_EDGES + 1)]
        bad_f = [np.array([1.0, 0.5]), np.array([0.0, 0.0]), np.array([-0.0, 0.0]), np.array([np.nan]), np.array([0.0, np.nan]),
                 np.array([np.nan, 1.0]), np.array([np.inf, np.inf]), np.zeros(0), np.arange(F.MAX_EDGES + 1.0)]
        for attr, dtype, cases in ((0, np.int64, bad_i), (1, np.float64, bad_f)):
            for edges in cases:
                with pytest.raises(RuntimeError, match=r"facet_bins failed \(1\)"):
                    eng.facet_bins(attr, edges.astype(dtype))
        with pytest.raises(RuntimeError, match=r"failed \(1\).*not defined"):
            eng.facet_bins(5, np.array([1], np.int64))
        with pytest.raises(RuntimeError, match="int64 column"):  # the binding refuses edges of the other type
            eng.facet_bins(0, np.array([1.0]))
        assert eng.facet_bins(1, np.array([-np.inf, np.inf]))[0].tolist() == [0, n, 0]
    finally:
        eng.close()


# ---------------------------------------------------------------- Index and QueryProcessor
def _want(live, by, where):
    rows = [v.metadata for v in live if where is None or py_match(where, v.metadata)]
    present = [m[by] for m in rows if m.get(by) is not None and m[by] == m[by]]
    return present, len(rows), len(rows) - len(present)


def test_index_and_query_processor_facets_equal_the_dict_semantics(tmp_path):
    rng = np.random.default_rng(7)
    n = 3000
    index = Index(space="l2", attributes=SCHEMA)
    qp = QueryProcessor(InMemoryStorage(), index)
    try:
        vecs = [Vector(values=rng.standard_normal(4).astype(np.float32), metadata=m) for m in random_metadata(rng, n)]
        vecs += [Vector(values=np.ones(4, np.float32), metadata={"genre": "dub"}) for _ in range(3)]  # tombstoned below
        qp.upsert_many(vecs[:2000], "ns")
        qp.upsert_many(vecs[2000:], "ns")
        vecs = list(qp._storage.namespace_map["ns"])  # the stored vectors carry the ids minted at upsert
        gone = {v.id for v in vecs[::9]} | {v.id for v in vecs[n:]}
        qp.delete(list(gone), "ns")
        live = [v for v in vecs if v.id not in gone]
        year_edges, price_edges = [1960, 1975, 1990, 2005, 2020], [0, 9.9, 25, 50.0, 99.9]

        def check(index, qp):
            for f in [None] + [random_filter(rng) for _ in range(20)]:
                for by in ("genre", "year", "in_stock"):
                    present, matched, absent = _want(live, by, f)
                    want = {"values": sorted(Counter(present).items(), key=lambda p: (-p[1], p[0])), "matched": matched,
                            "absent": absent}
                    assert index.facets("ns", by, f) == want, (by, f)
                    assert qp.facets(by, where=f, namespace="ns") == want
                    if f is not None:
                        assert matched == index.count("ns", f)
                        assert qp.facets(by, where=lambda m: py_match(f, m), namespace="ns") == want
                for by, edges in (("year", year_edges), ("price", price_edges)):
                    present, matched, absent = _want(live, by, f)
                    e = np.asarray(edges, dtype=np.int64 if by == "year" else np.float64)
                    bins = np.bincount(np.searchsorted(e, np.asarray(present, dtype=e.dtype), side="right"), minlength=e.size + 1)
                    got = index.histogram("ns", by, edges, f)
                    assert got["counts"].tolist() == bins.tolist() and (got["matched"], got["absent"]) == (matched, absent), (by, f)
                    got = qp.histogram(by, edges, where=f, namespace="ns")
                    assert got["counts"].tolist() == bins.tolist()
            assert "dub" not in dict(index.facets("ns", "genre")["values"])
            both = index.facets("ns", ["genre", "in_stock"], order="value", limit=3)
            assert both["in_stock"]["values"][0][0] is False and len(both["genre"]["values"]) == 3
            with pytest.raises(ValueError, match="max_values=10"):
                index.facets("ns", "year", max_values=10)

        check(index, qp)
        assert index.save_index(str(tmp_path / "snap"))
        loaded = Index(space="l2", attributes=SCHEMA)
        try:
            assert loaded.load_index(str(tmp_path / "snap"))
            check(loaded, QueryProcessor(qp._storage, loaded))
        finally:
            loaded.close()
    finally:
        index.close()
