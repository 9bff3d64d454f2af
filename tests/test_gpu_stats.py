"""Attribute statistics on the MI355X (include/mlvdb_stats.h) against the model of tests/stats_helpers.py: Python integers
for the sums, totalOrder min / max, the fixed-point rule of float sums written out.  Every comparison is exact equality --
floats by their bits --, every call is made twice and compared, and ``matched`` is compared with ``where_count``.  Rows are 4
floats wide, so the row store is negligible; the shapes are the smallest at which the kernels take another path: wave and
block edges, one size past a whole pass of the grid, cardinalities around the peel rounds, the wave, the block table and
the probe bound, and sums that need the high word and carry both ways."""
import math

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor
from mlvectordb_amd import stats as host_stats
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine, StatsOverflow
from mlvectordb_amd.vector import Vector
from tests import stats_helpers as S
from tests.conftest import dump_mismatch
from tests.where_helpers import (SCHEMA, eval_program, hostile_columns, program_depth, py_match, random_filter,
                                 random_metadata, random_raw_program)

pytestmark = pytest.mark.gpu

NOTHING = W.Program(np.array([(W.TRUE, 0, 0, 0), (W.NOT, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
EVERYTHING = W.Program(np.array([(W.TRUE, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
INT64_MAX, INT64_MIN1 = int(S.INT64_MAX), -int(S.INT64_MAX)  # (INT64_MIN itself marks absent)


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check(eng, attr, by, cols, live, max_groups=1, program=None, tag="stats"):
    """attr_stats twice (identical bytes) against the model; matched against where_count of the same program.  Returns the
    call's answer with the sums as Python ints."""
    col, by_col = cols[attr], None if by is None else cols[by]
    mask = live if program is None else live & eval_program(program, cols, col.size)
    want = S.stats_oracle(col, by_col, mask)
    got = eng.attr_stats(attr, by, max_groups, where=program)
    again = eng.attr_stats(attr, by, max_groups, where=program)
    assert got[0].size == want[0].size, f"{tag}: {got[0].size} groups, model {want[0].size}"
    has = want[2] > 0  # min / max are unspecified where nothing is present
    sums = [host_stats.int128(h, l) for h, l in zip(got[5].tolist(), got[6].tolist())]
    ok = got[7:] == want[6:] and all(np.array_equal(got[i], want[i]) for i in range(3)) and sums == want[5] and \
        np.array_equal(_bits(got[3])[has], _bits(want[3])[has]) and np.array_equal(_bits(got[4])[has], _bits(want[4])[has])
    if not ok:
        dump_mismatch(f"stats_{tag}", **{f"got_{i}": np.asarray(got[i]) for i in range(7)},
                      **{f"want_{i}": np.asarray(want[i]) for i in range(5)}, scalars=np.array(got[7:] + want[6:]))
    assert got[7:] == want[6:], f"{tag}: (matched, by_absent) {got[7:]}, model {want[6:]}"
    assert np.array_equal(got[0], want[0]), f"{tag}: {got[0].size} groups, model {want[0].size}"
    assert np.array_equal(got[1], want[1]), f"{tag}: rows differ"
    assert np.array_equal(got[2], want[2]), f"{tag}: counts differ"
    assert np.array_equal(_bits(got[3])[has], _bits(want[3])[has]), f"{tag}: min differs"
    assert np.array_equal(_bits(got[4])[has], _bits(want[4])[has]), f"{tag}: max differs"
    bad = [g for g in range(len(sums)) if sums[g] != want[5][g]]
    assert not bad, f"{tag}: sums differ in groups {bad[:8]}: {[(sums[g], want[5][g]) for g in bad[:3]]}"
    assert got[3].dtype == got[4].dtype == col.dtype and got[6].dtype == np.uint64
    assert all(a.dtype == np.int64 for a in (got[0], got[1], got[2], got[5])) and int(got[1].sum()) + got[8] == got[7]
    assert all(_bits(a).tobytes() == _bits(b).tobytes() for a, b in zip(got[:7], again[:7])) and got[7:] == again[7:], \
        f"{tag}: two calls"
    if program is not None:
        assert got[7] == eng.where_count(program), f"{tag}: matched != where_count"
    return got[:5] + (sums,) + got[7:]


def _final_sums(got, cols, attr, by, live):
    """The doubles the host makes of a float call's sums, checked against the model's single rounding, by their bits."""
    col, out = cols[attr], []
    for g, key in enumerate(got[0].tolist()):
        member = live if by is None else live & (cols[by] == key)
        want = S.float_sum_model(col[member])
        mine = host_stats.float_sum(got[5][g], float(got[3][g]), float(got[4][g])) if got[2][g] else 0.0
        assert np.float64(mine).tobytes() == np.float64(want).tobytes() or (math.isnan(mine) and math.isnan(want)), \
            (g, key, mine, want)
        out.append(mine)
    return out


def _with_absent(rng, col, share=0.1):
    col = col.copy()
    col[rng.random(col.size) < share] = np.nan if col.dtype == np.float64 else S.ABSENT
    return col


# ---------------------------------------------------------------- row counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 40_000, S.GRID_ROWS + 300])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    ints = _with_absent(rng, rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64))
    floats = _with_absent(rng, np.round(rng.uniform(-50, 1000, n), 2))
    by = _with_absent(rng, rng.integers(-3, 9, n).astype(np.int64))
    if n > S.GRID_ROWS:
        by[S.GRID_ROWS:] = 1000 + np.arange(n - S.GRID_ROWS) % 7  # the rows of the second pass hold groups of their own
    tomb = rng.random(n) < 0.1
    cols = {0: ints, 1: floats, 2: by}
    eng = _engine(cols, n, tomb)
    try:
        sel = W.Program(np.array([(W.GE, 2, 2, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
        for attr in (0, 1):
            got = _check(eng, attr, None, cols, ~tomb, 1, tag=f"rows_{n}_{attr}")
            assert got[0].tolist() == [0] and (n or (got[1].tolist(), got[2].tolist(), got[5]) == ([0], [0], [0]))
            grouped = _check(eng, attr, 2, cols, ~tomb, 64, tag=f"rows_{n}_{attr}_by")
            assert grouped[0].size == (0 if n == 0 else np.unique(by[~tomb & (by != S.ABSENT)]).size)
            if n:
                _check(eng, attr, None, cols, ~tomb, 1, sel, tag=f"rows_{n}_{attr}_where")
                _check(eng, attr, 2, cols, ~tomb, 64, sel, tag=f"rows_{n}_{attr}_by_where")
        if n:
            _final_sums(_check(eng, 1, None, cols, ~tomb, 1), cols, 1, None, ~tomb)
    finally:
        eng.close()


# ---------------------------------------------------------------- cardinality of by
N_CARD = 40_000
CHAIN = S.LDS_PROBES + 12  # keys that share one first slot of the block table: the later ones pass the probe bound


def _by_column(rng, card):
    if card == "unique":
        return rng.permutation(N_CARD).astype(np.int64) * 7 - 100_000
    if card == "chain":
        values = S.colliding_keys(S.LDS_SLOTS, CHAIN, slot=S.LDS_SLOTS - 1)  # (the chain wraps round the end of the table)
    else:
        values = rng.choice(np.arange(-(10 ** 6), 10 ** 6), card, replace=False).astype(np.int64)
    col = values[rng.integers(0, values.size, N_CARD)]
    col[:values.size] = values  # every value at least once
    return col if card == "chain" else col[rng.permutation(N_CARD)]  # (the chain: all of it inside the first block)


@pytest.mark.parametrize("card", [1, 2, S.PEEL_ROUNDS, S.PEEL_ROUNDS + 1, 64, 65, S.LDS_SLOTS - 1, S.LDS_SLOTS,
                                  S.LDS_SLOTS + 1, "chain", "unique"])
def test_cardinalities(card):
    rng = np.random.default_rng(card if isinstance(card, int) else len(card))
    by = _by_column(rng, card)
    distinct = np.unique(by).size
    assert distinct == {"chain": CHAIN, "unique": N_CARD}.get(card, card)
    if card == "chain":
        assert np.unique(S.facet_hash(np.unique(by)) & np.uint64(S.LDS_SLOTS - 1)).size == 1
    cols = {0: _with_absent(rng, rng.integers(-10 ** 15, 10 ** 15, N_CARD).astype(np.int64), 0.05),
            1: _with_absent(rng, rng.standard_normal(N_CARD) * 1e3, 0.05), 2: by}
    live = np.ones(N_CARD, bool)
    eng = _engine(cols)
    try:
        sel = W.Program(np.array([(W.GT, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
        for attr in (0, 1):
            got = _check(eng, attr, 2, cols, live, distinct, tag=f"card_{card}_{attr}_tight")  # exactly max_groups groups
            assert got[0].size == distinct and got[7] == 0
            if card != "unique":  # (the model walks the groups one by one)
                _check(eng, attr, 2, cols, live, 65536, tag=f"card_{card}_{attr}")
                _check(eng, attr, 2, cols, live, 65536, sel, tag=f"card_{card}_{attr}_where")
            if distinct > 1:
                with pytest.raises(StatsOverflow) as err:
                    eng.attr_stats(attr, 2, distinct - 1)
                assert (err.value.matched, err.value.by_absent) == (N_CARD, 0) and err.value.n_groups > distinct - 1
        if distinct <= 65:
            _final_sums(_check(eng, 1, 2, cols, live, 128), cols, 1, 2, live)
    finally:
        eng.close()


def test_overflow_keeps_matched_and_by_absent_exact_and_the_limits_are_refused():
    rng = np.random.default_rng(3)
    n = 5000
    by = _with_absent(rng, rng.integers(0, 100, n).astype(np.int64))
    by[:100] = np.arange(100)
    tomb = rng.random(n) < 0.2
    tomb[:100] = False
    cols = {0: rng.integers(-5, 5, n).astype(np.int64), 1: rng.standard_normal(n), 2: by}
    eng = _engine(cols, n, tomb)
    try:
        want = S.stats_oracle(cols[0], by, ~tomb)
        assert want[0].size == 100 and want[7] > 0
        for attr in (0, 1):
            _check(eng, attr, 2, cols, ~tomb, 100, tag="overflow_exact")
            for max_groups in (99, 50, 1):
                with pytest.raises(StatsOverflow) as err:
                    eng.attr_stats(attr, 2, max_groups)
                assert (err.value.matched, err.value.by_absent) == want[6:] and err.value.n_groups > max_groups
            two = W.Program(np.array([(W.IN, 2, 0, 2)], W.OP_DTYPE), np.array([7, 8], np.int64))
            with pytest.raises(StatsOverflow) as err:
                eng.attr_stats(attr, 2, 1, where=two)
            assert err.value.matched == int((~tomb & np.isin(by, [7, 8])).sum()) == eng.where_count(two)
            assert err.value.by_absent == 0
        _check(eng, 0, 2, cols, ~tomb, S.MAX_VALUES, tag="overflow_largest")
        for bad in (S.MAX_VALUES + 1, 0, -1):
            with pytest.raises(RuntimeError, match=r"failed \(1\).*max_groups"):
                eng.attr_stats(0, 2, bad)
            with pytest.raises(RuntimeError, match=r"failed \(1\).*max_groups"):
                eng.attr_stats(0, None, bad)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*int64 column"):
            eng.attr_stats(0, 1, 10)  # a float64 by
        with pytest.raises(RuntimeError, match=r"failed \(1\).*not defined"):
            eng.attr_stats(5, None, 1)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*not defined"):
            eng.attr_stats(0, 5, 10)
        eng.define_attr(6, "int64_list")
        eng.define_attr(7, "geo")
        for bad in (6, 7):
            with pytest.raises(RuntimeError, match=r"failed \(1\)"):
                eng.attr_stats(bad, None, 1)
            with pytest.raises(RuntimeError, match=r"failed \(1\)"):
                eng.attr_stats(0, bad, 10)
    finally:
        eng.close()


# ---------------------------------------------------------------- integer sums
INT_PATTERNS = {
    "max": lambda n: np.full(n, INT64_MAX, np.int64),                                   # the high word, upwards
    "min": lambda n: np.full(n, INT64_MIN1, np.int64),                                  # ... and downwards
    "ones": lambda n: np.where(np.arange(n) % 2 == 0, -1, 1).astype(np.int64),          # the low word carries both ways
    "ends": lambda n: np.where(np.arange(n) % 2 == 0, INT64_MAX, INT64_MIN1).astype(np.int64),
}


@pytest.mark.parametrize("pattern", sorted(INT_PATTERNS))
def test_integer_sums_need_the_high_word_and_carry_both_ways(pattern):
    n = 40_000
    col = INT_PATTERNS[pattern](n)
    interleaved = (np.arange(n) // 2 % 64).astype(np.int64)  # 64 groups, each holding both halves of an alternation
    cols = {0: col, 1: np.zeros(n, np.int64), 2: interleaved}
    live = np.ones(n, bool)
    eng = _engine(cols)
    try:
        got = _check(eng, 0, None, cols, live, 1, tag=f"int_{pattern}")
        assert got[5] == [{"max": n * INT64_MAX, "min": n * INT64_MIN1, "ones": 0, "ends": 0}[pattern]]
        _check(eng, 0, 1, cols, live, 1, tag=f"int_{pattern}_one_group")
        grouped = _check(eng, 0, 2, cols, live, 64, tag=f"int_{pattern}_64_groups")
        assert grouped[0].size == 64 and sum(grouped[5]) == got[5][0]
        assert abs(got[5][0]) >= 2 ** 64 or pattern in ("ones", "ends")
    finally:
        eng.close()


# ---------------------------------------------------------------- float columns
def _float_cases():
    rng = np.random.default_rng(21)
    big = 2.0 ** 61
    tiny = 5e-324
    return {
        "inf_alone": [np.inf], "ninf_alone": [-np.inf, -np.inf], "both_inf": [np.inf, -np.inf, 1.0],
        "inf_and_finite": [1.5, np.inf, -2.0, 1e300], "ninf_and_finite": [-np.inf, 3.0],
        "zeros": [0.0, -0.0, 0.0, -0.0], "neg_zeros": [-0.0, -0.0], "zero_and_nan": [0.0, np.nan],
        "subnormals": (rng.integers(-2 ** 40, 2 ** 40, 3000) * tiny).tolist(), "least": [tiny], "two_least": [tiny, -tiny, tiny],
        "near_max": [1.7e308] * 1000, "near_min": [-1.7e308] * 999 + [1.0], "max_cancels": [1.7e308, -1.7e308] * 300 + [2.0 ** 970],
        "span_600": (rng.standard_normal(2000) * 2.0 ** rng.integers(-300, 300, 2000)).tolist(),
        "span_600_top": [2.0 ** 300] + (rng.standard_normal(500) * 2.0 ** rng.integers(-300, 239, 500)).tolist(),
        "halves": [big, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.75, 0.25, 3.5],
        "halves_only_ties": [big] + [0.5] * 101 + [1.5] * 101,
        "power_of_two": [1.0, 0.5, 2.0 ** -61, 2.0 ** -62, 2.0 ** -63, 3 * 2.0 ** -62],
        "below_power_of_two": [math.nextafter(1.0, 0.0), 2.0 ** -62, 2.0 ** -63, 3 * 2.0 ** -63],
        "least_normal": [2.0 ** -1022, math.nextafter(2.0 ** -1022, 0.0), tiny], "top_power": [2.0 ** 1023, 2.0 ** 1023],
        "cents": np.round(rng.uniform(0, 1000, 3000), 2).tolist(), "all_nan": [np.nan, np.nan],
    }


@pytest.mark.parametrize("case", sorted(_float_cases()))
def test_float_columns(case):
    values = np.array(_float_cases()[case], dtype=np.float64)
    rng = np.random.default_rng(len(case))
    # ungrouped over the values as they are; then nine groups that each hold all of them, interleaved, and a tenth, key
    # 9, holding one value only
    col = np.concatenate([np.tile(values, 9), values[:1]])
    by = np.concatenate([np.repeat(np.arange(9, dtype=np.int64), values.size), [9]])
    order = rng.permutation(col.size)
    col, by = col[order], by[order]
    for cols, group in (({0: values, 1: np.zeros(values.size, np.int64)}, None), ({0: col, 1: by}, 1)):
        live = np.ones(cols[0].size, bool)
        eng = _engine(cols)
        try:
            got = _check(eng, 0, group, cols, live, 16, tag=f"float_{case}_{group}")
            sums = _final_sums(got, cols, 0, group, live)
            assert got[0].size == (1 if group is None else 10)
            present = values[~np.isnan(values)]
            if case in ("near_max", "near_min"):
                assert abs(sums[0]) == np.inf and np.isfinite(got[3][0]) and np.isfinite(got[4][0])
            if case == "zeros":
                assert np.signbit(got[3][0]) and not np.signbit(got[4][0]) and sums[0] == 0.0
            if case == "both_inf":
                assert math.isnan(sums[0]) and got[5][0] == 0
            if case == "halves":
                assert got[5][0] - 2 ** 61 == 0 + 2 + 2 - 0 - 2 - 2 + 1 + 0 + 4
            if present.size and np.isfinite(present).all() and 0 < np.abs(present).max() / 512 <= np.abs(present).min() \
                    and np.abs(present).max() < 1e308 / present.size:
                assert sums[0] == math.fsum(present.tolist())  # every term exact: the correctly rounded sum
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
    for j in range(24):
        size = 64 if j < 2 or rng.random() < 0.15 else int(rng.integers(1, 24))
        programs.append(random_raw_program(rng, kinds, size, deep=(j == 0)))
    assert program_depth(programs[2]) == W.MAX_DEPTH and programs[2].ops.size == programs[3].ops.size == W.MAX_OPS
    try:
        matched = []
        for j, p in enumerate([None] + programs):
            got = _check(eng, 0, None, cols, ~tomb, 1, p, tag=f"prog_{j}_i")
            _check(eng, 1, None, cols, ~tomb, 1, p, tag=f"prog_{j}_f")
            _check(eng, 2, 0, cols, ~tomb, 64, p, tag=f"prog_{j}_i_by")
            _final_sums(_check(eng, 3, 2, cols, ~tomb, 64, p, tag=f"prog_{j}_f_by"), cols, 3, 2,
                        ~tomb if p is None else ~tomb & eval_program(p, cols, n))
            matched.append(got[6])
        assert matched[0] == matched[2] == int((~tomb).sum()) and matched[1] == 0
        assert any(0 < m < matched[0] for m in matched[3:])
        nothing = eng.attr_stats(1, None, 1, where=NOTHING)
        assert nothing[0].tolist() == [0] and nothing[1].tolist() == [0] and nothing[7:] == (0, 0)
        assert eng.attr_stats(1, 0, 4, where=NOTHING)[0].size == 0
    finally:
        eng.close()


# ---------------------------------------------------------------- Index and QueryProcessor
def test_index_and_query_processor_stats_equal_the_dict_semantics_through_updates():
    rng = np.random.default_rng(7)
    n = 3000
    index = Index(space="l2", attributes=SCHEMA)
    qp = QueryProcessor(InMemoryStorage(), index)
    try:
        vecs = [Vector(values=rng.standard_normal(4).astype(np.float32), metadata=m) for m in random_metadata(rng, n)]
        qp.upsert_many(vecs[:2000], "ns")
        qp.upsert_many(vecs[2000:], "ns")

        def check(filters):
            metas = [v.metadata for v in qp._storage.namespace_map["ns"]]
            for f in [None] + filters:
                for attr in ("price", "year", "in_stock"):
                    want = S.metadata_stats(metas, attr, f)
                    assert index.stats("ns", attr, f) == want, (attr, f)
                    assert qp.stats(attr, where=f, namespace="ns") == want
                    if f is not None:
                        assert want["matched"] == index.count("ns", f)
                        assert qp.stats(attr, where=lambda m: py_match(f, m), namespace="ns") == want
                    for by in ("genre", "in_stock", "year"):
                        want = S.metadata_stats(metas, attr, f, by)
                        got = index.stats("ns", attr, f, by=by)
                        assert got == want, (attr, by, f)
                        assert all(type(v) is {"genre": str, "year": int, "in_stock": bool}[by] for v, _ in got["groups"])
                        if f is not None:
                            assert qp.stats(attr, where=lambda m: py_match(f, m), namespace="ns", by=by) == want
            with pytest.raises(ValueError, match="max_groups=10"):
                index.stats("ns", "price", by="year", max_groups=10)

        check([random_filter(rng) for _ in range(6)])
        stored = list(qp._storage.namespace_map["ns"])
        qp.delete([v.id for v in stored[::9]], "ns")
        check([random_filter(rng) for _ in range(3)])
        stored = list(qp._storage.namespace_map["ns"])
        qp.update_metadata([v.id for v in stored[::5]], {"price": 1e300, "year": 2 ** 62, "genre": "dub"}, "ns")
        qp.update_metadata([v.id for v in stored[1::5]], {"price": None, "in_stock": True}, "ns")
        check([random_filter(rng) for _ in range(3)] + [{"genre": "dub"}])
        assert qp.update_where({"year": {"$lt": 1980}}, {"year": {"$inc": 100}, "price": -0.0}, "ns") > 0
        check([random_filter(rng) for _ in range(3)] + [{"year": {"$gte": 2050}}])
        total = index.stats("ns", "year")
        assert type(total["sum"]) is int and total["sum"] > 2 ** 64 and total["max"] == 2 ** 62
    finally:
        index.close()
