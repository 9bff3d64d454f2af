"""Ordered metadata queries on the MI355X (include/mlvdb_order.h) against NumPy: np.lexsort over the live matching rows
(tests/order_helpers.py).  Every comparison is exact equality: of labels, of the values' bit patterns, of matched / absent;
every call is made twice and must agree.  Rows are 4 floats wide, so the row store is negligible; the shapes are the smallest
at which each mechanism can go wrong: wave and block edges, one size past a whole pass of the grid, more candidates than one
block ranks (so that the digit passes must select), ties that only label digits decide, ranks on bucket edges."""
import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from mlvectordb_amd.vector import Vector
from tests import facet_helpers as F
from tests import order_helpers as O
from tests.conftest import dump_mismatch
from tests.where_helpers import SCHEMA, eval_program, py_match, random_filter, random_metadata

pytestmark = pytest.mark.gpu

NOTHING = W.Program(np.array([(W.TRUE, 0, 0, 0), (W.NOT, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
EVERYTHING = W.Program(np.array([(W.TRUE, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
WINDOWS = ((0, 1), (0, 20), (4076, 20), (0, 4096))
INT64_MIN, INT64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


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


def _check(eng, attr, col, live, windows=WINDOWS, directions=(False, True), program=None, cols=None, tag="order"):
    """where_ordered twice per window and direction against the oracle: the ranking is computed once per direction (every
    window lies inside its first 4096 ranks); matched against where_count of the same program."""
    mask = live if program is None else live & eval_program(program, cols, col.size)
    count = None if program is None else eng.where_count(program)
    out = {}
    for descending in directions:
        top, _, matched, absent = O.ordered_oracle(col, mask, descending, 0, O.MAX_ROWS)
        for offset, limit in windows:
            want = top[offset:offset + limit]
            name = f"{tag}_{'desc' if descending else 'asc'}_{offset}_{limit}"
            got = eng.where_ordered(attr, limit, where=program, descending=descending, offset=offset)
            again = eng.where_ordered(attr, limit, where=program, descending=descending, offset=offset)
            ok = np.array_equal(got[0], want) and got[2:] == (matched, absent) and \
                np.array_equal(got[1].view(np.int64), col[want].view(np.int64))
            if not ok:
                dump_mismatch(name, got_labels=got[0], got_values=got[1], want_labels=want, want_values=col[want],
                              scalars=np.array(got[2:] + (matched, absent)))
            assert got[2:] == (matched, absent), f"{name}: (matched, absent) {got[2:]}, NumPy {(matched, absent)}"
            assert got[0].dtype == np.int64 and got[1].dtype == col.dtype
            assert got[0].size == want.size == max(0, min(matched - absent - offset, limit)), f"{name}: n_out {got[0].size}"
            assert np.array_equal(got[0], want), f"{name}: labels differ at {np.flatnonzero(got[0] != want)[:8]}"
            assert np.array_equal(got[1].view(np.int64), col[want].view(np.int64)), f"{name}: value bits differ"
            assert np.array_equal(got[0], again[0]) and got[2:] == again[2:] and \
                np.array_equal(got[1].view(np.int64), again[1].view(np.int64)), f"{name}: two calls"
            if count is not None:
                assert got[2] == count, f"{name}: matched != where_count"
            out[(descending, offset, limit)] = got
    return out


# ---------------------------------------------------------------- row counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 40_000, F.GRID_ROWS + 300])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    ints = rng.integers(-2000, 2000, n).astype(np.int64)
    ints[rng.random(n) < 0.1] = F.ABSENT
    floats = rng.integers(-2000, 2000, n).astype(np.float64) / 8
    floats[rng.random(n) < 0.1] = np.nan
    tomb = rng.random(n) < 0.1
    eng = _engine({0: ints, 1: floats}, n, tomb)
    try:
        got = _check(eng, 0, ints, ~tomb, tag=f"rows_{n}_i")
        _check(eng, 1, floats, ~tomb, tag=f"rows_{n}_f")
        if n == 0:
            assert all(g[0].size == 0 and g[2:] == (0, 0) for g in got.values())
        else:
            sel = W.Program(np.array([(W.GE, 0, 2, 0)], W.OP_DTYPE), np.zeros(0, np.int64))
            _check(eng, 1, floats, ~tomb, ((0, 20), (4076, 20)), program=sel, cols={0: ints, 1: floats}, tag=f"rows_{n}_where")
    finally:
        eng.close()


# ---------------------------------------------------------------- ties
def test_an_all_equal_column_is_decided_by_label_digits_above_bit_16():
    n = 70_000
    col = np.full(n, 1999, np.int64)
    tomb = np.zeros(n, bool)
    tomb[[0, 5, 4095, 4096, 65_536]] = True
    eng = _engine({0: col, 1: np.full(n, -0.0)}, n, tomb)
    try:
        got = _check(eng, 0, col, ~tomb, tag="all_equal")
        assert got[(True, 0, 4096)][0].tolist() == np.flatnonzero(~tomb)[:4096].tolist()  # descending: labels still ascend
        _check(eng, 1, np.full(n, -0.0), ~tomb, tag="all_equal_f")
        # every live row below label 65,000 tombstoned: the window starts just under 2^16 and ends beyond it (masked route)
        tail = np.ones(n, bool)
        tail[:65_000] = False
        eng.tombstone(np.flatnonzero(~tail & ~tomb))
        got = _check(eng, 0, col, tail & ~tomb, program=EVERYTHING, cols={0: col}, tag="all_equal_high")
        assert got[(False, 0, 4096)][0][0] == 65_000 and got[(False, 0, 4096)][0][-1] > 65_536
    finally:
        eng.close()


def test_a_bool_like_column():
    rng = np.random.default_rng(11)
    n = 40_000
    col = (rng.random(n) < 0.5).astype(np.int64)
    col[rng.random(n) < 0.1] = F.ABSENT
    eng = _engine({0: col})
    try:
        _check(eng, 0, col, np.ones(n, bool), WINDOWS + ((4000, 96),), tag="bool")
    finally:
        eng.close()


@pytest.mark.parametrize("values", [256, 1024])
def test_ranks_on_and_beside_bucket_edges(values):
    """Every value held by 16 rows in shuffled label order: offset + limit a multiple of 16 puts the N-th rank on the last row of
    a value, one more on the first row of the next.  256 values are the 4096 rows one block ranks; 1024 values are more, so the
    digit passes must select the bucket."""
    rng = np.random.default_rng(values)
    col = rng.permutation(np.repeat(np.arange(values, dtype=np.int64), 16))
    fcol = col.astype(np.float64) - values / 2
    windows = ((0, 16), (16, 16), (0, 4096), (4080, 16), (0, 17), (0, 15), (15, 17), (4079, 16), (4079, 17), (2032, 31),
               (2032, 32), (2032, 33))
    eng = _engine({0: col, 1: fcol})
    try:
        got = _check(eng, 0, col, np.ones(col.size, bool), windows, tag=f"edges_{values}")
        assert sorted(got[(False, 0, 16)][1].tolist()) == [0] * 16 and got[(True, 0, 17)][1].tolist() == [values - 1] * 16 + [values - 2]
        for g in got.values():  # ties by ascending label in both directions
            same = g[1][1:] == g[1][:-1]
            assert (g[0][1:][same] > g[0][:-1][same]).all()
        _check(eng, 1, fcol, np.ones(col.size, bool), windows, tag=f"edges_{values}_f")
    finally:
        eng.close()


# ---------------------------------------------------------------- key transform
INT_VALUES = np.array([INT64_MIN + 1, INT64_MIN + 2, -1, 0, 1, INT64_MAX, INT64_MAX - 1, 0x1200, 0x1201, -0x1200, -0x1201,
                       0x12 << 56, 0x13 << 56, -(0x12 << 56), -(0x13 << 56)], np.int64)
F_MAX, F_DEN = np.finfo(np.float64).max, 5e-324
FLOAT_VALUES = np.array([-np.inf, -F_MAX, -F_DEN, -0.0, 0.0, F_DEN, F_MAX, np.inf, 1.5, -1.5, np.nextafter(1.5, 2)])


@pytest.mark.parametrize("n", [3000, 20_000])
def test_key_transform_at_the_ends_of_both_types(n):
    """3000 rows are ranked by one block; 20,000 rows of so few values send the selection through every key digit."""
    rng = np.random.default_rng(n)
    ints = rng.choice(np.concatenate([INT_VALUES, [F.ABSENT]]), n)
    floats = rng.choice(np.concatenate([FLOAT_VALUES, [np.nan, -np.nan]]), n)
    ints[:INT_VALUES.size], floats[:FLOAT_VALUES.size] = INT_VALUES, FLOAT_VALUES
    live = np.ones(n, bool)
    eng = _engine({0: ints, 1: floats})
    try:
        got = _check(eng, 0, ints, live, WINDOWS + ((n // 15, 40), (4096 - 64, 64)), tag=f"keys_{n}_i")
        assert got[(False, 0, 1)][1][0] == INT64_MIN + 1 and got[(True, 0, 1)][1][0] == INT64_MAX
        assert got[(False, 0, 20)][3] == int((ints == F.ABSENT).sum()) > 0
        got = _check(eng, 1, floats, live, WINDOWS + ((n // 11, 40), (4096 - 64, 64)), tag=f"keys_{n}_f")
        assert got[(False, 0, 1)][1][0] == -np.inf and got[(True, 0, 1)][1][0] == np.inf
        assert got[(False, 0, 20)][3] == int(np.isnan(floats).sum()) > 0  # NaN rows are absent
    finally:
        eng.close()


def test_signed_zeros_tie_and_come_back_bit_for_bit():
    n = 10_000
    col = np.where(np.arange(n) % 2 == 0, -0.0, 0.0)  # interleaved by label
    col[::7] = np.where(np.arange(0, n, 7) % 3 == 0, -1.0, 1.0)
    eng = _engine({0: col})
    try:
        got = _check(eng, 0, col, np.ones(n, bool), tag="zeros")
        asc = got[(False, 0, 4096)]
        zeros = asc[1] == 0.0
        assert zeros.any() and np.signbit(asc[1][zeros]).any() and not np.signbit(asc[1][zeros]).all()
        assert (np.diff(asc[0][zeros]) > 0).all()  # the zeros of both signs in label order: they tie
    finally:
        eng.close()


# ---------------------------------------------------------------- all distinct
def test_all_distinct_values():
    rng = np.random.default_rng(13)
    n = 40_000
    col = rng.permutation(n).astype(np.int64)
    fcol = (col - n // 2) * 0.25
    # (0, 20) lies inside the first non-empty digit bucket (512 values), (500, 30) and (4076, 20) cross buckets
    windows = WINDOWS + ((500, 30), (511, 2), (512, 1), (3584, 512))
    eng = _engine({0: col, 1: fcol})
    try:
        got = _check(eng, 0, col, np.ones(n, bool), windows, tag="distinct")
        assert got[(False, 500, 30)][1].tolist() == list(range(500, 530))
        assert got[(True, 0, 20)][1].tolist() == list(range(n - 1, n - 21, -1))
        _check(eng, 1, fcol, np.ones(n, bool), windows, tag="distinct_f")
    finally:
        eng.close()


# ---------------------------------------------------------------- windows and refusals
def test_windows_beyond_the_candidates_and_refusals():
    rng = np.random.default_rng(17)
    n = 300
    col = rng.integers(0, 50, n).astype(np.int64)
    col[rng.random(n) < 0.2] = F.ABSENT
    live = np.ones(n, bool)
    candidates = int((col != F.ABSENT).sum())
    eng = _engine({0: col, 1: np.full(n, np.nan)})
    try:
        windows = ((candidates, 5), (candidates + 1, 5), (4095, 1), (candidates - 3, 20), (candidates - 1, 1), (0, 4096),
                   (4000, 96))
        got = _check(eng, 0, col, live, windows, tag="windows")
        assert got[(False, candidates, 5)][0].size == 0 and got[(False, candidates - 3, 20)][0].size == 3
        assert got[(False, 0, 4096)][0].size == candidates
        # no candidates: every value absent, a program that matches nothing, every row tombstoned
        got = _check(eng, 1, np.full(n, np.nan), live, tag="all_absent")
        assert all(g[0].size == 0 and g[2:] == (n, n) for g in got.values())
        got = _check(eng, 0, col, live, program=NOTHING, cols={0: col}, tag="nothing")
        assert all(g[0].size == 0 and g[2:] == (0, 0) for g in got.values())
        good = eng.where_ordered(0, 20)
        for kw in ({"limit": 4097}, {"limit": 1, "offset": 4096}, {"limit": 20, "offset": 4077}, {"limit": 0}, {"limit": -1},
                   {"limit": 5, "offset": -1}):
            with pytest.raises(RuntimeError, match=r"where_ordered failed \(1\).*offset \+ limit"):
                eng.where_ordered(0, **kw)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*not defined"):
            eng.where_ordered(5, 20)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*out of range"):
            eng.where_ordered(-1, 20)
        malformed = [W.Program(np.array([(W.AND, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64)),         # empty stack
                     W.Program(np.array([(W.TRUE, 0, 0, 0)] * 2, W.OP_DTYPE), np.zeros(0, np.int64)),     # two values left
                     W.Program(np.array([(W.EQ, 7, 1, 0)], W.OP_DTYPE), np.zeros(0, np.int64)),           # undefined column
                     W.Program(np.array([(99, 0, 0, 0)], W.OP_DTYPE), np.zeros(0, np.int64))]             # unknown op
        for p in malformed:
            with pytest.raises(RuntimeError, match=r"where_ordered failed \(1\)"):
                eng.where_ordered(0, 20, where=p)
            again = eng.where_ordered(0, 20)  # a valid call on the same handle after a refusal
            assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1]) and again[2:] == good[2:]
        _check(eng, 0, col, live, ((0, 20),), program=EVERYTHING, cols={0: col}, tag="after_refusals")
        eng.tombstone(np.arange(n))
        got = _check(eng, 0, col, np.zeros(n, bool), tag="all_tombstoned")
        assert all(g[0].size == 0 and g[2:] == (0, 0) for g in got.values())
    finally:
        eng.close()


# ---------------------------------------------------------------- filters and liveness
def _schema_columns(rng, n):
    metas = random_metadata(rng, n)
    strings = {}
    cols = {i: W.encode_column(name, kind, [m.get(name) for m in metas], strings.setdefault(name, {}))
            for i, (name, kind) in enumerate(SCHEMA.items())}
    return cols, strings


def test_random_filters_tombstones_compaction_and_regrowth():
    rng = np.random.default_rng(19)
    n = 12_000  # more candidates than one block ranks, so filtered calls select too
    cols, strings = _schema_columns(rng, n)
    programs = [EVERYTHING, NOTHING] + [W.compile_where(random_filter(rng), SCHEMA, strings) for _ in range(40)]
    tomb = rng.random(n) < 0.3
    eng = _engine(cols, n, tomb)
    by = (1, 2, 3)  # year, price, in_stock

    def sweep(cols, live, tag):
        matched = []
        for j, p in enumerate(programs):
            attr = by[j % 3]
            got = _check(eng, attr, cols[attr], live, (WINDOWS[j % 4], (j * 97 % 4000, 50)), (j % 2 == 1,), p, cols,
                         tag=f"{tag}_{j}")
            matched.append(next(iter(got.values()))[2])
        assert matched[0] == int(live.sum()) and matched[1] == 0 and any(0 < m < matched[0] for m in matched[2:])
        _check(eng, 1, cols[1], live, tag=f"{tag}_plain")

    try:
        sweep(cols, ~tomb, "filters")
        old = eng.compact()  # labels are renumbered
        assert np.array_equal(old, np.flatnonzero(~tomb))
        cols = {a: c[old] for a, c in cols.items()}
        sweep(cols, np.ones(old.size, bool), "compacted")
        # an append that regrows the capacity: the new rows hold no value until one column is set
        total, _ = eng.counts()
        more = 3 * total
        eng.append(np.ones((more, 4), dtype=np.float32))
        assert eng.counts()[0] == total + more
        cols = {a: np.concatenate([c, np.full(more, np.nan if c.dtype == np.float64 else F.ABSENT, c.dtype)])
                for a, c in cols.items()}
        cols[1][total:] = rng.integers(1940, 2030, more)
        eng.set_attr(1, total, cols[1][total:])
        sweep(cols, np.ones(total + more, bool), "regrown")
    finally:
        eng.close()


# ---------------------------------------------------------------- Index and QueryProcessor
def _want_top(live, by, where, descending, offset, limit):
    rows = [v for v in live if where is None or py_match(where, v.metadata)]
    have = [v for v in rows if v.metadata.get(by) is not None and v.metadata[by] == v.metadata[by]]
    ranked = sorted(have, key=lambda v: v.metadata[by], reverse=descending)[offset:offset + limit]  # stable: insertion order
    return {"ids": [v.id for v in ranked], "values": [v.metadata[by] for v in ranked], "matched": len(rows),
            "absent": len(rows) - len(have)}


def test_index_and_query_processor_top_by_equal_a_python_sort():
    rng = np.random.default_rng(23)
    n = 600
    index = Index(space="l2", attributes=SCHEMA)
    qp = QueryProcessor(InMemoryStorage(), index)
    try:
        vecs = [Vector(values=rng.standard_normal(4).astype(np.float32), metadata=m) for m in random_metadata(rng, n)]
        qp.upsert_many(vecs[:400], "ns")
        qp.upsert_many(vecs[400:], "ns")
        vecs = list(qp._storage.namespace_map["ns"])  # the stored vectors carry the ids minted at upsert
        gone = {v.id for v in vecs[::9]}
        qp.delete(list(gone), "ns")
        live = [v for v in vecs if v.id not in gone]
        kinds = {"year": int, "price": float, "in_stock": bool}
        for j, f in enumerate([None] + [random_filter(rng) for _ in range(12)]):
            for by in kinds:
                descending, (offset, limit) = j % 2 == 1, ((0, 20), (7, 5), (0, 4096))[j % 3]
                want = _want_top(live, by, f, descending, offset, limit)
                got = index.top_by("ns", by, limit, f, descending=descending, offset=offset)
                assert got == want, (by, f, descending, offset, limit)
                assert all(type(v) is kinds[by] for v in got["values"])
                assert qp.top_by(by, limit, f, "ns", descending=descending, offset=offset) == want
                if f is not None:
                    assert got["matched"] == index.count("ns", f)
                    assert index.query_by_metadata("ns", f, order_by=by, descending=descending, limit=limit, offset=offset) == \
                        want["ids"]
                    assert qp.top_by(by, limit, lambda m: py_match(f, m), "ns", descending=descending, offset=offset) == want
                    assert index.query_by_metadata("ns", f) == [v.id for v in live if py_match(f, v.metadata)]
        with pytest.raises(ValueError, match="str column"):
            index.top_by("ns", "genre", 5)
    finally:
        index.close()
