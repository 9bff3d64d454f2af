"""Attribute updates and deletes by filter on the MI355X (include/mlvdb_mutate.h): the update kernel against the NumPy model
on hostile column values, the scatter by label, ``tombstone_where`` against a twin index that takes the composition
``tombstone(where_labels(p))``, and the ``Index`` histories of tests/test_mutate_host.py on ``HipScanEngine``.  Every
comparison is exact: counts, labels, the columns' bit patterns, the distances of twin searches."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import Index, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.conftest import dump_mismatch
from tests.mutate_helpers import INT64_MAX, MutateOracleEngine, bits, replay_history
from tests.where_helpers import FLOAT_POOL, INT_POOL, SCHEMA, hostile_columns, random_raw_program

pytestmark = pytest.mark.gpu

ASSIGN, ADD = _native.SET_ASSIGN, _native.SET_ADD
KINDS = {0: "int64", 1: "float64", 5: "int64", 9: "float64"}
NAN_BITS = W.float_bits(float("nan"))


def fbits(x) -> int:
    return W.float_bits(x)


def prog(*ops) -> W.Program:
    return W.Program(np.array(list(ops), dtype=W.OP_DTYPE), np.zeros(0, np.int64))


def _pair(rng, n, d=3):
    """A HIP engine and the NumPy model holding the same rows, hostile columns and ~10 % tombstones."""
    rows = rng.standard_normal((n, d), dtype=np.float32)
    cols = hostile_columns(rng, n, KINDS)
    tomb = np.flatnonzero(rng.random(n) < 0.1)
    out = []
    for e in (HipScanEngine(d, "l2", device=0), MutateOracleEngine(d, "l2")):
        e.append(rows)
        for a, kind in KINDS.items():
            e.define_attr(a, kind)
            e.set_attr(a, 0, cols[a].copy())
        e.tombstone(tomb)
        out.append(e)
    return out[0], out[1], n


def _same_columns(eng, model, n, tag):
    for a, kind in KINDS.items():
        got = eng.get_attr(a, 0, n, np.float64 if kind == "float64" else np.int64)
        want = model.get_attr(a, 0, n, got.dtype)
        if not np.array_equal(bits(got), bits(want)):
            bad = np.flatnonzero(bits(got) != bits(want))
            dump_mismatch(f"mutate_{tag}".replace(" ", "_"), rows=bad[:4096], got=bits(got)[bad[:4096]], want=bits(want)[bad[:4096]])
            pytest.fail(f"{tag}: column {a} differs from the model at {bad.size} rows, first {bad[0]}: "
                        f"{bits(got)[bad[0]]:#x} vs {bits(want)[bad[0]]:#x}")


# ---------------------------------------------------------------- (a) the update kernel against the model
# 1,048,577 rows: one past a single stride of the kernels' capped grid (4096 blocks x 256 threads, where_eval_kernel's cap)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097, 1_048_577])
def test_update_where_chain_equals_the_model(n):
    rng = np.random.default_rng(7100 + n % 1000)
    eng, model, _ = _pair(rng, n)
    rand = lambda size=None: random_raw_program(rng, KINDS, int(size or rng.integers(1, 24)))  # noqa: E731
    steps = [
        # assignments, both sentinels and both column types; every live row, then random programs
        ("clear int", rand(), [(0, ASSIGN, int(W.INT64_ABSENT))]),
        ("clear float", rand(), [(1, ASSIGN, NAN_BITS)]),
        ("assign int", rand(64), [(5, ASSIGN, 3)]),
        ("assign float", rand(), [(9, ASSIGN, fbits(-0.0))]),
        ("assign payload", rand(), [(9, ASSIGN, int(FLOAT_POOL[2:3].view(np.int64)[0]))]),
        # the predicate reads the column it assigns: each row sees the value from before the call, and the second call
        # finds nothing left
        ("ge int", prog((W.GE, 5, 2000, 0)), [(5, ASSIGN, 1999)]),
        ("ge int again", prog((W.GE, 5, 2000, 0)), [(5, ASSIGN, 1999)]),
        ("lt float", prog((W.LT, 9, fbits(0.0), 0)), [(9, ASSIGN, fbits(5.0))]),
        ("lt float again", prog((W.LT, 9, fbits(0.0), 0)), [(9, ASSIGN, fbits(5.0))]),
        ("exists clears", prog((W.EXISTS, 1, 0, 0)), [(1, ASSIGN, NAN_BITS), (0, ASSIGN, 2)]),
        # several columns in one call, the program over the same columns
        ("four columns", rand(), [(0, ASSIGN, 7), (1, ASSIGN, fbits(1.5)), (9, ADD, fbits(1.0)), (5, ADD, 1)]),
        # increments by one: the hostile values next to the ends of int64 are refused or land on the ends
        ("inc int", prog((W.LT, 5, INT64_MAX - 1, 0)), [(5, ADD, 1)]),
        ("inc int all", prog((W.TRUE, 0, 0, 0)), [(5, ADD, 1)]),
        ("dec int", rand(), [(0, ADD, -1)]),
        ("dec int all", prog((W.TRUE, 0, 0, 0)), [(5, ADD, -1)]),
        ("inc float", rand(), [(9, ADD, fbits(1.0))]),
        ("dec float", prog((W.TRUE, 0, 0, 0)), [(1, ADD, fbits(-1.0)), (9, ADD, fbits(-1.0))]),
        # amounts that overflow for some hostile values: all or nothing
        ("add max", prog((W.TRUE, 0, 0, 0)), [(5, ADD, INT64_MAX), (9, ASSIGN, fbits(2.0))]),
        ("add -max", prog((W.TRUE, 0, 0, 0)), [(5, ADD, -INT64_MAX), (0, ASSIGN, 1)]),
        ("add max to the small", prog((W.LE, 5, 0, 0)), [(5, ADD, INT64_MAX)]),
        ("add dbl max", rand(), [(9, ADD, fbits(np.finfo(np.float64).max))]),
        ("add inf", prog((W.GT, 9, fbits(0.0), 0)), [(9, ADD, fbits(np.inf))]),
        ("add -inf", prog((W.TRUE, 0, 0, 0)), [(9, ADD, fbits(-np.inf)), (5, ASSIGN, 0)]),
        ("add -inf to the finite", prog((W.LT, 9, fbits(np.inf), 0)), [(9, ADD, fbits(-np.inf))]),
    ]
    hostile = [("inc hostile", prog((W.TRUE, 0, 0, 0)), [(0, ADD, 1)]), ("dec hostile", rand(), [(5, ADD, -1)]),
               ("dec hostile all", prog((W.TRUE, 0, 0, 0)), [(5, ADD, -2), (0, ADD, 2)]),
               ("inc hostile some", prog((W.LT, 0, INT64_MAX - 1, 0)), [(0, ADD, 2), (5, ASSIGN, int(W.INT64_ABSENT))])]
    seen = set()

    def run(chain):
        for tag, p, sets in chain:
            got, want = eng.update_where(p, sets), model.update_where(p, sets)
            print(f"n={n} {tag}: (matched, refused) = {got}, model {want}")
            assert got == want, f"n={n} {tag}"
            _same_columns(eng, model, n, f"n={n} {tag}")
            seen.add((got[0] > 0, got[1] > 0))
            if tag.endswith("again"):
                assert got == (0, 0), tag

    try:
        run(steps)
        for a in (0, 5):  # hostile values again under the increments: the chain above has flattened the columns
            fresh = rng.choice(INT_POOL, n)
            eng.set_attr(a, 0, fresh)
            model.set_attr(a, 0, fresh.copy())
        run(hostile)
        if n >= 257:  # the chain met both outcomes: rows updated, and a call refused as a whole
            assert {(True, False), (True, True)} <= seen, seen
    finally:
        eng.close()


def test_update_where_refusals():
    rng = np.random.default_rng(1)
    eng, model, n = _pair(rng, 65)
    true = prog((W.TRUE, 0, 0, 0))
    try:
        for sets in ([], [(0, ASSIGN, 1)] * 2, [(2, ASSIGN, 1)], [(16, ASSIGN, 1)], [(-1, ASSIGN, 1)], [(0, 2, 1)],
                     [(1, ADD, NAN_BITS)], [(a, ASSIGN, 0) for a in range(17)]):
            with pytest.raises(RuntimeError, match=r"\(1\)"):
                eng.update_where(true, sets)
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            eng.update_where(prog((W.AND, 0, 0, 0)), [(0, ASSIGN, 1)])
        _same_columns(eng, model, n, "refusals")
    finally:
        eng.close()


# ---------------------------------------------------------------- (b) values by label
def test_set_attr_at_equals_the_model():
    rng = np.random.default_rng(7200)
    eng, model, n = _pair(rng, 700)
    try:
        for m in (1, 64, 65, 257, n):
            for a, kind in KINDS.items():
                labels = rng.permutation(n)[:m].astype(np.int64)  # random order, tombstoned labels among them
                values = rng.choice(INT_POOL if kind == "int64" else FLOAT_POOL, m)
                got, want = eng.set_attr_at(a, labels, values), model.set_attr_at(a, labels, values)
                print(f"set_attr_at m={m} attr={a}: updated {got}, model {want}")
                assert got == want, (m, a)
                _same_columns(eng, model, n, f"set_attr_at m={m} attr={a}")
        assert eng.set_attr_at(0, np.zeros(0, np.int64), np.zeros(0, np.int64)) == 0
        for labels in ([3, 9, 3], [0, n], [-1, 4], [n + 5], list(range(300)) + [299]):
            with pytest.raises(RuntimeError, match=r"\(1\)"):
                eng.set_attr_at(0, np.array(labels, np.int64), np.ones(len(labels), np.int64))
        with pytest.raises(RuntimeError, match=r"\(1\)"):
            eng.set_attr_at(2, np.array([1], np.int64), np.ones(1, np.int64))  # not defined
        _same_columns(eng, model, n, "set_attr_at refusals")
    finally:
        eng.close()


# ---------------------------------------------------------------- (c) tombstone_where against a twin
def _raw_tombstone_where(eng, program, capacity):
    """The C entry itself: (status, matches, labels or None); capacity < 0: the no-labels form."""
    w, keep = eng._where(program)
    out = np.full(max(capacity, 1), -7, dtype=np.int64)
    n = C.c_int64(-1)
    rc = eng._lib.mlvdb_tombstone_where(eng.handle, C.byref(w), out.ctypes.data if capacity >= 0 else None, capacity,
                                        C.byref(n))
    return rc, int(n.value), (out[:min(capacity, n.value)] if capacity >= 0 else None)


@pytest.mark.parametrize("space", ["cosine", "l2", "ip"])
def test_tombstone_where_leaves_the_state_of_tombstone(space):
    rng = np.random.default_rng(7300)
    n, d = 8229, 128
    rows = rng.standard_normal((n, d), dtype=np.float32)
    extra = rng.standard_normal((300, d), dtype=np.float32)
    tenant = rng.integers(0, 12, n + 300).astype(np.int64)
    qs = rng.standard_normal((8, d), dtype=np.float32)
    radius = float(np.sort(exact_scan.exact_distances(qs[:2], rows, space), axis=1)[:, 40].mean())
    a, b = (HipScanEngine(d, space, device=0, strategy="filter") for _ in range(2))
    for e in (a, b):
        e.append(rows)
        e.define_attr(0, "int64")
        e.set_attr(0, 0, tenant[:n])
    host = {"rows": rows, "tenant": tenant[:n].copy(), "dead": np.zeros(n, bool)}
    true = prog((W.TRUE, 0, 0, 0))

    def same(tag):
        assert a.counts() == b.counts() == (host["dead"].size, int(host["dead"].sum())), tag
        assert a.where_count(true) == b.where_count(true) == int((~host["dead"]).sum()), tag
        for nq in (1, 8):
            la, da, ca = a.search(qs[:nq], 10)
            lb, db, cb = b.search(qs[:nq], 10)
            assert np.array_equal(la, lb) and np.array_equal(da.view(np.int32), db.view(np.int32)) and np.array_equal(ca, cb), (tag, nq)
            ol, _, oc = exact_scan.knn(qs[:nq], host["rows"], 10, space, deleted=host["dead"])
            assert np.array_equal(la, ol) and np.array_equal(ca, oc), (tag, nq, "oracle")
        ra, rb = a.range(qs[:2], radius, 1024), b.range(qs[:2], radius, 1024)
        for (l1, d1), (l2, d2) in zip(ra, rb):
            assert np.array_equal(l1, l2) and np.array_equal(d1.view(np.int32), d2.view(np.int32)), (tag, "range")

    def both(tag, p):
        want = np.flatnonzero(~host["dead"] & np.isin(host["tenant"], p.set if p.set.size else [int(p.ops["a"][0])]))
        got = a.tombstone_where(p)
        assert b.tombstone(b.where_labels(p)) == want.size, tag
        print(f"{space} {tag}: {got.size} rows")
        assert np.array_equal(got, want) and want.size > 0, tag
        host["dead"][want] = True
        same(tag)

    try:
        both("no shadow yet", prog((W.EQ, 0, 3, 0)))                       # 1. before any search
        both("shadow built", W.Program(np.array([(W.IN, 0, 0, 2)], dtype=W.OP_DTYPE), np.array([5, 7], np.int64)))  # 2. after warm searches
        for e in (a, b):                                                   # 3. rows the shadow does not hold yet
            assert e.append(extra) == n
            e.set_attr(0, n, tenant[n:])
        host = {"rows": np.concatenate([rows, extra]), "tenant": tenant.copy(), "dead": np.concatenate([host["dead"], np.zeros(300, bool)])}
        assert (tenant[:n] == 9).any() and (tenant[n:] == 9).any()
        both("appended, not searched", prog((W.EQ, 0, 9, 0)))
        # a buffer one short: nothing happens, the count is exact
        p = prog((W.EQ, 0, 1, 0))
        matches = a.where_count(p)
        before = a.search(qs, 10)
        rc, m, _ = _raw_tombstone_where(a, p, matches - 1)
        assert (rc, m) == (0, matches) and matches > 1
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(before, a.search(qs, 10)))
        same("short buffer")
        # no labels wanted: tombstone and count only
        rc, m, _ = _raw_tombstone_where(a, p, -1)
        assert (rc, m) == (0, matches) and b.tombstone(b.where_labels(p)) == matches
        host["dead"][np.flatnonzero(~host["dead"] & (host["tenant"] == 1))] = True
        same("no labels")
        assert _raw_tombstone_where(a, p, -1)[:2] == (0, 0) and _raw_tombstone_where(a, p, 0)[:2] == (0, 0)
        same("nothing left")
        oa, ob = a.compact(), b.compact()
        assert np.array_equal(oa, ob) and np.array_equal(oa, np.flatnonzero(~host["dead"]))
        host = {"rows": host["rows"][oa], "tenant": host["tenant"][oa], "dead": np.zeros(oa.size, bool)}
        same("compacted")
        both("after compaction", prog((W.EQ, 0, 11, 0)))
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- (d) Index histories on the HIP engine
@pytest.mark.parametrize("seed,space", [(2, "cosine"), (6, "l2")])
def test_index_histories_on_the_hip_engine(seed, space):
    index = Index(space=space, attributes=SCHEMA)
    try:
        ran = replay_history(index, space, seed, n_rows=600, d=16)
        print(f"history {seed} {space}: {ran}")
        assert sum(v for k, v in ran.items() if k != "refused") == 40
    finally:
        index.close()
