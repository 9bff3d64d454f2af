"""The seeded call histories of tests/history_helpers.py without a GPU: they are deterministic, the model agrees with the oracle
engines it is composed from, the committed seed set meets every coverage condition (printed with the seed and step that meets
it), the driver reports three seeded stale-state defects, and near-tie redraws stay under 1 % of the drawn queries."""
import json

import numpy as np
import pytest

from mlvectordb_amd import where as W
from tests import history_helpers as H
from tests.distinct_helpers import DistinctOracleEngine
from tests.facet_helpers import FacetOracleEngine
from tests.where_helpers import EachOracleEngine, EachRangeOracleEngine

SEARCHES = ("search", "search64")
HALF = [[W.LT, 2, 8, 0]]


def trace(ops, expected, space):
    """The handle's state BEFORE each step, from the ops and the counts the model reported: enough to name routes."""
    st = dict(strategy="auto", total=0, deleted=0, space=space, cap=0, gather=150, oversample=4, regrowths=0, valued=False)
    out = []
    for op, exp in zip(ops, expected):
        out.append(dict(st))
        kind = op["op"]
        if kind == "set_strategy":
            st["strategy"] = op["strategy"]
        elif kind == "set_tuning":
            st["gather" if op["key"] == "WHERE_GATHER" else "oversample"] = op["value"]
        elif kind == "append":
            cap = H.capacity_after(st["cap"], st["total"] + op["n"])
            if cap != st["cap"] and st["cap"] and st["valued"]:
                st["regrowths"] += 1
            st["cap"] = cap
        elif kind == "compact":
            st["cap"] = H.capacity_after_compact(st["cap"], st["total"] - st["deleted"], st["deleted"])
        elif kind == "set_attr" and op["n"]:
            st["valued"] = True
        elif kind == "reset":
            st.update(regrowths=0, valued=False)
            st["space"] = op["space"] or st["space"]
        if "counts" in exp:
            st["total"], st["deleted"] = exp["counts"]
    return out


def filter_route(op, st):
    return op["op"] in SEARCHES and (st["strategy"] == "filter" or (
        st["strategy"] == "auto" and st["total"] >= H.FILTER_MIN_ROWS and op["nq"] >= 12))


def masked(op, st):
    if op["op"] in ("search_mask", "search_where"):
        return op["op"]
    if op["op"] == "search_each" and st["gather"] != 1 << 30 and (st["gather"] == 0 or any(p["ops"] == HALF for p in op["programs"])):
        return "search_each"  # a program on the SCAN route: gathering is off, or it matches half the rows and is not forced
    return None


def run_of_queries(ops, i):
    kinds = []
    while i < len(ops) and ops[i]["op"] in H.QUERIES:
        kinds.append(ops[i]["op"])
        i += 1
    return set(kinds), i


def conditions(ops, expected, space):
    """{condition: step} for every coverage condition this history meets."""
    st = trace(ops, expected, space)
    kinds = [op["op"] for op in ops]
    n = len(ops)
    met = {}

    def put(name, step):
        met.setdefault(name, step)

    for i, op in enumerate(ops):
        k = kinds[i]
        nxt = kinds[i + 1] if i + 1 < n else None
        if st[i]["regrowths"] >= 2 and k in H.ATTR_READERS:
            put("a", i)
        if filter_route(op, st[i]):  # (b): only mutations between the two searches, `x` among them
            j = i + 1
            while j < n and kinds[j] in H.MUTATIONS and kinds[j] not in ("set_strategy", "set_tuning"):
                j += 1
            if j > i + 1 and j < n and filter_route(ops[j], st[j]):
                for x in range(i + 1, j):
                    name = kinds[x] if kinds[x] != "reset" else ("reset" if ops[x]["space"] is None else "reset_other")
                    if name in ("append", "tombstone", "compact", "reset", "reset_other"):
                        put("b_" + name, i)
            if st[i]["space"] == "l2" and i + 3 < n and filter_route(ops[i + 1], st[i + 1]) and ops[i + 1]["nq"] != op["nq"] \
                    and kinds[i + 2] == "tombstone" and kinds[i + 3] in SEARCHES:
                put("h", i)
        m = masked(op, st[i])
        if m and nxt in SEARCHES:
            put("c_" + m, i)
        if m and nxt in H.MUTATIONS and i + 2 < n and kinds[i + 2] in SEARCHES:
            put("c_mutation", i)
        if (k == "range" or (k in SEARCHES and op["k"] > 64)) and kinds[i + 1:i + 5] == ["append", "range", "compact", "range"]:
            put("d", i)
        if k == "refuse" and nxt in H.QUERIES:
            put("e_" + op["which"], i)
        emptied = (k == "compact" and st[i]["total"] > 0 and expected[i]["counts"] == (0, 0)) or (k == "reset" and st[i]["total"] > 0)
        if emptied:
            first, j = run_of_queries(ops, i + 1)
            if j < n and kinds[j] == "append":
                again, _ = run_of_queries(ops, j + 1)
                if len(first & again) >= 4:
                    put("f_" + k, i)
        if k in H.MUTATIONS and nxt in H.QUERIES:
            put(f"g_{k}>{nxt}", i)
        if k == "define_attr" and op["attr"] == 3 and st[i]["total"] > 0 and "i_defined" not in met:
            put("i_defined", i)
        if "i_defined" in met and i > met["i_defined"]:
            if k in ("facet_values", "search_distinct") and op["attr"] == 3:
                put("i_" + k, i)
            programs = ([op["program"]] if op.get("program") else []) + op.get("programs", [])
            if k in H.ATTR_READERS and any(o[1] == 3 and o[0] not in (W.AND, W.OR, W.NOT, W.TRUE) for p in programs for o in p["ops"]):
                put("i_where", i)
        if k == "search_distinct":
            put(f"j_oversample{st[i]['oversample']}", i)
        if k == "search_each":
            put(f"j_gather{st[i]['gather']}", i)
    if all(x in met for x in ("i_defined", "i_facet_values", "i_search_distinct", "i_where")):
        met["i"] = met["i_defined"]
    if all(f"j_{x}" in met for x in ("oversample0", "oversample4", "gather0", "gather150", f"gather{1 << 30}")):
        met["j"] = met["j_oversample0"]
    return met


WANTED = (["a", "d", "h", "i", "j", "c_search_mask", "c_search_where", "c_search_each", "c_mutation", "f_compact", "f_reset"]
          + ["b_" + x for x in ("append", "tombstone", "compact", "reset", "reset_other")]
          + ["e_" + w for w in H.REFUSALS] + [f"g_{m}>{q}" for m, q in H.PAIRS])


# ---------------------------------------------------------------- determinism
def test_make_history_is_deterministic_and_json_serialisable():
    key = H.SMALL[0]
    ops, expected = H.make_history(*key)
    H._history.cache_clear()
    ops2, expected2 = H.make_history(*key)
    assert ops2 is not ops and json.dumps(ops) == json.dumps(ops2)
    assert json.loads(json.dumps(ops)) == ops
    for a, b in zip(expected, expected2):
        assert a["args"].keys() == b["args"].keys()
        for name, x in a["args"].items():
            if isinstance(x, np.ndarray):
                assert np.array_equal(x.view(np.uint8), b["args"][name].view(np.uint8)), name
    other, _ = H.make_history(key[0] + 1, *key[1:])
    assert json.dumps(other) != json.dumps(ops)


def test_capacity_after_mirrors_reserve_rows_and_compaction():
    assert H.capacity_after(0, 1) == 768 and H.capacity_after(0, 769) == 1536 and H.capacity_after(768, 768) == 768
    assert H.capacity_after(768, 769) == 1536           # 1.5 x 768 = 1152 -> the next granule
    assert H.capacity_after(1536, 1537) == 2304         # 1.5 x 1536
    assert H.capacity_after(1536, 5000) == 5376         # the rows needed, when they exceed 1.5 x
    assert H.capacity_after_compact(3072, 10, 0) == 3072 and H.capacity_after_compact(3072, 10, 5) == 768
    assert H.capacity_after_compact(3072, 0, 9) == 768 and H.capacity_after_compact(3072, 769, 1) == 1536


# ---------------------------------------------------------------- the model against the oracle engines it is made of
def test_history_model_agrees_with_the_individual_oracle_engines():
    rng = np.random.default_rng(3)
    d, n = 12, 400
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows[7] = rows[300]
    qs = rng.standard_normal((5, d), dtype=np.float32)
    engines = [cls(d, "cosine") for cls in (H.HistoryModel, DistinctOracleEngine, FacetOracleEngine, EachOracleEngine, EachRangeOracleEngine)]
    for e in engines:
        for attr, kind in ((0, "int64"), (1, "float64"), (2, "int64")):
            e.define_attr(attr, kind)
        e.append(rows[:250])
        e.append(rows[250:])
        for attr in range(3):
            e.set_attr(attr, 0, H.column_values(attr, n, np.random.default_rng(attr), n))
        e.tombstone(np.arange(0, n, 7))
    model, distinct, facet, each, each_range = engines
    half, few = H.program_of({"ops": HALF, "set": []}), H.program_of({"ops": [[W.EQ, 2, 3, 0]], "set": []})
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))  # noqa: E731
    assert same(model.search64(qs, 9, where=half), distinct.search64(qs, 9, where=half))
    assert same(model.search(qs, 9, (np.arange(n) % 3 > 0).astype(np.uint8)), facet.search(qs, 9, (np.arange(n) % 3 > 0).astype(np.uint8)))
    assert same(model.search_distinct(qs, 6, 0, where=half, want64=True), distinct.search_distinct(qs, 6, 0, where=half, want64=True))
    assert same(model.facet_values(0, 100, few)[:2], facet.facet_values(0, 100, few)[:2])
    assert model.facet_values(0, 100, few)[2:] == facet.facet_values(0, 100, few)[2:]
    edges = np.array([-1.0, 0.0, 1.5])
    assert np.array_equal(model.facet_bins(1, edges)[0], facet.facet_bins(1, edges)[0])
    of = np.array([0, -1, 1, 0, 1], np.int32)
    assert same(model.search_each(qs, 4, [half, few], of, want64=True), each.search_each(qs, 4, [half, few], of, want64=True))
    assert np.array_equal(model.count_each([half, few]), each.count_each([half, few]))
    got, want = model.range_each(qs, 0.9, 64, [half, few], of), each_range.range_each(qs, 0.9, 64, [half, few], of)
    assert sum(len(g[0]) for g in got) > 0 and all(same(g, w) for g, w in zip(got, want))
    assert all(same(g, w) for g, w in zip(model.range(qs, 0.9, 64, where=few), facet.range(qs, 0.9, 64, where=few)))
    assert model.where_count(half) == facet.where_count(half) and np.array_equal(model.where_labels(few), facet.where_labels(few))
    # what the model adds: a column defined after rows is all absent, reset keeps the definitions and may change the space
    model.define_attr(3, "int64")
    assert (model.get_attr(3, 0, n) == W.INT64_ABSENT).all()
    values, counts, matched, absent = model.facet_values(3, 4)
    assert values.size == 0 and matched == absent == model.counts()[0] - model.counts()[1]
    model.define_attr(3, "int64")
    model.reset("ip")
    assert model.counts() == (0, 0) and model.space == "ip" and sorted(model._cols) == [0, 1, 2, 3]
    assert model.append(rows[:3]) == 0 and np.isnan(model.get_attr(1, 0, 3, np.float64)).all()
    for refused in (lambda: model.search(qs, 0), lambda: model.search_distinct(qs, 3, 1), lambda: model.facet_values(0, 0),
                    lambda: model.facet_bins(2, np.array([5, 3])), lambda: model.where_count(H.program_of({"ops": [[W.EQ, 9, 1, 0]], "set": []}))):
        with pytest.raises(RuntimeError):
            refused()


def test_the_shard_history_passes_through_logical_shards_of_oracle_engines():
    """The ops of the shard history are ones ``MultiDeviceEngine`` answers as one engine would (here over NumPy shards)."""
    from mlvectordb_amd.multi_device import MultiDeviceEngine
    from oracle.engine import OracleScanEngine

    seed, space, d, _ = key = H.MULTI[0]
    ops, expected = H.make_history(*key)
    assert {"range", "pair_distances", "get_rows", "search_mask", "compact"} <= {op["op"] for op in ops}
    engine = MultiDeviceEngine(d, space, [0, 0, 0], shard_factory=lambda dev: OracleScanEngine(d, space))
    try:
        assert H.run_history(engine, ops, expected, H.history_tag(*key))["steps"] == len(ops)
    finally:
        engine.close()


# ---------------------------------------------------------------- coverage
def test_the_committed_seed_set_meets_every_coverage_condition():
    where = {}
    for key in H.HISTORIES:
        ops, expected = H.make_history(*key)
        for name, step in conditions(ops, expected, key[1]).items():
            where.setdefault(name, (key[0], step))
    for name in WANTED:
        if name in where:
            print(f"condition {name}: seed {where[name][0]}, step {where[name][1]}")
    missing = [name for name in WANTED if name not in where]
    assert not missing, f"coverage conditions never met: {missing}"
    # the histories stay small, and the large ones cross the threshold of `auto` in both directions
    for key in H.SMALL:
        ops, expected = H.make_history(*key)
        assert max(e["counts"][0] for e in expected if "counts" in e) <= H.MAX_ROWS_SMALL + 40, key
        print(f"history {H.history_tag(*key)}: {len(ops)} steps")
    for key in H.LARGE:
        ops, expected = H.make_history(*key)
        st = trace(ops, expected, key[1])
        routes = [filter_route(op, s) for op, s in zip(ops, st) if op["op"] in SEARCHES and op["nq"] >= 12]
        assert routes[0] is False and True in routes and False in routes[routes.index(True):], (key, routes)
        assert sum(op["op"] in H.QUERIES for op in ops) <= 20


# ---------------------------------------------------------------- sensitivity: three seeded stale-state defects
class ForgetsColumnsOnCompact(H.HistoryModel):
    fired = None

    def compact(self):
        cols = self._cols
        old = super().compact()
        stale = {a: col[:old.size].copy() for a, col in cols.items()}
        if self.fired is None and any(not np.array_equal(stale[a].view(np.int64), self._cols[a].view(np.int64)) for a in cols):
            self.fired = self.step
        self._cols = stale
        return old


class KeepsTheRowMask(H.HistoryModel):
    fired = None
    _stale = None

    def search(self, queries, k, mask=None, where=None):
        if mask is not None:
            self._stale = np.asarray(mask)
        elif where is None and self._stale is not None:
            if self._stale.size == self._rows.shape[0]:
                mask = self._stale
                if self.fired is None and (mask == 0)[~self._deleted].any():
                    self.fired = self.step
            self._stale = None
        return super().search(queries, k, mask, where)


class SearchesTheOldRows(H.HistoryModel):
    fired = None
    _snapshot = None
    _appended = False

    def append(self, rows):
        self._appended = True
        return super().append(rows)

    def search(self, queries, k, mask=None, where=None):
        if self._appended and self._snapshot is not None and mask is None and where is None and \
                self._snapshot[0].shape[0] <= self._rows.shape[0] and \
                np.array_equal(self._snapshot[0], self._rows[:self._snapshot[0].shape[0]]):
            keep = self._rows, self._deleted
            self._rows, self._deleted = self._snapshot[0], keep[1][:self._snapshot[0].shape[0]]
            try:
                if self.fired is None:
                    self.fired = self.step
                return super().search(queries, k)
            finally:
                self._rows, self._deleted = keep
                self._appended = False
                self._snapshot = (self._rows.copy(), None)
        if mask is None and where is None:
            self._snapshot, self._appended = (self._rows.copy(), None), False
        return super().search(queries, k, mask, where)


@pytest.mark.parametrize("defect", [ForgetsColumnsOnCompact, KeepsTheRowMask, SearchesTheOldRows])
def test_the_driver_reports_a_seeded_stale_state_defect(defect, tmp_path, monkeypatch):
    from tests import conftest

    monkeypatch.setattr(conftest, "OUT_DIR", tmp_path)
    reported, real_call = 0, H.call
    for key in H.SMALL[:4]:
        ops, expected = H.make_history(*key)
        engine = defect(key[2], key[1])
        stepped = []

        def counted(e, op, a, engine=engine, stepped=stepped):
            if e is engine:
                engine.step = len(stepped)
                stepped.append(op["op"])
            return real_call(e, op, a)

        monkeypatch.setattr(H, "call", counted)
        tag = H.history_tag(*key)
        try:
            H.run_history(engine, ops, expected, tag)
        except AssertionError as err:
            failed = len(stepped) - 1
            assert f"history {tag}: step {failed}, op " in str(err) and f"seed{key[0]}" in str(err)
            assert engine.fired is not None
            if defect is ForgetsColumnsOnCompact:  # first seen by the first later call that reads the columns
                assert failed > engine.fired and ops[failed]["op"] in H.ATTR_READERS + ("refuse",), ops[failed]
                between = [ops[s]["op"] for s in range(engine.fired + 1, failed) if ops[s]["op"] in H.ATTR_READERS]
                assert not between, f"{tag}: fired at step {engine.fired}, reported at {failed}, after {between}"
            else:                                   # seen by the call that it fires in: a search, or the unfiltered queries of a search_each
                assert failed == engine.fired and ops[failed]["op"] in SEARCHES + ("search_each",), (failed, engine.fired, ops[failed])
            dumped = json.loads((tmp_path / f"history_{tag}.json").read_text())
            assert dumped["failed_step"] == failed and dumped["ops"] == ops[:failed + 1]
            print(f"{defect.__name__}: {tag} fired at step {engine.fired}, reported at step {failed} ({ops[failed]['op']})")
            reported += 1
        else:  # the history ran through: the defect never showed, or only where no later call could see it
            assert engine.fired is None or (defect is ForgetsColumnsOnCompact and not any(
                op["op"] in H.ATTR_READERS for op in ops[engine.fired + 1:])), f"{tag}: fired at step {engine.fired}, never reported"
        monkeypatch.setattr(H, "call", real_call)
    assert reported >= 2, f"{defect.__name__}: reported in {reported} of 4 histories"


# ---------------------------------------------------------------- redraws
def test_near_tie_redraws_stay_under_one_percent():
    drawn = redrawn = 0
    for key in H.HISTORIES:
        a, b = H.redraw_counts(*key)
        drawn, redrawn = drawn + a, redrawn + b
    print(f"{redrawn} of {drawn} drawn queries were redrawn")
    assert drawn > 300 and redrawn <= 0.01 * drawn
