"""The seeded call histories of tests/history_helpers.py without a GPU: they are deterministic, the first ones are pinned by the
sha256 of their op lists, the models agree with the oracle engines they are composed from, the committed seed sets meet every
coverage condition (a to j for the first histories, k to w for the wide ones, ``RECENT_WANTED`` for the recent ones of
tests/history_recent_helpers.py; each printed with the seed and step that meets it), the driver reports three plus five plus
six seeded stale-state defects, and near-tie and guard redraws stay under 1 % of the drawn queries."""
import hashlib
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


# ---------------------------------------------------------------- the first histories are pinned
# sha256(json.dumps(ops)) of every history of HISTORIES as generated before the wide scale existed: new ops and program kinds
# live in scales of their own, so that these seeds keep drawing what they drew.
PINNED = {
    "small_l2_d20_seed0": "626dbe9888705c21eedbe3f9b8be9739267a6497a35301372648ec86d5e3ef06",
    "small_l2_d20_seed1": "b3aba4a086d5f19f003c218810a007fceec1028fac0b06d74828b13b83c69c1b",
    "small_cosine_d64_seed2": "14400f45c4b8484234286a4ce4e986959d9a77a98e6d1b12231c94e46690a3a0",
    "small_cosine_d64_seed3": "0a211e6d419f59c49595e7e6813546171d0d956efcdc778e3309010c11593d57",
    "small_ip_d128_seed4": "d422f1da0dbc62f45de75d71dedefbd65a99d668a6a0d1ca661fc7f66242cfac",
    "small_ip_d128_seed5": "f0dc7388bbae902c17d2526827535108eeeffed53cdac4be3c9edb11cd7f5e63",
    "small_l2_d256_seed6": "97a17951ed51e5b5c9547dcaeffe90a707027c6d2b55f88856bb52b0eb40c5cb",
    "small_l2_d256_seed7": "8cd3a0b5df189f2d42e89487d3564318f4548e89f76284a43efa571d51672b3a",
    "small_cosine_d100_seed8": "5c804b324151158e185b0886b052d25ba7c3057f396a007c878b749091ae12f0",
    "small_cosine_d100_seed9": "c6cc02820740349a6decc2ce9aa6e91d474b67db96002bcc90e5fae6d36bea32",
    "large_l2_d64_seed100": "5f0eeca469b09fa431a96bba515a3bf72f1bdaa22b544a4b97711a9a2d1dca2b",
    "large_cosine_d64_seed101": "1591b3011333674f2bb4309d74f5bd7248e3a9a230393ec45a91434551817f55",
    "large_ip_d64_seed102": "3c823f4c4ad7cee5cfa35d1477927ba794b1c672cb3b5062ed3296e2280d523f",
    "multi_cosine_d48_seed200": "fae4c7f1d6cda9416b7ab8a917bfa337bf41709adcba36b725a2bf25a982d2d7",
}


def test_the_first_histories_generate_byte_identical_op_lists():
    assert {H.history_tag(*key) for key in H.HISTORIES} == set(PINNED)
    for key in H.HISTORIES:
        ops, _ = H.make_history(*key)
        assert hashlib.sha256(json.dumps(ops).encode()).hexdigest() == PINNED[H.history_tag(*key)], H.history_tag(*key)


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
    _the_wide_model_agrees_with_the_oracle_engines_of_the_newer_entries(rows, qs)


def _the_wide_model_agrees_with_the_oracle_engines_of_the_newer_entries(rows, qs):
    """The same state -- two appends, every column valued, tombstones -- in ``WideHistoryModel`` and in each oracle engine it
    is composed from; one call per new entry, list programs inside the kNN entries included."""
    from mlvectordb_amd import _native
    from tests.grouped_helpers import GroupedOracleEngine
    from tests.like_helpers import LikeOracleEngine
    from tests.maxsim_helpers import MaxSimOracleEngine, offsets_of
    from tests.mmr_helpers import MmrOracleEngine
    from tests.order_helpers import OrderOracleEngine
    from tests.sparse_helpers import SparseOracleEngine, random_corpus, sparse_csr

    n, d = rows.shape
    lists = H.csr(H.wide_lists(np.random.default_rng(4), n))
    vectors = sparse_csr(random_corpus(np.random.default_rng(5), n, H.SPARSE_VOCAB, True))
    engines = [cls(d, "l2") for cls in (H.WideHistoryModel, SparseOracleEngine, OrderOracleEngine, GroupedOracleEngine,
                                        MmrOracleEngine, LikeOracleEngine, MaxSimOracleEngine)]
    for e in engines:
        pooled = isinstance(e, SparseOracleEngine)
        for attr, kind in ((0, "int64"), (1, "float64"), (2, "int64")) + (((4, "int64_list"), (5, "sparse")) if pooled else ()):
            e.define_attr(attr, kind)
        e.append(rows[:250])
        e.append(rows[250:])
        for attr in range(3):
            e.set_attr(attr, 0, H.column_values(attr, n, np.random.default_rng(attr), n))
        if pooled:
            e.set_attr_list(4, 0, lists)
            e.set_attr_sparse(5, 0, vectors)
        e.tombstone(np.arange(0, n, 7))
    model, sparse, order, grouped, mmr, like, maxsim = engines
    half = H.program_of({"ops": HALF, "set": []})
    tagged = H.program_of({"ops": [[W.HAS, 4, 3, 0], [W.LT, 2, 8, 0], [W.AND, 0, 0, 0]], "set": []})
    same = lambda a, b: len(a) == len(b) and all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))  # noqa: E731
    column = lambda c: tuple(vars(c).values())  # noqa: E731
    assert same(model.where_ordered(1, 20, half, True, 3)[:2], order.where_ordered(1, 20, half, True, 3)[:2])
    assert model.where_ordered(0, 5, half)[2:] == order.where_ordered(0, 5, half)[2:]
    assert same(model.search_grouped(qs, 4, 3, 0, where=half, want64=True), grouped.search_grouped(qs, 4, 3, 0, where=half, want64=True))
    assert same(model.search_mmr(qs, 5, 40, 0.3, where=half, want64=True), mmr.search_mmr(qs, 5, 40, 0.3, where=half, want64=True))
    ex = (np.array([3, 9, 14, 200]), np.array([1.0, 0.5, 1.0, -0.25]), np.array([0, 2, 4]))  # (14 is tombstoned)
    assert same(model.search_like(*ex, 6, where=half, want64=True, want_queries=True),
                like.search_like(*ex, 6, where=half, want64=True, want_queries=True))
    toks, off = np.concatenate([qs, qs[:3]]), offsets_of([3, 1, 4])
    assert same(model.search_maxsim(toks, off, 5, 0, half, True), maxsim.search_maxsim(toks, off, 5, 0, half, True))
    # the entries of the pooled columns, and list programs inside the kNN entries, against the sparse / tags / mutate engine
    sq = H._sparse_queries(np.random.default_rng(6), 4)
    for e in (model, sparse):
        assert e.set_attr_at(2, np.array([5, 14, 30]), np.array([1, 2, 3])) == 2
        assert e.update_where(tagged, [(0, _native.SET_ADD, 1), (2, _native.SET_ASSIGN, 4)])[1] == 0
        assert e.update_where(half, [(0, _native.SET_ADD, 2 ** 63 - 1)])[1] > 0
        assert e.set_attr_list_at(4, np.array([8, 14, 2]), H.csr([[1, 2], [3], None])) == 2
        assert e.set_attr_sparse_at(5, np.array([9, 14]), sparse_csr([{3: 0.5}, {4: 1.0}])) == 1
        assert e.update_where_list(tagged, 4, np.array([2, 6])) > 0
    assert np.array_equal(model.tombstone_where(tagged), sparse.tombstone_where(tagged))
    for attr in range(3):
        assert np.array_equal(model.get_attr(attr, 0, n, np.float64), sparse._cols[attr].astype(np.float64), equal_nan=True)
    assert same(column(model.get_attr_list(4, 0, n)), column(sparse.get_attr_list(4, 0, n)))
    assert same(column(model.get_attr_sparse(5, 0, n)), column(sparse.get_attr_sparse(5, 0, n)))
    assert model.list_stats(4) == sparse.list_stats(4) and model.list_stats(5) == sparse.list_stats(5)
    got, want = model.facet_list_values(4, 4096, half), sparse.facet_list_values(4, 4096, half)
    assert same(got[:2], want[:2]) and got[2:] == want[2:]
    has = H.program_of({"ops": [[W.HAS_ANY, 4, 0, 2, ]], "set": [2, 6]})
    assert same(model.search_batch_sparse(5, sq, 7, has), sparse.search_batch_sparse(5, sq, 7, has))
    assert same(model.search_grouped(qs, 4, 3, 0, where=has, want64=True)[:4], grouped_with(sparse, qs, 4, 3, has))
    assert np.array_equal(model.compact(), sparse.compact()) and model.list_stats(4) == sparse.list_stats(4)
    assert same(model.search_batch_sparse(5, sq, 7, has), sparse.search_batch_sparse(5, sq, 7, has))
    # what the model adds: pools mirrored, a reset that empties the lists and keeps their definitions, the refusals
    used, cap, live = model.pools()[4]
    assert used == cap == live == model.list_stats(4)[1] > 0
    model.reset()
    assert model.pools()[4] == (0, cap, 0) and model.append(rows[:5]) == 0
    assert not model.get_attr_list(4, 0, 5).present.any() and not model.get_attr_sparse(5, 0, 5).present.any()
    tok129 = np.zeros((129, d), np.float32)
    for status, refused in ((1, lambda: model.search_mmr(qs, 10, 9, 0.5)), (1, lambda: model.search_grouped(qs, 3, 0, 0)),
                            (6, lambda: model.search_grouped(qs, 3, 65, 0)), (1, lambda: model.search_like([5], [1.0], [0, 1], 3)),
                            (1, lambda: model.search_maxsim(tok129[:3], offsets_of([2, 0, 1]), 3, 0)),
                            (1, lambda: model.search_maxsim(tok129, offsets_of([129]), 3, 0)),
                            (1, lambda: model.where_ordered(2, 4091, None, False, 6)),
                            (1, lambda: model.set_attr_at(2, np.array([0, 0]), np.array([1, 2]))),
                            (1, lambda: model.set_attr(4, 0, np.array([1]))), (1, lambda: model.set_attr_list(5, 0, H.csr([[1]]))),
                            (1, lambda: model.search_batch_sparse(4, sq, 5))):
        with pytest.raises(RuntimeError) as err:
            refused()
        assert H._status_of(err.value) == status


def grouped_with(engine, qs, k, g, where):
    """``search_grouped`` of tests/grouped_helpers.py over the state of another oracle engine (one that evaluates list programs)."""
    from oracle import exact_scan
    from tests.grouped_helpers import grouped_knn

    dist = exact_scan.exact_distances(qs, engine._rows, engine.space)
    labels, d64, counts, gcnt, _ = grouped_knn(dist, engine._cols[0], engine.match(where), k, g)
    return labels, d64.astype(np.float32), counts, gcnt


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


# ================================================================ the wide histories (conditions k to w)
LIST_OPS = (W.HAS, W.HAS_ANY, W.HAS_ALL, W.LEN)
GROUP_READERS = ("search_grouped", "search_maxsim", "search_distinct", "where_ordered")


def programs_of(op):
    return ([op["program"]] if op.get("program") else []) + op.get("programs", [])


def list_leaf(op, attr):
    return any(o[0] in LIST_OPS and o[1] == attr for p in programs_of(op) for o in p["ops"])


def pooled_leaf(op):
    """A list op, or EXISTS on a list or sparse column, in one of the op's programs."""
    return any(o[0] in LIST_OPS or (o[0] == W.EXISTS and o[1] in H.POOLED) for p in programs_of(op) for o in p["ops"])


PROGRAM_TAKING = ("search_where", "search_each", "range_where", "range_each", "search_distinct", "facet_values", "facet_bins",
                  "where_count", "where_labels", "count_each", "update_where", "tombstone_where", "update_where_list",
                  "where_ordered", "search_mmr", "search_grouped", "search_like", "search_maxsim", "facet_list_values",
                  "search_batch_sparse")


def write_floor(op):
    """The lowest row a write to a pooled column may touch."""
    if "first" in op:
        return op["first"]
    if "labels" in op:
        return min(op["labels"])
    return op.get("lo", 0)


def wide_trace(ops, expected, space):
    """The handle's state BEFORE each step of a wide history, from the ops and what the model counted (rows, tombstones,
    used / capacity / live values of every pool)."""
    st = dict(strategy="auto", total=0, deleted=0, space=space, cap=0, regrowths=0, valued=set(), pools={})
    out = []
    for op, exp in zip(ops, expected):
        out.append({**st, "valued": set(st["valued"])})
        kind = op["op"]
        if kind == "set_strategy":
            st["strategy"] = op["strategy"]
        elif kind == "append":
            cap = H.capacity_after(st["cap"], st["total"] + op["n"])
            if cap != st["cap"] and st["cap"] and {H.LIST_A, H.SPARSE_A} <= st["valued"]:
                st["regrowths"] += 1
            st["cap"] = cap
        elif kind == "compact":  # (the slot columns are rebuilt: what regrew before is gone)
            st["cap"] = H.capacity_after_compact(st["cap"], st["total"] - st["deleted"], st["deleted"])
            st["regrowths"] = 0
        elif kind in ("set_attr_list", "set_attr_sparse") and op["n"]:
            st["valued"] = st["valued"] | {op["attr"]}
        elif kind == "reset":
            st.update(regrowths=0, valued=set())
            st["space"] = op["space"] or st["space"]
        if "counts" in exp:
            st["total"], st["deleted"] = exp["counts"]
        st["pools"] = exp["pools"]
    return out


def run_of(ops, i, kinds):
    seen = []
    while i < len(ops) and ops[i]["op"] in kinds:
        seen.append(i)
        i += 1
    return seen, i


def wide_conditions(ops, expected, space):
    """{condition: step} for every condition k to w this wide history meets."""
    st = wide_trace(ops, expected, space)
    kinds = [op["op"] for op in ops]
    n = len(ops)
    met = {}
    grow = {a: 0 for a in H.POOLED}
    floor = {a: np.inf for a in H.POOLED}
    late = dict(defined=False, written=set())

    def put(name, step):
        met.setdefault(name, step)

    def nq_of(op):
        return len(op["groups"]) if op["op"] == "search_like" else op["nq"]

    for i, op in enumerate(ops):
        k = kinds[i]
        nxt = kinds[i + 1] if i + 1 < n else None
        s = st[i]
        pooled_name = lambda a: "sparse" if H.POOLED[a] == "sparse" else "list"  # noqa: E731
        # (k)
        if k in H.WIDE_MUTATIONS and nxt in H.WIDE_QUERIES and (k in H.NEW_MUTATIONS or nxt in H.NEW_QUERIES):
            put(f"k_{k}>{nxt}", i)
        # (l)
        if k == "compact" and i + 2 < n:
            for a, (used, _, live) in s["pools"].items():
                tag_query = (ops[i + 1]["op"] == "search_batch_sparse" and ops[i + 1]["attr"] == a) or list_leaf(ops[i + 1], a)
                if used > live > 0 and tag_query and kinds[i + 2] == "list_stats" and ops[i + 2]["attr"] == a:
                    assert expected[i + 2]["want"][0] == expected[i + 2]["want"][1] > 0  # the repack: used == live
                    put(f"l_{pooled_name(a)}_{'dead' if s['deleted'] else 'clean'}", i)
        # (m)
        if k in ("compact", "reset"):
            grow, floor = {a: 0 for a in H.POOLED}, {a: np.inf for a in H.POOLED}
        if k in H.NEW_MUTATIONS and op.get("attr") in s["pools"] and k != "set_attr_at":
            a = op["attr"]
            used, cap, live = s["pools"][a]
            if expected[i]["pools"][a][1] != cap:
                assert expected[i]["pools"][a][1] == H.pool_capacity_after(cap, expected[i]["pools"][a][0])
                if used > 0 and live > 0:
                    grow[a] += 1
            if grow[a]:
                floor[a] = min(floor[a], write_floor(op))
        if k in ("get_attr_list", "get_attr_sparse") and op["first"] == 0 and 0 < op["n"] <= floor[op["attr"]] and grow[op["attr"]] >= 2:
            put(f"m_{pooled_name(op['attr'])}", i)
        # (n)
        if s["regrowths"] >= 2:
            if k in ("get_attr_list", "facet_list_values", "search_batch_sparse") and \
                    op["attr"] == (H.SPARSE_A if k == "search_batch_sparse" else H.LIST_A):
                put("n_" + k, i)
            if list_leaf(op, H.LIST_A):
                put("n_tag_program", i)
        # (o) and (w): a reset or an emptying compaction, what is asked then, a refill, what is asked again
        emptied_by_compact = (k == "compact" and s["total"] > 0 and expected[i]["counts"] == (0, 0) and i > 0
                              and kinds[i - 1] == "tombstone_where" and ops[i - 1]["program"]["ops"] == [[W.TRUE, 0, 0, 0]])
        if k == "reset" and s["total"] > 0 and nxt == "append":
            first, j = run_of(ops, i + 2, H.WIDE_QUERIES)
            sets, j2 = run_of(ops, j, H.WIDE_MUTATIONS)
            again, _ = run_of(ops, j2, H.WIDE_QUERIES)
            absent = True
            for x in first:
                want = expected[x]["want"]
                if kinds[x] == "list_stats":
                    absent &= tuple(want) == (0, 0)
                elif kinds[x] in ("get_attr_list", "get_attr_sparse"):
                    absent &= ops[x]["n"] > 0 and not want.present.any()
                elif kinds[x] == "search_batch_sparse":
                    absent &= not want[2].any()
                elif kinds[x] == "facet_list_values":
                    absent &= want[0].size == 0 and want[2] == want[3] > 0
                elif kinds[x] == "where_count" and list_leaf(ops[x], H.LIST_A):
                    absent &= want == 0
            if (absent and set(H.LIST_READERS) <= {kinds[x] for x in first} and {"set_attr_list", "set_attr_sparse"} <= {kinds[x] for x in sets}
                    and set(H.LIST_READERS) <= {kinds[x] for x in again}):
                put("o_reset" if op["space"] is None else "o_reset_other", i)
        if emptied_by_compact or (k == "reset" and s["total"] > 0):
            first, j = run_of(ops, i + 1, H.WIDE_QUERIES)
            if j < n and kinds[j] == "append":
                _, j2 = run_of(ops, j, H.WIDE_MUTATIONS)
                again, _ = run_of(ops, j2, H.WIDE_QUERIES)
                padding = all(not np.asarray(expected[x]["want"][2]).any() for x in first if kinds[x] in H.MASKABLE)
                if padding and set(H.NEW_QUERIES) <= {kinds[x] for x in first} and set(H.NEW_QUERIES) <= {kinds[x] for x in again}:
                    put("w_" + k, i)
        # (p)
        if k in H.INNER_SEARCHES and s["strategy"] == "filter":
            between, j = run_of(ops, i + 1, [m for m in H.WIDE_MUTATIONS if m not in ("set_strategy", "set_tuning")])
            if between and j < n and kinds[j] == k:
                for x in between:
                    if kinds[x] in ("tombstone_where", "tombstone", "append", "compact"):
                        put(f"p_{k}_{kinds[x]}", i)
            if s["space"] == "l2" and i + 3 < n and nxt in H.INNER_SEARCHES and nq_of(ops[i + 1]) != nq_of(op) \
                    and kinds[i + 2] == "tombstone_where" and kinds[i + 3] in SEARCHES:
                put("p_l2", i)
        # (q)
        if k in H.MASKABLE and op.get("program") is not None:
            if nxt == "search64":
                put(f"q_{k}_plain", i)
            if nxt == k and ops[i + 1].get("program") is None:
                put(f"q_{k}_own", i)
        # (r)
        if k == "define_attr" and op["attr"] == H.LATE_LIST and s["total"] > 0 and not late["defined"]:
            late["defined"] = True
            put("r_defined", i)
        elif late["defined"]:
            if k in H.NEW_MUTATIONS and op.get("attr") in (H.LATE_LIST, H.LATE_SPARSE) and k != "set_attr_at":
                late["written"].add(op["attr"])
            phase = {0: "absent", 2: "set"}.get(len(late["written"]))
            if phase:
                if list_leaf(op, H.LATE_LIST):
                    put(f"r_{phase}_has", i)
                if k in ("facet_list_values", "get_attr_list") and op["attr"] == H.LATE_LIST:
                    put(f"r_{phase}_{k}", i)
                if k in ("get_attr_sparse", "search_batch_sparse") and op["attr"] == H.LATE_SPARSE:
                    put(f"r_{phase}_{k}", i)
        # (s)
        if nxt in GROUP_READERS:
            written = [a for a, _, _ in op["assigns"]] if k == "update_where" else [op["attr"]] if k == "set_attr_at" else []
            if ops[i + 1]["attr"] in written and ops[i + 1]["attr"] != 1:
                put(f"s_{k}>{nxt}", i)
            if k == "update_where" and nxt == "where_ordered" and ops[i + 1]["attr"] == 1 and [1, 1] in [x[:2] for x in op["assigns"]]:
                put("s_float_add", i)
        # (t)
        if k == "update_where" and expected[i]["want"][1] > 0 and nxt == "get_attr" and ops[i + 1]["attr"] in [x[0] for x in op["assigns"]]:
            put("t", i)
        # (u)
        if k == "tombstone" and op["mode"] == "labels" and op["labels"] and kinds[i + 1:i + 7] == \
                ["search_like", "get_rows_at", "compact", "search_like", "get_rows_at", "refuse"] and i + 7 < n:
            dead, new_total = set(op["labels"]), expected[i + 3]["counts"][0]
            stale = ops[i + 6]
            if (any(set(g) & dead for g in ops[i + 1]["groups"]) and set(ops[i + 2]["labels"]) <= dead
                    and stale["which"] == "like_label" and new_total <= stale["label"] < st[i + 3]["total"]
                    and expected[i + 6]["want"] == ("refused", 1) and kinds[i + 7] in H.WIDE_QUERIES):
                put("u", i)
        # (v)
        if k == "refuse" and op["which"] in H.WIDE_REFUSALS and expected[i]["want"][0] == "refused" and nxt in H.WIDE_QUERIES:
            put("v_" + op["which"], i)
    for name, parts in (("n", ["n_get_attr_list", "n_tag_program", "n_facet_list_values", "n_search_batch_sparse"]),
                        ("r", ["r_defined"] + [f"r_{p}_{x}" for p in ("absent", "set") for x in
                                               ("has", "facet_list_values", "get_attr_list", "get_attr_sparse", "search_batch_sparse")])):
        if all(x in met for x in parts):
            met[name] = met[parts[0]]
    return met


WIDE_WANTED = ([f"k_{m}>{q}" for m, q in H.WIDE_PAIRS]
               + [f"l_{c}_{v}" for c in ("list", "sparse") for v in ("clean", "dead")] + ["m_list", "m_sparse", "n", "o_reset", "o_reset_other"]
               + [f"p_{i}_{x}" for i in H.INNER_SEARCHES for x in ("tombstone_where", "tombstone", "append", "compact")] + ["p_l2"]
               + [f"q_{k}_{x}" for k in H.MASKABLE for x in ("plain", "own")] + ["r"]
               + [f"s_{w}>{r}" for w in ("update_where", "set_attr_at") for r in GROUP_READERS] + ["s_float_add", "t", "u"]
               + ["v_" + w for w in H.WIDE_REFUSALS] + ["w_compact", "w_reset"])


def test_the_wide_histories_meet_every_coverage_condition():
    where, tagged = {}, {}
    for key in H.WIDE:
        ops, expected = H.make_history(*key)
        for name, step in wide_conditions(ops, expected, key[1]).items():
            where.setdefault(name, (key[0], step))
        assert max(e["counts"][0] for e in expected if "counts" in e) <= H.MAX_ROWS_WIDE, key
        for step, op in enumerate(ops):  # the kinds that take a program, and those of them that got a list or sparse leaf
            if programs_of(op):
                tagged.setdefault(op["op"], None)
                if tagged[op["op"]] is None and pooled_leaf(op):
                    tagged[op["op"]] = (key[0], step)
        print(f"history {H.history_tag(*key)}: {len(ops)} steps")
    for name in WIDE_WANTED:
        if name in where:
            print(f"condition {name}: seed {where[name][0]}, step {where[name][1]}")
    missing = [name for name in WIDE_WANTED if name not in where]
    assert not missing, f"coverage conditions never met: {missing}"
    assert len(H.WIDE_PAIRS) == 16 * 29 - 8 * 19 and len(H.WIDE) == 12
    # the new program kinds go into every program-taking op, old kinds included
    for kind, at in sorted(tagged.items()):
        print(f"a list or sparse leaf in {kind}: " + ("never" if at is None else f"seed {at[0]}, step {at[1]}"))
    assert set(PROGRAM_TAKING) <= set(tagged) and not [kind for kind, at in tagged.items() if at is None], tagged
    # the large ones move the inner search between the routes by `auto` alone: exact, filter, exact after the compaction, filter
    for key in H.WIDE_LARGE:
        ops, expected = H.make_history(*key)
        st = wide_trace(ops, expected, key[1])
        assert all(s["strategy"] == "auto" for s in st)
        for kind in ("search_mmr", "search_like", "search_grouped"):
            routes = [s["total"] >= H.FILTER_MIN_ROWS for op, s in zip(ops, st) if op["op"] == kind and
                      (len(op["groups"]) if kind == "search_like" else op["nq"]) >= 12]
            assert True in routes and False in routes[routes.index(True):] and routes[-1] is True, (key, kind, routes)
        each = [(op["nq"], s["total"] >= H.FILTER_MIN_ROWS, any(list_leaf({"programs": op["programs"]}, H.LIST_A) for _ in [0]))
                for op, s in zip(ops, st) if op["op"] == "search_each"]
        assert {(12, True, True), (40, True, True)} <= set(each), each
        kinds = {op["op"] for op in ops}
        assert {"search_mmr", "search_like", "search_grouped", "search_maxsim", "search_each", "tombstone_where", "compact"} <= kinds
        assert sum(op["op"] in H.WIDE_QUERIES for op in ops) <= 20
        i = [op["op"] for op in ops].index("tombstone_where")
        died = expected[i]["counts"][1] / expected[i]["counts"][0]
        assert 0.25 < died < 0.42, died
        print(f"history {H.history_tag(*key)}: {len(ops)} steps, tombstone_where of {died:.0%} of the rows at step {i}")


def test_pool_capacity_after_mirrors_list_pool_reserve():
    assert H.pool_capacity_after(0, 0) == 0 and H.pool_capacity_after(0, 1) == 1024 and H.pool_capacity_after(1024, 1024) == 1024
    assert H.pool_capacity_after(1024, 1025) == 2048 and H.pool_capacity_after(2048, 9000) == 9000
    assert H.pool_capacity_after(700, 701) == 1400  # after a repack the capacity is the live sum, whatever it is
    m = H.WideHistoryModel(4, "l2")
    m.define_attr(4, "int64_list")
    m.append(np.zeros((600, 4), np.float32))
    lists = H.csr([[1, 2, 3]] * 600)
    m.set_attr_list(4, 0, lists)
    assert m.pools()[4] == (1800, 1800, 1800)
    m.set_attr_list(4, 0, lists)
    assert m.pools()[4] == (3600, 3600, 1800)
    m.compact()
    assert m.pools()[4] == (1800, 1800, 1800)
    m.reset()
    assert m.pools()[4] == (0, 1800, 0)


# ---------------------------------------------------------------- sensitivity of the wide histories: five seeded defects
def _differs(a, b):
    return any((x is None) != (y is None) or (x is not None and np.asarray(x).tobytes() != np.asarray(y).tobytes()) for x, y in zip(a, b))


def reads_pooled(op):
    return op["op"] in H.LIST_READERS + ("get_attr_list",) or any(
        o[1] in H.POOLED and o[0] not in (W.AND, W.OR, W.NOT, W.TRUE) for p in programs_of(op) for o in p["ops"])


class KeepsListsInOldRowOrder(H.WideHistoryModel):
    """Lists and sparse vectors stay in pre-compaction row order while the scalar columns move."""
    fired = None
    seen_by = staticmethod(reads_pooled)
    at_once = False

    def compact(self):
        lists = {a: list(rows) for a, rows in self._lists.items()}
        lengths = {a: self._cols[a].copy() for a in self._lists}
        old = super().compact()
        for a in lists:
            if self.fired is None and lists[a][:old.size] != self._lists[a]:
                self.fired = self.step
            self._lists[a], self._cols[a] = lists[a][:old.size], lengths[a][:old.size]
        return old


class ListsSurviveReset(H.WideHistoryModel):
    """``reset`` leaves the lists where they were: freshly appended rows inherit them."""
    fired = None
    seen_by = staticmethod(reads_pooled)
    at_once = False
    _left = None

    def reset(self, space=None):
        self._left = {a: list(rows) for a, rows in self._lists.items()}
        super().reset(space)

    def append(self, rows):
        first = super().append(rows)
        for a, left in (self._left or {}).items():
            for row in range(first, min(self._rows.shape[0], len(left))):
                if left[row] is not None:
                    self._put(a, row, left[row])
                    if self.fired is None:
                        self.fired = self.step
        self._left = None
        return first


class InnerSearchMissesFilteredDeletes(H.WideHistoryModel):
    """``search_mmr`` and ``search_like`` do not see the rows ``tombstone_where`` deleted (until a compaction drops them)."""
    fired = None
    seen_by = staticmethod(lambda op: op["op"] in ("search_mmr", "search_like"))
    at_once = True
    _ghosts = None

    def tombstone_where(self, program):
        labels = super().tombstone_where(program)
        self._ghosts = labels if self._ghosts is None else np.union1d(self._ghosts, labels)
        return labels

    def compact(self):
        self._ghosts = None
        return super().compact()

    def reset(self, space=None):
        self._ghosts = None
        super().reset(space)

    def _haunted(self, name, *a, **kw):
        right = getattr(super(), name)(*a, **kw)
        if self._ghosts is None or not self._ghosts.size:
            return right
        keep = self._deleted.copy()
        self._deleted[self._ghosts] = False
        try:
            wrong = getattr(super(), name)(*a, **kw)
        finally:
            self._deleted = keep
        if self.fired is None and _differs(right, wrong):
            self.fired = self.step
        return wrong

    def search_mmr(self, *a, **kw):
        return self._haunted("search_mmr", *a, **kw)

    def search_like(self, *a, **kw):
        return self._haunted("search_like", *a, **kw)


class AppliesARefusedUpdate(H.WideHistoryModel):
    """``update_where`` writes what it can although ``refused > 0``."""
    fired = None
    seen_by = staticmethod(lambda op: op["op"] == "get_attr")
    at_once = False

    def update_where(self, program, assigns):
        hit = self.match(program)
        matched, refused = super().update_where(program, assigns)
        if refused:
            for attr, op, a in assigns:
                col = self._cols[attr]
                if op == H._native.SET_ASSIGN:
                    col.view(np.int64)[hit] = a
                elif col.dtype == np.int64:
                    rows = hit & (col != W.INT64_ABSENT)
                    with np.errstate(over="ignore"):
                        col[rows] = col[rows] + np.int64(a)
            if self.fired is None:
                self.fired = self.step
        return matched, refused


class MaxsimReadsTheOldDocumentColumn(H.WideHistoryModel):
    """``search_maxsim`` is answered from the document column as it was before the last ``update_where``."""
    fired = None
    seen_by = staticmethod(lambda op: op["op"] == "search_maxsim")
    at_once = True
    _before = None

    def update_where(self, program, assigns):
        self._before = {a: col.copy() for a, col in self._cols.items()}
        return super().update_where(program, assigns)

    def search_maxsim(self, tokens, offsets, k, attr, where=None, want_matches=False):
        right = super().search_maxsim(tokens, offsets, k, attr, where, want_matches)
        old = (self._before or {}).get(attr)
        if old is None or old.size != self._cols[attr].size:
            return right
        keep = self._cols[attr]
        self._cols[attr] = old
        try:
            wrong = super().search_maxsim(tokens, offsets, k, attr, where, want_matches)
        finally:
            self._cols[attr] = keep
        if self.fired is None and _differs(right, wrong):
            self.fired = self.step
        return wrong


@pytest.mark.parametrize("defect", [KeepsListsInOldRowOrder, ListsSurviveReset, InnerSearchMissesFilteredDeletes,
                                    AppliesARefusedUpdate, MaxsimReadsTheOldDocumentColumn])
def test_the_driver_reports_a_seeded_defect_in_the_wide_histories(defect, tmp_path, monkeypatch):
    from tests import conftest

    monkeypatch.setattr(conftest, "OUT_DIR", tmp_path)
    reported, real_call = 0, H.call
    for key in H.WIDE[:4]:
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
            assert engine.fired is not None and defect.seen_by(ops[failed]), (engine.fired, failed, ops[failed])
            if defect.at_once:  # `fired` is the first call whose answer the defect changes: that call is the one reported
                assert failed == engine.fired, (failed, engine.fired)
            else:               # the state breaks in a mutation; the first later call that reads it differently reports it
                assert failed > engine.fired and ops[engine.fired]["op"] in H.WIDE_MUTATIONS, (failed, engine.fired)
            dumped = json.loads((tmp_path / f"history_{tag}.json").read_text())
            assert dumped["failed_step"] == failed and dumped["ops"] == ops[:failed + 1]
            print(f"{defect.__name__}: {tag} fired at step {engine.fired}, reported at step {failed} ({ops[failed]['op']})")
            reported += 1
        else:
            assert engine.fired is None or not defect.at_once, f"{tag}: fired at step {engine.fired}, never reported"
        monkeypatch.setattr(H, "call", real_call)
    assert reported >= 2, f"{defect.__name__}: reported in {reported} of 4 histories"




# ================================================================ the recent histories: bits, geo, stats and hybrid on one handle
from mlvectordb_amd import _native  # noqa: E402
from mlvectordb_amd.engine import StatsOverflow  # noqa: E402
from tests import geo_helpers as GH  # noqa: E402
from tests import history_recent_helpers as R  # noqa: E402

GEO_OPS = (W.GEO_BOX, W.GEO_RADIUS)


def leaf_on(op, attr, kinds):
    return any(o[0] in kinds and o[1] == attr for p in R.programs_of(op) for o in p["ops"])


def test_the_recent_model_agrees_with_the_oracle_engines_it_is_composed_from():
    """The same state -- two appends, every column valued, tombstones -- in ``RecentHistoryModel`` and in the bits, hybrid,
    statistics and geo oracle engines; one call per new entry with a program, then what the model adds: the bits pool
    mirrored, one ``match`` for list, geo and bits leaves together, the refusals with the status the headers name."""
    from tests.bits_helpers import BitsOracleEngine
    from tests.hybrid_helpers import HybridOracleEngine
    from tests.sparse_helpers import random_corpus, sparse_csr
    from tests.stats_helpers import StatsOracleEngine

    rng = np.random.default_rng(11)
    d, n = 12, 400
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((5, d), dtype=np.float32)
    centre = R.CENTRES[0]
    points = R.geo_values(np.random.default_rng(12), n, centre)
    codes = R.bits_column(np.random.default_rng(13), n, R.WORDS, 0.1)
    short = R.bits_column(np.random.default_rng(14), 50, R.WORDS_FEW, 0.0)
    short_at = np.arange(0, 100, 2, dtype=np.int64)
    lists = H.csr(H.wide_lists(np.random.default_rng(4), n))
    vectors = sparse_csr(random_corpus(np.random.default_rng(5), n, H.SPARSE_VOCAB, True))
    engines = [cls(d, "l2") for cls in (R.RecentHistoryModel, BitsOracleEngine, HybridOracleEngine, StatsOracleEngine,
                                        GH.oracle_engine_class())]
    model, bits, hybrid, stats, geo = engines
    for e in engines:
        pooled, is_bits, is_geo = isinstance(e, HybridOracleEngine), isinstance(e, BitsOracleEngine), e in (model, geo)
        columns = ((0, "int64"), (1, "float64"), (2, "int64")) + (((4, "int64_list"), (5, "sparse")) if pooled else ()) \
            + (((R.GEO_A, "geo"),) if is_geo else ()) + (((R.BITS_A, "bits"),) if is_bits else ())
        for attr, kind in columns:
            e.define_attr(attr, kind)
        e.append(rows[:250])
        e.append(rows[250:])
        for attr in range(3):
            e.set_attr(attr, 0, H.column_values(attr, n, np.random.default_rng(attr), n))
        if pooled:
            e.set_attr_list(4, 0, lists)
            e.set_attr_sparse(5, 0, vectors)
        if is_geo:
            e.set_attr(R.GEO_A, 0, points)
        if is_bits:
            e.bits_set(R.BITS_A, 0, codes)
        e.tombstone(np.arange(0, n, 7))
        if is_bits:
            assert e.bits_set_at(R.BITS_A, short_at, short) == 50 - 8  # (eight of the labels are tombstoned)
    half = H.program_of({"ops": HALF, "set": []})
    same = lambda a, b: len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))  # noqa: E731
    # bits
    coded = H.program_of({"ops": [[W.EXISTS, R.BITS_A, 0, 0], [W.LT, 2, 8, 0], [W.AND, 0, 0, 0]], "set": []})
    for words in (R.WORDS, R.WORDS_FEW):
        bq = R.bits_codes(np.random.default_rng(15), 4, words)
        for metric in ("hamming", "jaccard"):
            got, want = model.search_bits(R.BITS_A, bq, 9, metric, coded), bits.search_bits(R.BITS_A, bq, 9, metric, coded)
            assert same(got, want) and got[2].min() > 0
    assert same(model.bits_get(R.BITS_A, 0, n), bits.bits_get(R.BITS_A, 0, n))
    assert model.list_stats(R.BITS_A) == bits.list_stats(R.BITS_A)
    # hybrid: the entry's seven outputs, and behind them the whole union
    sq = H._sparse_queries(np.random.default_rng(6), 5)
    for method in ("rrf", "linear", "relative"):
        got = model.search_hybrid(qs, 5, sq, 10, 40, 20, method=method, weights=(0.75, 1.3), rrf_k=7.5, where=half)
        want = hybrid.search_hybrid(qs, 5, sq, 10, 40, 20, method=method, weights=(0.75, 1.3), rrf_k=7.5, where=half, components=True)
        assert same(got[:7], want)
        union = hybrid.search_hybrid(qs, 5, sq, 60, 40, 20, method=method, weights=(0.75, 1.3), rrf_k=7.5, where=half, components=True)
        assert same(got[7], union) and (union[2] > 40).all()
    # statistics
    for attr, by in ((1, 0), (0, None), (2, 2)):
        assert same(model.attr_stats(attr, by, 4096, half), stats.attr_stats(attr, by, 4096, half))
    for e in (model, stats):
        with pytest.raises(StatsOverflow) as err:
            e.attr_stats(1, 2, 3, half)
        assert (err.value.matched, err.value.by_absent) == (model.where_count(half), 0) and err.value.n_groups > 3
    # geo: a radius leaf AND-ed with a scalar one, a box, nearest under a program
    c = int(GH.quantise([centre[0]], [centre[1]])[0])
    near = GH.radius_program(R.GEO_A, c, 3.0e4)
    both = W.Program(np.concatenate([near.ops, half.ops, np.array([(W.AND, 0, 0, 0)], W.OP_DTYPE)]), near.set)
    box = GH.box_program(R.GEO_A, *GH.quantise([centre[0] - 5, centre[0] + 5], [179.5, -179.5]))
    for program in (near, both, box, GH.negate(near)):
        assert np.array_equal(model.match(program), geo.match(program)) and model.match(program).any()
    got, want = model.geo_nearest(R.GEO_A, c, 20, both, 3), geo.geo_nearest(R.GEO_A, c, 20, both, 3)
    assert same(got[:2], want[:2]) and np.array_equal(got[2].astype(np.float64), want[2]) and got[3:] == want[3:]
    assert got[2].dtype == GH.LD and got[0].size == 20
    # what the model adds: list, geo and bits leaves in one program
    mixed = H.program_of({"ops": [[W.HAS, 4, 3, 0], [W.EXISTS, R.BITS_A, 0, 0], [W.AND, 0, 0, 0]] + [list(map(int, o)) for o in near.ops.tolist()]
                          + [[W.OR, 0, 0, 0]], "set": []})
    want = (hybrid.match(H.program_of({"ops": [[W.HAS, 4, 3, 0]], "set": []}))
            & bits.match(H.program_of({"ops": [[W.EXISTS, R.BITS_A, 0, 0]], "set": []}))) | geo.match(near)
    assert np.array_equal(model.match(mixed), want) and 0 < want.sum() < model.counts()[0] - model.counts()[1]
    # ... the bits pool mirrored as a list's, through the repack and the reset
    used, cap, live = model.pools()[R.BITS_A]
    assert used == R.WORDS * int(codes.present.sum()) + R.WORDS_FEW * 50 and cap == H.pool_capacity_after(R.WORDS * int(codes.present.sum()), used)
    assert 0 < live < used
    assert np.array_equal(model.compact(), bits.compact()) and model.list_stats(R.BITS_A) == bits.list_stats(R.BITS_A)
    assert model.pools()[R.BITS_A] == (live, live, live)
    assert same(model.bits_get(R.BITS_A, 0, 300), bits.bits_get(R.BITS_A, 0, 300))
    model.reset()
    assert model.pools()[R.BITS_A] == (0, live, 0) and model.append(rows[:5]) == 0
    assert not model.bits_get(R.BITS_A, 0, 5)[0].any() and (model.get_attr(R.GEO_A, 0, 5) == GH.ABSENT).all()
    # ... and the refusals, with the status codes the headers name, none of which changes the state
    before = (model.get_attr(R.GEO_A, 0, 5).copy(), model.pools())
    a = {"qs": qs[:3], "sq": H._sparse_queries(np.random.default_rng(7), 3), "bq": R.bits_codes(rng, 2, R.WORDS)}
    for which in R.RECENT_REFUSALS:
        op = {"op": "refuse_recent", "which": which, "seed": 1, "centre": c}
        if which.startswith("bits_words") or which == "bits_at_repeat":
            a["col"] = R.materialise(model, op)["col"]
        assert R.CALLS["refuse_recent"](model, op, a) == ("refused", 6 if which in R.UNSUPPORTED_REFUSALS else 1), which
    assert np.array_equal(model.get_attr(R.GEO_A, 0, 5), before[0]) and model.pools() == before[1]


def recent_trace(ops, expected, space):
    """The handle's state BEFORE each step of a recent history.  ``shadow`` counts what resets the derived row shadows (a
    compaction that drops rows, a reset, an append that regrows the capacity); ``regrowths`` the capacity regrowths while the
    sparse, geo and bits columns hold values."""
    st = dict(strategy="auto", total=0, deleted=0, space=space, cap=0, regrowths=0, valued=set(), pools={}, shadow=0)
    out = []
    for op, exp in zip(ops, expected):
        out.append({**st, "valued": set(st["valued"])})
        kind = op["op"]
        if kind == "set_strategy":
            st["strategy"] = op["strategy"]
        elif kind == "append":
            cap = H.capacity_after(st["cap"], st["total"] + op["n"])
            if cap != st["cap"] and st["cap"]:
                st["shadow"] += 1
                if {H.SPARSE_A, R.GEO_A, R.BITS_A} <= st["valued"]:
                    st["regrowths"] += 1
            st["cap"] = cap
        elif kind == "compact":
            st["cap"] = H.capacity_after_compact(st["cap"], st["total"] - st["deleted"], st["deleted"])
            st["regrowths"] = 0
            st["shadow"] += bool(st["deleted"])
        elif kind in ("set_attr_sparse", "bits_set", "set_attr") and op["n"] and op["attr"] in (H.SPARSE_A, R.GEO_A, R.BITS_A):
            st["valued"] = st["valued"] | {op["attr"]}
        elif kind == "reset":
            st.update(regrowths=0, valued=set(), shadow=st["shadow"] + 1)
            st["space"] = op["space"] or st["space"]
        if "counts" in exp:
            st["total"], st["deleted"] = exp["counts"]
        st["pools"] = exp["pools"]
    return out


def answers_nothing(op, want):
    """A new query on an index without rows: padding or zeros."""
    kind = op["op"]
    if kind in ("search_bits", "search_hybrid"):
        return not np.asarray(want[2]).any() and (want[0] == -1).all()
    if kind == "bits_get":
        return want[0].size == 0 and want[1].size == 0
    if kind == "attr_stats":
        return tuple(want[7:]) == (0, 0) and not want[1].any()
    return want[0].size == 0 and tuple(want[3:]) == (0, 0)  # geo_nearest


def recent_conditions(ops, expected, space):
    """{condition: step} for every condition of RECENT_WANTED this recent history meets."""
    st = recent_trace(ops, expected, space)
    kinds = [op["op"] for op in ops]
    n = len(ops)
    met = {}
    grow, floor = 0, np.inf
    late = dict(defined=False, written=set())
    mutations = [m for m in R.RECENT_MUTATIONS if m not in ("set_strategy", "set_tuning")]
    full = lambda o: o["offset"] + o["limit"] == R.ORDER_MAX_ROWS  # noqa: E731
    one = lambda o: o["limit"] == 1  # noqa: E731

    def put(name, step):
        met.setdefault(name, step)

    for i, op in enumerate(ops):
        k = kinds[i]
        nxt = kinds[i + 1] if i + 1 < n else None
        after = ops[i + 1] if i + 1 < n else {}
        s = st[i]
        # pairs: either side is new
        if k in R.RECENT_MUTATIONS and nxt in R.RECENT_QUERIES and (k in R.BITS_MUTATIONS or nxt in R.RECENT_NEW_QUERIES):
            put(f"k_{k}>{nxt}", i)
        # the bits pool: a compaction with garbage, then search_bits and list_stats
        if k == "compact" and i + 2 < n and R.BITS_A in s["pools"]:
            used, _, live = s["pools"][R.BITS_A]
            if used > live > 0 and nxt == "search_bits" and after["attr"] == R.BITS_A and kinds[i + 2] == "list_stats" \
                    and ops[i + 2]["attr"] == R.BITS_A:
                assert expected[i + 2]["want"][0] == expected[i + 2]["want"][1] > 0  # the repack: used == live
                put(f"l_bits_{'dead' if s['deleted'] else 'clean'}", i)
        # ... its capacity grows twice while it holds live codes, then rows written before the first growth are read
        if k in ("compact", "reset"):
            grow, floor = 0, np.inf
        if k in R.BITS_MUTATIONS and op["attr"] == R.BITS_A:
            used, cap, live = s["pools"][R.BITS_A]
            if expected[i]["pools"][R.BITS_A][1] != cap:
                assert expected[i]["pools"][R.BITS_A][1] == H.pool_capacity_after(cap, expected[i]["pools"][R.BITS_A][0])
                if used > 0 and live > 0:
                    grow += 1
            if grow:
                floor = min(floor, write_floor(op))
        if k == "bits_get" and op["attr"] == R.BITS_A and op["first"] == 0 and 0 < op["n"] <= floor and grow >= 2:
            put("m_bits", i)
        # width: rows of 5 words rewritten with 2 words (or made absent), then a 5-word and a 2-word search
        if k == "bits_set_at" and op["attr"] == R.BITS_A and op["words"] == R.WORDS_FEW and op["p_absent"] in (0.0, 1.0) \
                and set(expected[i]["widths_before"]) == {R.WORDS} and kinds[i + 1:i + 3] == ["search_bits", "search_bits"] \
                and [ops[i + 1]["words"], ops[i + 2]["words"]] == [R.WORDS, R.WORDS_FEW]:
            put("width_2" if op["p_absent"] == 0.0 else "width_absent", i)
        # two regrowths of the rows with values present, then the readers
        if s["regrowths"] >= 2:
            if k in ("bits_get", "search_bits", "geo_nearest", "search_hybrid"):
                put("n_" + k, i)
            if leaf_on(op, R.GEO_A, GEO_OPS):
                put("n_geo_program", i)
            if k == "attr_stats" and op["by"] is not None:
                put("n_attr_stats_by", i)
        # emptied: the five new queries answer padding or zeros, a refill, the five again
        emptied_by_compact = (k == "compact" and s["total"] > 0 and expected[i]["counts"] == (0, 0) and i > 0
                              and kinds[i - 1] == "tombstone_where" and ops[i - 1]["program"]["ops"] == [[W.TRUE, 0, 0, 0]])
        if emptied_by_compact or (k == "reset" and s["total"] > 0):
            first, j = run_of(ops, i + 1, R.RECENT_QUERIES)
            if j < n and kinds[j] == "append":  # rows, the five, the values of every column, the five again
                bare, j2 = run_of(ops, j + 1, R.RECENT_QUERIES)
                values, j3 = run_of(ops, j2, R.RECENT_MUTATIONS)
                again, _ = run_of(ops, j3, R.RECENT_QUERIES)
                new = [x for x in first if kinds[x] in R.RECENT_NEW_QUERIES]
                written = {(kinds[x], ops[x].get("attr")) for x in values}
                if all(answers_nothing(ops[x], expected[x]["want"]) for x in new) and set(R.RECENT_NEW_QUERIES) <= {kinds[x] for x in new} \
                        and set(R.RECENT_NEW_QUERIES) <= {kinds[x] for x in bare} and set(R.RECENT_NEW_QUERIES) <= {kinds[x] for x in again} \
                        and {("bits_set", R.BITS_A), ("set_attr", R.GEO_A), ("set_attr_sparse", H.SPARSE_A)} <= written:
                    put("w_compact" if k == "compact" else "w_reset" if op["space"] is None else "w_reset_other", i)
        # hybrid on the filter route across mutations
        if k == "search_hybrid" and s["strategy"] == "filter":
            between, j = run_of(ops, i + 1, mutations)
            if between and j < n and kinds[j] == "search_hybrid" and st[j]["strategy"] == "filter":
                small = op["fd"] <= 64 and ops[j]["fd"] <= 64
                big = op["fd"] > 64 and ops[j]["fd"] > 64
                for x in between:
                    if small and kinds[x] in ("tombstone_where", "tombstone", "append", "compact"):
                        put(f"p_hybrid_small_{kinds[x]}", i)
                    if big and st[j]["shadow"] > s["shadow"]:  # the fp16 shadow was dropped in between
                        if kinds[x] == "compact" and st[x]["deleted"]:
                            put("p_hybrid_big_compact", i)
                        if kinds[x] == "append" and st[x + 1]["cap"] != st[x]["cap"] and st[x]["cap"]:
                            put("p_hybrid_big_regrowth", i)
            if s["space"] == "l2" and i + 3 < n and nxt == "search_hybrid" and after["nq"] != op["nq"] \
                    and kinds[i + 2] == "tombstone_where" and kinds[i + 3] in SEARCHES:
                put("p_l2_hybrid", i)
        # the mask is handed back
        if k in ("search_hybrid", "search_bits") and op.get("program") is not None:
            if nxt == "search64":
                put(f"q_{k}_plain", i)
            if nxt == k and after.get("program") is None:
                put(f"q_{k}_own", i)
        # one workspace, two windows
        if {k, nxt} == {"where_ordered", "geo_nearest"} and ((full(op) and one(after)) or (one(op) and full(after))):
            put("ws_ordered>nearest" if k == "where_ordered" else "ws_nearest>ordered", i)
        # the grow-only table of the statistics
        if k == "attr_stats" and op["by"] is not None and kinds[i + 1:i + 4] == ["attr_stats"] * 3 and not isinstance(expected[i]["want"][0], str):
            groups = int(expected[i]["want"][0].size)
            a, b, c = ops[i + 1:i + 4]
            wa, wb, wc = (expected[x]["want"] for x in (i + 1, i + 2, i + 3))
            if op["max_groups"] > 8 * groups and all(o["by"] == op["by"] and o.get("program") is None for o in (op, a, b, c)) \
                    and a["max_groups"] == groups and not isinstance(wa[0], str) and wa[0].size == groups \
                    and b["max_groups"] == groups - 1 and tuple(wb) == ("overflow", True) + tuple(wa[7:]) \
                    and not isinstance(wc[0], str):
                put("g_chain", i)
        if k == "attr_stats" and nxt == "facet_values" and after["attr"] == op["by"]:
            put("g_stats>facet", i)
        if k == "facet_values" and nxt == "attr_stats" and after["by"] == op["attr"]:
            put("g_facet>stats", i)
        # writers, then at once the readers of what they wrote
        if k == "update_where":
            if [R.GEO_A, _native.SET_ASSIGN] in [x[:2] for x in op["assigns"]]:
                if nxt == "geo_nearest" and after["attr"] == R.GEO_A:
                    put("s_geo_assign>geo_nearest", i)
                if leaf_on(after, R.GEO_A, (W.GEO_RADIUS,)):
                    put("s_geo_assign>radius", i)
            if [1, _native.SET_ADD] in [x[:2] for x in op["assigns"]] and nxt == "attr_stats" and after["attr"] == 1:
                put("s_float_add>attr_stats", i)
        if k == "set_attr_at" and nxt == "attr_stats" and after["by"] == op["attr"]:
            put("s_by>attr_stats", i)
        if k == "set_attr_sparse_at" and nxt == "search_hybrid" and after["attr"] == op["attr"]:
            put("s_sparse_at>search_hybrid", i)
        if k == "bits_set_at" and 0 < expected[i]["dead"] and expected[i]["want"] < len(expected[i]["widths_before"]) \
                and nxt == "search_bits" and after["attr"] == op["attr"]:
            put("s_bits_at_dead>search_bits", i)
        if k == "tombstone_where" and leaf_on(op, R.GEO_A, (W.GEO_RADIUS,)) and nxt in ("attr_stats", "geo_nearest", "search_bits"):
            put(f"s_tombstone_radius>{nxt}", i)
        # the late columns: all absent, then written
        if k == "define_attr" and op["attr"] == R.LATE_GEO and s["total"] > 0 and not late["defined"]:
            late["defined"] = True
            put("r_defined", i)
        elif late["defined"]:
            if (k in ("set_attr", "set_attr_at", "bits_set", "bits_set_at") and op["attr"] in (R.LATE_GEO, R.LATE_BITS)) or \
                    (k == "update_where" and R.LATE_GEO in [x[0] for x in op["assigns"]]):
                late["written"].add(R.LATE_GEO if k in ("set_attr", "set_attr_at", "update_where") else R.LATE_BITS)
            phase = {0: "absent", 2: "set"}.get(len(late["written"]))
            if phase:
                if k == "geo_nearest" and op["attr"] == R.LATE_GEO:
                    put(f"r_{phase}_geo_nearest", i)
                if leaf_on(op, R.LATE_GEO, GEO_OPS):
                    put(f"r_{phase}_geo_leaf", i)
                if k in ("search_bits", "bits_get") and op["attr"] == R.LATE_BITS:
                    put(f"r_{phase}_{k}", i)
        # refusals with the status the header names, the pools as they were, each followed at once by a query
        if k == "refuse_recent" and nxt in R.RECENT_QUERIES and expected[i]["pools"] == s["pools"] and \
                expected[i]["want"] == ("refused", 6 if op["which"] in R.UNSUPPORTED_REFUSALS else 1):
            put("v_" + op["which"], i)
    for name, parts in (("n", ["n_bits_get", "n_search_bits", "n_geo_nearest", "n_geo_program", "n_attr_stats_by", "n_search_hybrid"]),
                        ("r", ["r_defined"] + [f"r_{p}_{x}" for p in ("absent", "set") for x in
                                               ("geo_nearest", "geo_leaf", "search_bits", "bits_get")])):
        if all(x in met for x in parts):
            met[name] = met[parts[0]]
    return met


RECENT_WANTED = ([f"k_{m}>{q}" for m, q in R.RECENT_PAIRS] + ["l_bits_clean", "l_bits_dead", "m_bits", "width_2", "width_absent", "n",
                                                               "w_reset", "w_reset_other", "w_compact"]
                 + [f"p_hybrid_small_{x}" for x in ("tombstone_where", "tombstone", "append", "compact")]
                 + ["p_hybrid_big_compact", "p_hybrid_big_regrowth", "p_l2_hybrid"]
                 + [f"q_{k}_{x}" for k in ("search_hybrid", "search_bits") for x in ("plain", "own")]
                 + ["ws_ordered>nearest", "ws_nearest>ordered", "g_chain", "g_stats>facet", "g_facet>stats"]
                 + ["s_geo_assign>geo_nearest", "s_geo_assign>radius", "s_by>attr_stats", "s_float_add>attr_stats",
                    "s_sparse_at>search_hybrid", "s_bits_at_dead>search_bits"]
                 + [f"s_tombstone_radius>{q}" for q in ("attr_stats", "geo_nearest", "search_bits")] + ["r"]
                 + ["v_" + w for w in R.RECENT_REFUSALS])


def test_the_recent_histories_meet_every_coverage_condition():
    where, tagged = {}, {}
    for key in R.RECENT:
        ops, expected = H.make_history(*key)
        for name, step in recent_conditions(ops, expected, key[1]).items():
            where.setdefault(name, (key[0], step))
        assert max(e["counts"][0] for e in expected if "counts" in e) <= H.MAX_ROWS_WIDE, key
        for step, op in enumerate(ops):  # the kinds that take a program, and those of them that got a geo leaf or EXISTS on bits
            if R.programs_of(op):
                tagged.setdefault(op["op"], None)
                if tagged[op["op"]] is None and any(R.has_recent_leaf(p) for p in R.programs_of(op)):
                    tagged[op["op"]] = (key[0], step)
        print(f"history {H.history_tag(*key)}: {len(ops)} steps, distance bar {R.geo_bar(*key):.3e}")
    for name in RECENT_WANTED:
        if name in where:
            print(f"condition {name}: seed {where[name][0]}, step {where[name][1]}")
    missing = [name for name in RECENT_WANTED if name not in where]
    assert not missing, f"coverage conditions never met: {missing}"
    assert len(R.RECENT_PAIRS) == 18 * 34 - 16 * 29 and len(R.RECENT) == 12 and len(set(RECENT_WANTED)) == len(RECENT_WANTED)
    # the new program kinds go into every program-taking op, old kinds included; and every one of the six kinds is drawn
    for kind, at in sorted(tagged.items()):
        print(f"a geo leaf or EXISTS on the bits column in {kind}: " + ("never" if at is None else f"seed {at[0]}, step {at[1]}"))
    assert set(R.PROGRAM_TAKING) <= set(tagged) and not [kind for kind, at in tagged.items() if at is None], tagged
    shapes = set()
    for key in R.RECENT:
        for op in H.make_history(*key)[0]:
            for p in R.programs_of(op):
                codes = [o[0] for o in p["ops"]]
                box = [o for o in p["ops"] if o[0] == W.GEO_BOX]
                shapes |= {"radius"} if codes == [W.GEO_RADIUS] else {"not_radius"} if codes == [W.GEO_RADIUS, W.NOT] else set()
                shapes |= {"geo_and_scalar"} if codes == [W.GEO_RADIUS, W.LT, W.AND] else set()
                shapes |= {"bits_exists"} if [o[:2] for o in p["ops"]] == [[W.EXISTS, R.BITS_A]] else set()
                for o in box:
                    (_, w), (_, e) = GH.unpack(np.int64(o[2])), GH.unpack(np.int64(o[3]))
                    shapes.add("box" if w <= e else "box_anti")
    assert shapes == set(R.RECENT_PROGRAMS), shapes
    # the large ones move hybrid's dense leg between the routes by `auto` alone, with the paged depths on each side
    for key in R.RECENT_LARGE:
        ops, expected = H.make_history(*key)
        st = recent_trace(ops, expected, key[1])
        assert all(s["strategy"] == "auto" for s in st)
        hybrid = [(op, s["total"] >= H.FILTER_MIN_ROWS) for op, s in zip(ops, st) if op["op"] == "search_hybrid"]
        routes = [above for op, above in hybrid if op["nq"] >= 12 and op["fd"] <= 64]
        assert routes[0] is False and True in routes and False in routes[routes.index(True):] and routes[-1] is True, (key, routes)
        assert {(12, True), (40, True)} <= {(op["nq"], above) for op, above in hybrid if op["fd"] <= 64}
        for fd in (65, 1024):
            assert {above for op, above in hybrid if op["fd"] == fd} == {True, False}, (key, fd)
        new = [(op["op"], s["total"] >= H.FILTER_MIN_ROWS) for op, s in zip(ops, st) if op["op"] in R.RECENT_NEW_QUERIES]
        assert len(new) <= 20 and {(q, True) for q in R.RECENT_NEW_QUERIES} <= set(new), new
        i = [op["op"] for op in ops].index("tombstone_where")
        assert [o[0] for o in ops[i]["program"]["ops"]] == [W.GEO_BOX] and "compact" in [op["op"] for op in ops[i:]]
        died = expected[i]["counts"][1] / expected[i]["counts"][0]
        assert 0.25 < died < 0.42, died
        assert max(e["counts"][0] for e in expected if "counts" in e) > H.FILTER_MIN_ROWS
        print(f"history {H.history_tag(*key)}: {len(ops)} steps, tombstone_where through a geo box of {died:.0%} of the rows at "
              f"step {i}, distance bar {R.geo_bar(*key):.3e}")


def test_the_recent_op_lists_are_deterministic_and_json_serialisable():
    key = R.RECENT[1]
    ops, expected = H.make_history(*key)
    again = H._history.__wrapped__(*key)  # (generated anew; the cache keeps what the other tests share)
    ops2, expected2 = again.ops, again.expected
    assert ops2 is not ops and json.dumps(ops) == json.dumps(ops2) and json.loads(json.dumps(ops)) == ops
    for a, b in zip(expected, expected2):
        assert a["args"].keys() == b["args"].keys()
        for name, x in a["args"].items():
            if isinstance(x, np.ndarray):
                assert x.tobytes() == b["args"][name].tobytes(), name
    other, _ = H.make_history(key[0] + 1, *key[1:])
    assert json.dumps(other) != json.dumps(ops)


# ---------------------------------------------------------------- sensitivity of the recent histories: six seeded defects
def reads_bits(op):
    return op["op"] in ("search_bits", "bits_get") or (op["op"] == "list_stats" and op["attr"] in R.BITS_COLUMNS) or any(
        leaf_on(op, a, (W.EXISTS,)) for a in R.BITS_COLUMNS)


class KeepsCodesInOldRowOrder(R.RecentHistoryModel):
    """Bit codes stay in pre-compaction row order while the scalar columns move."""
    fired = None
    seen_by = staticmethod(reads_bits)
    at_once = False

    def compact(self):
        codes = {a: list(self._lists[a]) for a in self._bits}
        lengths = {a: self._cols[a].copy() for a in self._bits}
        old = super().compact()
        for a in codes:
            if self.fired is None and codes[a][:old.size] != self._lists[a]:
                self.fired = self.step
            self._lists[a], self._cols[a] = codes[a][:old.size], lengths[a][:old.size]
        return old


class CodesSurviveReset(R.RecentHistoryModel):
    """``reset`` leaves the codes where they were: freshly appended rows inherit them."""
    fired = None
    seen_by = staticmethod(reads_bits)
    at_once = False
    _left = None

    def reset(self, space=None):
        self._left = {a: list(self._lists[a]) for a in self._bits}
        super().reset(space)

    def append(self, rows):
        first = super().append(rows)
        for a, left in (self._left or {}).items():
            for row in range(first, min(self._rows.shape[0], len(left))):
                if left[row] is not None:
                    self._put(a, row, left[row])
                    if self.fired is None:
                        self.fired = self.step
        self._left = None
        return first


class SearchBitsTakesOtherWidths(R.RecentHistoryModel):
    """``search_bits`` takes the rows of another width as candidates (their first words, zero-extended)."""
    fired = None
    seen_by = staticmethod(lambda op: op["op"] == "search_bits")
    at_once = True

    def search_bits(self, attr, queries, k, metric="hamming", where=None):
        from tests.bits_helpers import distances, rank

        right = super().search_bits(attr, queries, k, metric, where)
        words = queries.shape[1]
        cand = self.candidates(attr, where)
        idx = np.flatnonzero(cand)
        codes = np.zeros((idx.size, words), np.uint64)
        for j, i in enumerate(idx.tolist()):
            code = self._lists[attr][i][:words]
            codes[j, :len(code)] = code
        dist = distances(queries, codes, metric) if idx.size else np.zeros((queries.shape[0], 0))
        labels, d64, counts = rank(dist, cand, k)
        wrong = (labels, d64.astype(np.float32), counts, d64)
        if self.fired is None and _differs(right, wrong):
            self.fired = self.step
        return wrong


class StatsCountsFilteredDeletes(R.RecentHistoryModel):
    """``attr_stats`` counts the rows ``tombstone_where`` deleted, until a compaction drops them."""
    fired = None
    seen_by = staticmethod(lambda op: op["op"] == "attr_stats")
    at_once = True
    _ghosts = None

    def tombstone_where(self, program):
        labels = super().tombstone_where(program)
        self._ghosts = labels if self._ghosts is None else np.union1d(self._ghosts, labels)
        return labels

    def compact(self):
        self._ghosts = None
        return super().compact()

    def reset(self, space=None):
        self._ghosts = None
        super().reset(space)

    def _outcome(self, *a):
        try:
            return super().attr_stats(*a), None
        except StatsOverflow as err:
            return (np.array([err.matched, err.by_absent]),), err

    def attr_stats(self, attr, by=None, max_groups=1, where=None):
        right, err = self._outcome(attr, by, max_groups, where)
        if self._ghosts is not None and self._ghosts.size:
            keep = self._deleted.copy()
            self._deleted[self._ghosts] = False
            try:
                wrong, wrong_err = self._outcome(attr, by, max_groups, where)
            finally:
                self._deleted = keep
            if self.fired is None and (len(right) != len(wrong) or _differs(right, wrong)):
                self.fired = self.step
            right, err = wrong, wrong_err
        if err is not None:
            raise err
        return right


class NearestReadsTheOldGeoColumn(R.RecentHistoryModel):
    """``geo_nearest`` is answered from the geo column as it was before the last ``update_where``."""
    fired = None
    seen_by = staticmethod(lambda op: op["op"] == "geo_nearest")
    at_once = True
    _before = None

    def update_where(self, program, assigns):
        self._before = {a: self._cols[a].copy() for a in R.GEO_COLUMNS if a in self._cols}
        return super().update_where(program, assigns)

    def geo_nearest(self, attr, center, limit, where=None, offset=0):
        right = super().geo_nearest(attr, center, limit, where, offset)
        old = (self._before or {}).get(attr)
        if old is None or old.size != self._cols[attr].size:
            return right
        keep = self._cols[attr]
        self._cols[attr] = old
        try:
            wrong = super().geo_nearest(attr, center, limit, where, offset)
        except AssertionError:  # (the rank guard was checked for the column as it is, not as it was)
            return right
        finally:
            self._cols[attr] = keep
        differs = any(not np.array_equal(x, y) for x, y in zip(right[:3], wrong[:3])) or right[3:] != wrong[3:]
        if self.fired is None and differs:  # (by value: a long double's bytes hold padding)
            self.fired = self.step
        return wrong


class SparseLegIgnoresTheProgram(R.RecentHistoryModel):
    """Hybrid's sparse leg ignores the program: only the dense leg is masked."""
    fired = None
    seen_by = staticmethod(lambda op: op["op"] == "search_hybrid")
    at_once = True
    _unmasked = False

    def candidates(self, attr, where=None, words=None):
        return super().candidates(attr, None if self._unmasked else where, words)

    def search_hybrid(self, *a, **kw):
        right = super().search_hybrid(*a, **kw)
        self._unmasked = True
        try:
            wrong = super().search_hybrid(*a, **kw)
        finally:
            self._unmasked = False
        if self.fired is None and _differs(right[:7], wrong[:7]):
            self.fired = self.step
        return wrong


@pytest.mark.parametrize("defect", [KeepsCodesInOldRowOrder, CodesSurviveReset, SearchBitsTakesOtherWidths,
                                    StatsCountsFilteredDeletes, NearestReadsTheOldGeoColumn, SparseLegIgnoresTheProgram])
def test_the_driver_reports_a_seeded_defect_in_the_recent_histories(defect, tmp_path, monkeypatch):
    from tests import conftest

    monkeypatch.setattr(conftest, "OUT_DIR", tmp_path)
    reported, real_call = 0, H.call
    for key in R.RECENT[:4]:
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
            assert engine.fired is not None and defect.seen_by(ops[failed]), (engine.fired, failed, ops[failed])
            if defect.at_once:  # `fired` is the first call whose answer the defect changes: that call is the one reported
                assert failed == engine.fired, (failed, engine.fired)
            else:               # the state breaks in a mutation; the first later call that reads it differently reports it
                assert failed > engine.fired and ops[engine.fired]["op"] in R.RECENT_MUTATIONS, (failed, engine.fired)
            dumped = json.loads((tmp_path / f"history_{tag}.json").read_text())
            assert dumped["failed_step"] == failed and dumped["ops"] == ops[:failed + 1]
            print(f"{defect.__name__}: {tag} fired at step {engine.fired}, reported at step {failed} ({ops[failed]['op']})")
            reported += 1
        else:
            assert engine.fired is None or not defect.at_once, f"{tag}: fired at step {engine.fired}, never reported"
        monkeypatch.setattr(H, "call", real_call)
    assert reported >= 2, f"{defect.__name__}: reported in {reported} of 4 histories"


# ---------------------------------------------------------------- redraws
def test_near_tie_redraws_stay_under_one_percent():
    """Near-ties of the kNN kinds, and in the recent histories the draws that tripped a guard of tests/geo_helpers.py."""
    drawn = redrawn = 0
    for key in H.HISTORIES + H.WIDE + H.WIDE_LARGE + R.RECENT + R.RECENT_LARGE:
        a, b = H.redraw_counts(*key)
        if key[3] in R.RECENT_SCALES:
            print(f"history {H.history_tag(*key)}: {b} of {a} drawn queries were redrawn")
        drawn, redrawn = drawn + a, redrawn + b
    print(f"{redrawn} of {drawn} drawn queries were redrawn")
    assert drawn > 300 and redrawn <= 0.01 * drawn
