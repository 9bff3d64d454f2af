"""``Index.join_within`` / ``duplicate_groups`` and ``QueryProcessor.find_duplicates`` on the MI355X: a 3,000 x 48
namespace with planted groups of identical rows and perturbed copies, against the route the join replaces
(``fetch_values_by_id`` -> ``range_search_many``, stripped on the host) and against the planted truth."""
import functools

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO
from mlvectordb_amd.engine import JoinOverflow

pytestmark = pytest.mark.gpu

N, D = 3000, 48
GROUPS = [[5, 1500, 2999], [40, 41], [700, 2100, 2101, 2500], [0, 256]]
PERTURBED = [(900 + j, 1900 + 3 * j) for j in range(8)]  # joined to their originals at the radius, to nothing else
RADIUS = {"l2": 0.01, "euclidean": 0.1, "cosine": 1e-4}


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(99)
    rows = rng.standard_normal((N, D), dtype=np.float32)
    for g in GROUPS:
        rows[g[1:]] = rows[g[0]]
    for a, b in PERTURBED:
        rows[b] = rows[a] * (1 + np.float32(1e-3) * rng.standard_normal(D, dtype=np.float32))
    rows.setflags(write=False)
    truth = sorted([(a, b) for g in GROUPS for i, a in enumerate(g) for b in g[i + 1:]] + PERTURBED)
    return rows, truth


def filled(space: str):
    rows, truth = planted()
    index = Index(space=space, attributes={"g": "int"})
    vecs = [Vector(values=r, metadata={"g": i % 2, "i": i}) for i, r in enumerate(rows)]
    index.add(vecs, "ns")
    return index, [v.id for v in vecs], rows, truth


def host_route(index, ids, metric, radius, where=None):
    """The pairs by the calls the join replaces: per 256 rows fetch_values_by_id -> range_search_many, b <= a stripped."""
    at = {u: i for i, u in enumerate(ids)}
    live = [i for i, u in enumerate(ids) if where is None or where(i)]
    out = []
    for s in range(0, len(live), 256):
        chunk = live[s:s + 256]
        values = index.fetch_values_by_id("ns", [ids[i] for i in chunk])
        kw = {} if where is None else {"where": {"g": 1}}
        for a, hits in zip(chunk, index.range_search_many(values, radius, "ns", metric, max_results=None, **kw)):
            out += [(a, at[h.vector_id], h.score) for h in hits if at[h.vector_id] > a]
    return out


@pytest.mark.parametrize("space,metric", [("l2", "l2"), ("l2", "euclidean"), ("cosine", "cosine")])
def test_self_join_by_ids_and_groups_agree_with_the_route_they_replace(space, metric):
    index, ids, rows, truth = filled(space)
    radius = RADIUS[metric]
    try:
        pairs = index.join_within("ns", metric, radius)
        got = list(zip(pairs.left_labels.tolist(), pairs.right_labels.tolist(), pairs.scores.tolist()))
        assert [(a, b) for a, b, _ in got] == truth and pairs.complete, "the planted pairs, every one once, grouped by left row"
        assert got == host_route(index, ids, metric, radius), "pairs and scores of fetch_values_by_id -> range_search_many"
        assert pairs.left_ids.tolist() == [ids[a] for a, _ in truth] and pairs.right_ids.tolist() == [ids[b] for _, b in truth]
        assert int(pairs.counts.sum()) == len(truth) and pairs.counts.size == N
        # with a dict where: both sides match it
        odd = index.join_within("ns", metric, radius, where={"g": 1})
        want_odd = [(a, b) for a, b in truth if a % 2 and b % 2]
        assert list(zip(odd.left_labels.tolist(), odd.right_labels.tolist())) == want_odd and want_odd
        assert list(zip(odd.left_labels.tolist(), odd.right_labels.tolist(), odd.scores.tolist())) == \
            host_route(index, ids, metric, radius, where=lambda i: i % 2 == 1)
        # by ids, in the caller's order, the row itself left out
        asked = [2101, 7, 5, 700]
        near = index.join_within("ns", metric, radius, ids=[ids[j] for j in asked])
        assert near.counts.tolist() == [3, 0, 2, 3]
        assert sorted(zip(near.left_labels.tolist(), near.right_labels.tolist())) == sorted(
            [(2101, 700), (2101, 2100), (2101, 2500), (5, 1500), (5, 2999), (700, 2100), (700, 2101), (700, 2500)])
        assert near.left_labels.tolist() == [2101] * 3 + [5] * 2 + [700] * 3
        # order="distance": nearest pair first
        ranked = index.join_within("ns", metric, radius, order="distance")
        keys = list(zip(ranked.distances.tolist(), ranked.left_labels.tolist(), ranked.right_labels.tolist()))
        assert keys == sorted(keys) and sorted((a, b) for _, a, b in keys) == truth
        # the groups: connected components in insertion order, ordered by their first member
        components = sorted([sorted(g) for g in GROUPS] + [sorted(p) for p in PERTURBED])
        assert index.duplicate_groups("ns", metric, radius) == [[ids[x] for x in g] for g in components]
        assert index.duplicate_groups("ns", metric, radius, where={"g": 1}) == \
            [[ids[x] for x in g if x % 2] for g in components if sum(x % 2 for x in g) >= 2]
        # a row with more partners than max_per_row: the nearest come back, complete says so, the groups raise
        cut = index.join_within("ns", metric, radius, max_per_row=1)
        assert not cut.complete and np.array_equal(cut.counts, pairs.counts) and len(cut) == int((pairs.counts > 0).sum())
        with pytest.raises(JoinOverflow) as e:
            index.duplicate_groups("ns", metric, radius, max_per_row=2)
        assert e.value.most == 3
        # a removed row is nobody's partner and no left row
        index.remove([ids[2100]], "ns")
        after = index.join_within("ns", metric, radius)
        assert list(zip(after.left_labels.tolist(), after.right_labels.tolist())) == [p for p in truth if 2100 not in p]
    finally:
        index.close()


def test_query_processor_find_duplicates_over_in_memory_storage():
    rows, truth = planted()
    index = Index(space="cosine", attributes={"g": "int"})
    qp = QueryProcessor(InMemoryStorage(), index)
    try:
        qp.upsert_many([VectorDTO(values=r.tolist(), metadata={"g": i % 2, "i": i}) for i, r in enumerate(rows[:1000])], "ns")
        groups = qp.find_duplicates(1e-4, "ns")
        want = sorted(sorted(x for x in g if x < 1000) for g in GROUPS)
        want = [g for g in want if len(g) >= 2]
        assert [[m["metadata"]["i"] for m in g] for g in groups] == want and want
        assert all(np.array_equal(np.asarray(m["values"], np.float32), rows[m["metadata"]["i"]]) for g in groups for m in g)
        found = qp.find_near_pairs(1e-4, "ns")
        assert [(p["left"]["metadata"]["i"], p["right"]["metadata"]["i"]) for p in found["pairs"]] == \
            [(a, b) for a, b in truth if b < 1000] and found["complete"]
        assert all(abs(p["score"] - 1.0) < 1e-6 for p in found["pairs"])
        on_device = qp.find_near_pairs(1e-4, "ns", where={"g": 0})
        on_host = qp.find_near_pairs(1e-4, "ns", where=lambda m: m["g"] == 0)
        assert [(p["left"]["id"], p["right"]["id"], p["score"]) for p in on_device["pairs"]] == \
            [(p["left"]["id"], p["right"]["id"], p["score"]) for p in on_host["pairs"]] and on_host["pairs"]
    finally:
        index.close()
