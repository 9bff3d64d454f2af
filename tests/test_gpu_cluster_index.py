"""``Index.cluster`` / ``assign_clusters`` and ``QueryProcessor.cluster_vectors`` on the MI355X: a 2,400 x 32 namespace of six
separated blobs, the cluster id written on the device and then read by the families that already read attribute columns
-- facets, filters, distinct -- and kept through save / load and in the storage's metadata."""
import functools

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO

pytestmark = pytest.mark.gpu

N, D, K = 2400, 32, 6


@functools.lru_cache(maxsize=None)
def blobs():
    rng = np.random.default_rng(77)
    centres = rng.standard_normal((K, D)) * 20.0
    blob = rng.integers(K, size=N)
    rows = (centres[blob] + 0.5 * rng.standard_normal((N, D))).astype(np.float32)
    rows.setflags(write=False)
    return rows, blob


def filled(space):
    rows, blob = blobs()
    index = Index(space=space, attributes={"cluster": "int", "g": "int"})
    vecs = [Vector(values=r, metadata={"g": i % 2, "i": i}) for i, r in enumerate(rows)]
    index.add(vecs, "ns")
    return index, [v.id for v in vecs], rows, blob


@pytest.mark.parametrize("space", ["l2", "cosine"])
def test_the_cluster_column_serves_facets_filters_distinct_and_save_load(space, tmp_path):
    index, ids, rows, blob = filled(space)
    try:
        seeds = [int(np.flatnonzero(blob == j)[0]) for j in range(K)]
        got = index.cluster("ns", space, K, init=[ids[i] for i in seeds], assign_to="cluster")
        assert got.converged and got.iterations == 2 and np.array_equal(got.sizes, np.bincount(blob, minlength=K))
        column = index._int_attribute_of("ns", "cluster", ids)
        assert column == blob.tolist()  # centroid j was seeded inside blob j
        # facets: the sizes
        facet = index.facets("ns", "cluster", order="value")
        assert facet["values"] == [(j, int(s)) for j, s in enumerate(got.sizes)] and facet["matched"] == N and facet["absent"] == 0
        # a filter on the cluster id: only members come back
        queries = rows[[seeds[2], seeds[4]]]
        hits = index.search_many(queries, 20, "ns", space, where={"cluster": 2})
        at = {u: i for i, u in enumerate(ids)}
        assert all(len(h) == 20 and all(blob[at[x.vector_id]] == 2 for x in h) for h in hits)
        # distinct: one hit per cluster, the query's own cluster first
        one_each = index.search_many(queries, K, "ns", space, distinct="cluster")
        for q, h in zip((2, 4), one_each):
            found = [blob[at[x.vector_id]] for x in h]
            assert sorted(found) == list(range(K)) and found[0] == q
        # init by seed and by array: the same partition, whatever the labelling
        by_seed = index.cluster("ns", space, K, seed=5, max_iterations=50, assign_to="cluster")
        assert by_seed.sizes.sum() == N and index.facets("ns", "cluster", order="value")["values"] == \
            [(j, int(s)) for j, s in enumerate(by_seed.sizes) if s]
        again = index.cluster("ns", space, K, seed=5, max_iterations=50)
        assert again.centroids.tobytes() == by_seed.centroids.tobytes() and again.iterations == by_seed.iterations
        by_array = index.cluster("ns", space, K, init=got.centroids, assign_to="cluster")
        assert by_array.converged and np.array_equal(by_array.sizes, got.sizes)
        assert index._int_attribute_of("ns", "cluster", ids) == column
        # rows appended later go to the centroids there already are; the others are not candidates of the filtered call
        more = [Vector(values=r, metadata={"g": 7, "i": N + i}) for i, r in enumerate(rows[:60] + np.float32(0.01))]
        index.add(more, "ns")
        new_ids = [v.id for v in more]
        assert index._int_attribute_of("ns", "cluster", new_ids) == [None] * 60
        sizes, costs = index.assign_clusters("ns", space, got.centroids, assign_to="cluster", where={"g": 7})
        assert index._int_attribute_of("ns", "cluster", new_ids) == blob[:60].tolist() and sizes.sum() == 60
        assert index._int_attribute_of("ns", "cluster", ids) == column and (costs >= 0).all()
        # save / load keeps the ids
        assert index.save_index(str(tmp_path / "ix"))
        loaded = Index(space=space, attributes={"cluster": "int", "g": "int"})
        try:
            assert loaded.load_index(str(tmp_path / "ix"))
            assert loaded._int_attribute_of("ns", "cluster", ids + new_ids) == column + blob[:60].tolist()
            assert loaded.facets("ns", "cluster", order="value")["values"] == index.facets("ns", "cluster", order="value")["values"]
        finally:
            loaded.close()
    finally:
        index.close()


def test_query_processor_writes_the_cluster_id_into_the_column_and_the_metadata():
    rows, blob = blobs()
    index = Index(space="cosine", attributes={"cluster": "int", "g": "int"})
    storage = InMemoryStorage()
    qp = QueryProcessor(storage, index)
    try:
        n = 800
        qp.upsert_many([VectorDTO(values=r.tolist(), metadata={"g": i % 2, "i": i}) for i, r in enumerate(rows[:n])], "ns")
        stored = storage.namespace_map["ns"]
        ids = [v.id for v in stored]
        assert [v.metadata["i"] for v in stored] == list(range(n))
        result = qp.cluster_vectors(K, "ns", "cosine", seed=3, max_iterations=50, assign_to="cluster")
        column = index._int_attribute_of("ns", "cluster", ids)
        meta = [v.metadata.get("cluster") for v in storage.read_vectors(ids, "ns")]
        assert meta == column and None not in column and np.array_equal(np.bincount(column, minlength=K), result.sizes)
        assert result.inertia == float(np.add.accumulate(result.costs)[-1])
        # only the even rows against the blob seeds: the odd rows keep column and metadata
        seeds = np.stack([rows[:n][blob[:n] == j][0] for j in range(K)])
        sizes, costs = qp.assign_clusters(seeds, "ns", "cosine", assign_to="cluster", where={"g": 0})
        column2 = index._int_attribute_of("ns", "cluster", ids)
        meta2 = [v.metadata.get("cluster") for v in storage.read_vectors(ids, "ns")]
        assert meta2 == column2 and column2[1::2] == column[1::2] and column2[0::2] == blob[:n][0::2].tolist()
        assert sizes.sum() == n // 2
        hits = qp.find_similar_many([VectorDTO(values=seeds[1].tolist(), metadata={})], 5, "ns", "cosine", where={"cluster": 1, "g": 0})
        assert len(hits[0]) == 5 and all(h["metadata"]["cluster"] == 1 and h["metadata"]["g"] == 0 for h in hits[0])
    finally:
        index.close()
