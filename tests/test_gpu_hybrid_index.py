"""Hybrid search through ``Index`` and ``QueryProcessor`` on the real engine, end to end: the same vectors go into an
``Index`` on the device and into one on the model engine of tests/hybrid_helpers.py, and every answer -- ids, fused scores,
components and ranks -- is compared, before and after removals, updates by id, a v4 snapshot round trip and a compaction.
Dense components are small integers and sparse weights multiples of 1/8: the comparison is exact."""
import numpy as np
import pytest

from mlvectordb_amd import HybridBatchHits, Index, Vector
from mlvectordb_amd.query_processor import QueryProcessor
from mlvectordb_amd.storage import InMemoryStorage
from tests.hybrid_helpers import METHODS, HybridOracleEngine
from tests.sparse_helpers import random_corpus, random_vector

pytestmark = pytest.mark.gpu

SCHEMA = {"lexical": "sparse", "year": "int", "tags": "str[]"}
VOCAB = 64
DIM = 32


def _same(a, b, tag):
    assert type(a) is type(b) and np.array_equal(a.counts, b.counts), tag
    assert a == b, tag  # (ids and scores of every hit)
    assert a.scores.tobytes() == b.scores.tobytes(), tag
    if isinstance(a, HybridBatchHits):
        for name in ("dense", "sparse", "rank_dense", "rank_sparse"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (tag, name)


def test_index_and_query_processor_on_the_device_against_the_model_index(tmp_path):
    rng = np.random.default_rng(21)
    rows = random_corpus(rng, 600, VOCAB, exact=True)
    metas = [{"lexical": r, "year": 1990 + i % 9, "tags": ["a", "b"] if i % 3 else ["b"]} for i, r in enumerate(rows)]
    for m in metas[::17]:
        del m["lexical"]
    vectors = [Vector(values=rng.integers(-4, 5, DIM).astype(np.float32).tolist(), metadata=m) for m in metas]
    real = Index(space="l2", attributes=SCHEMA)
    model = Index(space="l2", engine_factory=lambda dim, sp: HybridOracleEngine(dim, sp), attributes=SCHEMA)
    kept = real
    try:
        for lo in (0, 200, 400):
            for index in (real, model):
                index.add(vectors[lo:lo + 200], "ns")
        q = rng.integers(-4, 5, (7, DIM)).astype(np.float32)
        sq = [random_vector(rng, n, VOCAB, exact=True) for n in (1, 4, 9, 25, 40)] + [{}, {0: 1.0, 2 ** 31 - 1: 1.0}]
        filters = [None, {"year": {"$gte": 1995}}, {"tags": "a", "lexical": {"$size": {"$gte": 2, "$lt": 30}}},
                   {"lexical": {"$exists": False}}, {"year": 1800}]

        def check(tag):
            for where in filters:
                for method in METHODS:
                    for kw in (dict(), dict(top_k=64, fetch_k=1024, fetch_k_sparse=64), dict(top_k=3, fetch_k=2, fetch_k_sparse=1)):
                        args = dict(top_k=10, namespace="ns", metric="l2", by="lexical", fusion=method, weights=(0.5, 2.0),
                                    rrf_k=4.0, where=where)
                        args.update(kw)
                        for components in (False, True):
                            _same(real.search_hybrid(q, sq, components=components, **args),
                                  model.search_hybrid(q, sq, components=components, **args), (tag, where, method, kw))
            assert real.search_hybrid(q, sq, 5, "ns", "l2", "lexical").counts.tolist() == [5] * 7

        check("ingest")
        patches = [{"lexical": random_vector(rng, 12, VOCAB, exact=True)}, {"lexical": None}, {"lexical": {}},
                   {"lexical": ([3, 1], [0.5, -2.0]), "year": 1999}] * 10
        ids = [v.id for v in vectors]
        for index in (real, model):
            assert index.update_attributes(ids[:40], patches, "ns") == 40
            index.remove(ids[5:600:6], "ns")
        check("updated and removed")
        real.save_index(str(tmp_path))
        assert '"mlvdb-index-v4"' in (tmp_path / "index.json").read_text()
        real = Index(space="l2")
        assert real.load_index(str(tmp_path)) and real.attributes == SCHEMA
        check("loaded")
        for index in (real, model):
            assert index.compact("ns")
        check("compacted")
    finally:
        kept.close()
        if real is not kept:
            real.close()


def test_query_processor_find_similar_hybrid_many_on_the_device():
    rng = np.random.default_rng(8)
    rows = random_corpus(rng, 300, VOCAB, exact=True)
    metas = [{"lexical": r, "year": 2000 + i % 5} if r is not None else {"year": 2000 + i % 5} for i, r in enumerate(rows)]
    vectors = [Vector(values=rng.integers(-4, 5, DIM).astype(np.float32).tolist(), metadata=m) for m in metas]
    real = Index(space="l2", attributes={"lexical": "sparse", "year": "int"})
    model = Index(space="l2", engine_factory=lambda dim, sp: HybridOracleEngine(dim, sp),
                  attributes={"lexical": "sparse", "year": "int"})
    try:
        qps = []
        for index in (real, model):
            qp = QueryProcessor(InMemoryStorage(), index)
            qp.upsert_many(vectors)
            qps.append(qp)
        q = rng.integers(-4, 5, (4, DIM)).astype(np.float32)
        sq = [random_vector(rng, n, VOCAB, exact=True) for n in (2, 7, 20)] + [{}]

        def plain(answer):  # (each processor gave its copies of the vectors ids of its own)
            return [[(h["score"], np.asarray(h["values"]).tolist(), h["metadata"]) for h in hits] for hits in answer]

        for kw in (dict(), dict(fusion="rrf", rrf_k=0.0, weights=(1.0, 3.0)), dict(fusion="linear", weights=(0.25, 2.0)),
                   dict(fusion="relative", where={"year": {"$lt": 2003}})):
            got, want = (qp.find_similar_hybrid_many(q, sq, 10, "default", "l2", "lexical", **kw) for qp in qps)
            assert plain(got) == plain(want), kw
            assert all(len(hits) == 10 and set(hits[0]) == {"id", "values", "metadata", "score"} for hits in got)
        one = qps[0].find_similar_hybrid(vectors[3], sq[1], 5, metric="l2", by="lexical")
        assert plain([one]) == plain([qps[1].find_similar_hybrid(vectors[3], sq[1], 5, metric="l2", by="lexical")]) and len(one) == 5
    finally:
        real.close()
