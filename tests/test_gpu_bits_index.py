"""Bits attributes through ``Index`` and ``QueryProcessor`` on the real engine, end to end: ingest from metadata,
``search_bits`` with and without a filter, updates by id, removals by id and by filter, a v6 snapshot and a compaction --
every answer against the model of tests/bits_helpers.py, which reads the metadata dicts alone.  All comparisons are exact."""
import numpy as np
import pytest

from mlvectordb_amd import Index, Vector
from mlvectordb_amd import where as W
from mlvectordb_amd.interfaces import VectorDTO
from mlvectordb_amd.query_processor import QueryProcessor
from mlvectordb_amd.storage import InMemoryStorage
from tests.bits_helpers import METRICS, distances, near, random_codes, rank, unpack

pytestmark = pytest.mark.gpu

SCHEMA = {"sig": "bits320", "year": "int", "tags": "str[]"}
WORDS = 5


def form(words, i):
    """One code in the i-th of its three value forms: bytes, a uint8 array, a bool array."""
    raw = np.asarray(words, dtype="<u8").tobytes()
    return (raw, np.frombuffer(raw, dtype=np.uint8), unpack(np.asarray(words, np.uint64)[None, :])[0].astype(bool))[i % 3]


def words_of(value):
    return None if value is None else W.encode_bits_code(value, 64 * WORDS, "x")


def test_index_with_a_bits_attribute_on_the_device(tmp_path):
    rng = np.random.default_rng(14)
    codes, base = random_codes(rng, 600, WORDS)
    metas = [{"sig": form(c, i), "year": 1990 + i % 9, "tags": ["a", "b"] if i % 3 else ["b"]} for i, c in enumerate(codes)]
    for m in metas[::17]:
        del m["sig"]
    vectors = [Vector(values=rng.standard_normal(32).astype(np.float32).tolist(), metadata=m) for m in metas]
    index = Index(space="cosine", attributes=SCHEMA)
    try:
        for lo in (0, 200, 400):
            index.add(vectors[lo:lo + 200], "ns")
        model = {v.id: dict(m) for v, m in zip(vectors, metas)}
        order = [v.id for v in vectors]
        queries = np.stack([base[0], base[1], base[3], near(rng, base[5], 4), codes[77], rng.integers(0, 2 ** 64, WORDS, dtype=np.uint64)])
        asked = [form(q, i) for i, q in enumerate(queries)]
        filters = [(None, lambda m: True), ({"year": {"$gte": 1995}}, lambda m: m["year"] >= 1995),
                   ({"tags": "a", "sig": {"$exists": True}}, lambda m: "a" in m["tags"]),
                   ({"year": 1800}, lambda m: False)]

        def check(tag):
            ids = [i for i in order if i in model]
            held = [words_of(model[i].get("sig")) for i in ids]
            have = [j for j, w in enumerate(held) if w is not None]
            for where, keep in filters:
                cand = np.zeros(len(ids), dtype=bool)
                cand[[j for j in have if keep(model[ids[j]])]] = True
                rows = np.array([held[j] for j in np.flatnonzero(cand).tolist()], dtype=np.uint64).reshape(-1, WORDS)
                for metric in METRICS:
                    dist = distances(queries, rows, metric) if rows.size else np.zeros((len(queries), 0))
                    for k in (1, 10, 64):
                        labels, d64, counts = rank(dist, cand, k)
                        want = [[(ids[l], d) for l, d in zip(labels[q, :counts[q]].tolist(), d64[q, :counts[q]].tolist())]
                                for q in range(len(queries))]
                        got = index.search_bits(asked, k, "ns", "sig", metric=metric, where=where)
                        assert [[(h.vector_id, h.score) for h in hits] for hits in got] == want, (tag, where, metric, k)
            assert index.count("ns", {"sig": {"$exists": True}}) == len(have), tag

        check("ingest")
        patches = [{"sig": form(near(rng, base[3], 2), 0)}, {"sig": None}, {"sig": form(base[0], 2)},
                   {"sig": form(codes[300], 1), "year": 1999}] * 10
        assert index.update_attributes(order[:40], patches, "ns") == 40
        for i, p in zip(order[:40], patches):
            model[i].update(p)
        check("update_attributes")
        with pytest.raises(ValueError, match="39 bytes"):
            index.update_attributes(order[:2], [{"sig": b"\x00" * 40}, {"sig": b"\x00" * 39}], "ns")
        with pytest.raises(ValueError, match="bits320 attribute"):
            index.update_where("ns", {"year": 1999}, {"sig": b"\x00" * 40})
        with pytest.raises(ValueError, match="bits320 column"):
            index.facets("ns", "sig")
        check("after the refusals")
        gone = order[5:600:6]
        index.remove(gone, "ns")
        for i in gone:
            del model[i]
        check("remove")
        assert index.remove_where("ns", {"year": 1993}) == sum(m["year"] == 1993 for m in model.values()) > 0
        for i in [i for i, m in model.items() if m["year"] == 1993]:
            del model[i]
        check("remove_where")
        index.save_index(str(tmp_path))
        assert '"mlvdb-index-v6"' in (tmp_path / "index.json").read_text()
        dense = np.fromfile(tmp_path / "ns0.attr0.bits.u64", dtype="<u8")
        assert dense.size == WORDS * sum(m.get("sig") is not None for m in model.values())
        loaded = Index(space="cosine")
        try:
            assert loaded.load_index(str(tmp_path)) and loaded.attributes == SCHEMA
            index, kept = loaded, index
            check("loaded")
            assert index.compact("ns")
            order = [i for i in order if i in model]
            check("loaded and compacted")
            used, live = index._ns["ns"].engine.list_stats(0)
            assert used == live == WORDS * sum(m.get("sig") is not None for m in model.values())
        finally:
            loaded.close()
            index = kept
    finally:
        index.close()


def test_query_processor_find_similar_bits_on_the_device():
    rng = np.random.default_rng(15)
    qp = QueryProcessor(InMemoryStorage(), Index(space="cosine", attributes={"sig": "bits128", "year": "int"}))
    try:
        codes, base = random_codes(rng, 300, 2)
        # (the metadata travels through the storage: a code is kept there as a list of 0 / 1)
        metas = [{"sig": None if i % 11 == 0 else unpack(c[None, :])[0].tolist(), "year": i % 5, "i": i} for i, c in enumerate(codes)]
        qp.upsert_many([VectorDTO(values=rng.standard_normal(16).tolist(), metadata=m) for m in metas])
        queries = np.stack([base[1], base[4], near(rng, codes[8], 3)])
        asked = [unpack(q[None, :])[0].astype(bool) for q in queries]
        for metric in METRICS:
            for where, keep in ((None, lambda m: True), ({"year": {"$lt": 2}}, lambda m: m["year"] < 2)):
                cand = np.array([m["sig"] is not None and keep(m) for m in metas], dtype=bool)
                labels, d64, counts = rank(distances(queries, codes[cand], metric), cand, 10)
                got = qp.find_similar_bits_many(asked, 10, by="sig", metric=metric, where=where)
                assert [[(h["metadata"]["i"], h["score"]) for h in hits] for hits in got] == \
                    [list(zip(labels[q, :counts[q]].tolist(), d64[q, :counts[q]].tolist())) for q in range(3)]
                one = qp.find_similar_bits(asked[0], 10, by="sig", metric=metric, where=where)
                assert [(h["id"], h["score"]) for h in one] == [(h["id"], h["score"]) for h in got[0]]
                assert set(got[0][0]) == {"id", "values", "metadata", "score"}
    finally:
        qp._index.close()
