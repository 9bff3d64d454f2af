"""Per-query metadata filters in batched range search (include/mlvdb_where_each_range.h) without a GPU: the C ABI's shape,
the stitching of chunked native calls in ``HipScanEngine.range_each`` (over a fake library), and Index / QueryProcessor on
an oracle engine that answers every query under its own program."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine, RangeHits, stitch_range_hits
from tests.where_helpers import SCHEMA, EachRangeOracleEngine, py_match, random_filter, random_metadata

ROOT = Path(__file__).resolve().parents[1]
ENTRY = "mlvdb_range_batch_packed_where_each"


def header_text():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_where_each_range.h").read_text(), flags=re.S)


# ---------------------------------------------------------------- C ABI
def test_header_declares_the_entry_and_the_library_exports_it():
    text = header_text()
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == [ENTRY]
    assert sorted(_native.WHERE_EACH_RANGE_SIGNATURES) == [ENTRY]
    lib = _native.load()
    assert hasattr(lib, ENTRY)
    assert lib.mlvdb_abi_version() == _native.ABI_VERSION == 7  # additive: the version did not move
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert int(consts["MLVDB_WHERE_EACH_RANGE_LIST"]) == _native.WHERE_EACH_RANGE_LIST
    internal = (ROOT / "mlvectordb_amd" / "csrc" / "internal.h").read_text()
    assert re.search(r"constexpr int kCandCap = %d;" % _native.WHERE_EACH_RANGE_LIST, internal)
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert "mlvdb_where_each_range.h" in make


def test_ctypes_signature_matches_the_header():
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % ENTRY, header_text(), flags=re.S).group(1)
    params = [" ".join(p.split()) for p in proto.split(",")]

    def ctype(p):
        if "*" in p:
            return C.POINTER(_native.Where) if "mlvdb_where" in p else C.c_void_p
        return {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}[p.split()[-2]]

    restype, argtypes = _native.WHERE_EACH_RANGE_SIGNATURES[ENTRY]
    assert restype is C.c_int
    assert argtypes == [ctype(p) for p in params], params
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["h", "queries", "nq", "radius", "capacity", "total_capacity", "programs", "n_programs",
                     "program_of_query", "out_labels", "out_dist", "out_offsets", "out_counts", "out_routes"]


def test_the_entry_refuses_a_null_handle_with_a_status_code_and_runs_guarded():
    lib = _native.load()
    buf = (C.c_int64 * 4)()
    w = (_native.Where * 1)()
    rc = getattr(lib, ENTRY)(C.c_void_p(), buf, 1, 1.0, 4, 4, w, 1, buf, buf, buf, buf, buf, buf)
    assert rc == 1  # MLVDB_ERR_INVALID_ARG
    assert b"null index handle" in lib.mlvdb_last_global_error()
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    region = text[text.index('extern "C" {'):text.rindex('}  // extern "C"')]
    bodies = dict(re.findall(r"^int (mlvdb_\w+)\([^)]*\) \{\n(.*?)^\}", region, flags=re.S | re.M))
    assert bodies[ENTRY].lstrip().startswith("return guarded(")


def test_the_gathered_range_kernel_is_in_the_build():
    src = (ROOT / "mlvectordb_amd" / "csrc" / "kernels_where_each.hip").read_text()
    assert "where_gather_range_kernel" in src and "launch_where_gather_range" in src
    assert "asm" not in src  # plain HIP: vector stores and atomicAdd


# ---------------------------------------------------------------- stitching
def test_stitch_range_hits_keeps_query_order():
    parts = []
    for idx in (np.array([1, 4]), np.array([0, 2, 3])):
        lens = idx % 3
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        lab = np.concatenate([np.full(n, i, np.int64) for i, n in zip(idx, lens)] + [np.zeros(0, np.int64)])
        parts.append((idx, lab, lab.astype(np.float32) + 0.5, off))
    hits = stitch_range_hits(parts, 5)
    assert len(hits) == 5 and hits.offsets.tolist() == [0, 0, 1, 3, 3, 4]
    for i in range(5):
        lab, dst = hits[i]
        assert lab.tolist() == [i] * (i % 3) and dst.tolist() == [i + 0.5] * (i % 3)
    one = (np.arange(3), np.arange(3, dtype=np.int64), np.ones(3, np.float32), np.arange(4, dtype=np.int64))
    assert stitch_range_hits([one], 3).labels is one[1]  # a single call over the whole batch: nothing is copied


class FakeLib:
    """``mlvdb_range_batch_packed_where_each`` under the packed-output rules, in Python: query i (its number rides in its first
    component) under program p has the hits ``hits_of(i, p)``; every call is recorded."""

    def __init__(self, programs, dim):
        self.key = {W._program_key(p): j for j, p in enumerate(programs)}
        self.dim = dim
        self.calls = []

    @staticmethod
    def hits_of(i, p):
        n = (i * 7 + p + 1) % 5
        return [1000 * i + 10 * (p + 1) + t for t in range(n)]

    @staticmethod
    def _arr(ptr, ctype, n):
        if not ptr or n == 0:
            return np.zeros(0, ctype)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,))

    def mlvdb_range_batch_packed_where_each(self, h, q, nq, radius, capacity, total, arr, n_programs, of, labels, dist,
                                            offsets, counts, routes):
        assert n_programs <= W.EACH_MAX_PROGRAMS
        qs = self._arr(q, C.c_float, nq * self.dim).reshape(nq, self.dim)
        local = self._arr(of, C.c_int32, nq)
        ops_n = 0
        glob = []
        for j in range(n_programs):
            w = arr[j]
            ops = np.ctypeslib.as_array(C.cast(w.ops, C.POINTER(C.c_uint8)), shape=(w.n_ops * W.OP_DTYPE.itemsize,))
            st = self._arr(w.set, C.c_int64, w.n_set)
            glob.append(self.key[(ops.tobytes(), st.tobytes())])
            ops_n += w.n_ops
        assert ops_n <= W.EACH_MAX_OPS
        self.calls.append((nq, n_programs, total))
        off, cnt = self._arr(offsets, C.c_int64, nq + 1), self._arr(counts, C.c_int64, nq)
        per = [self.hits_of(int(qs[j, 0]), glob[local[j]] if local[j] >= 0 else -1) for j in range(nq)]
        off[0] = 0
        for j, hs in enumerate(per):
            cnt[j] = len(hs)
            off[j + 1] = off[j] + min(len(hs), capacity)
        self._arr(routes, C.c_int32, n_programs)[:] = _native.ROUTE_GATHER
        if off[nq] > total:
            return _native.ERR_OVERFLOW
        lab, dst = self._arr(labels, C.c_int64, total), self._arr(dist, C.c_float, total)
        for j, hs in enumerate(per):
            lab[off[j]:off[j + 1]] = hs[:capacity]
            dst[off[j]:off[j + 1]] = np.asarray(hs[:capacity], np.float32) / 8
        return _native.ERR_OVERFLOW if any(len(hs) > capacity for hs in per) else _native.OK

    def mlvdb_last_error(self, h):
        return b"fake"


def fake_engine(programs, dim):
    eng = object.__new__(HipScanEngine)
    eng._lib, eng._h, eng.dim, eng.space = FakeLib(programs, dim), None, dim, "l2"
    return eng


def test_range_each_stitches_chunked_calls_in_query_order():
    nq, dim = 300, 4
    wheres = [None if i % 11 == 0 else {"year": int((i * 37) % 150)} for i in range(nq)]
    programs, of = W.compile_each(wheres, SCHEMA)
    assert len(programs) > 2 * W.EACH_MAX_PROGRAMS  # three native calls
    eng = fake_engine(programs, dim)
    qs = np.zeros((nq, dim), np.float32)
    qs[:, 0] = np.arange(nq)
    hits, routes = eng.range_each(qs, 1.0, 16, programs, of, return_routes=True)
    assert isinstance(hits, RangeHits) and len(hits) == nq
    assert len(eng._lib.calls) == 3 and sum(c[0] for c in eng._lib.calls) == nq
    assert (routes == _native.ROUTE_GATHER).all() and routes.shape == (len(programs),)
    for i in range(nq):
        want = FakeLib.hits_of(i, int(of[i]))
        lab, dst = hits[i]
        assert lab.tolist() == want and dst.tolist() == [w / 8 for w in want], i
    # truncation: the nearest `capacity` of every query, the call not repeated
    eng._lib.calls.clear()
    cut = eng.range_each(qs, 1.0, 2, programs, of, truncate=True)
    assert len(eng._lib.calls) == 3
    assert all(cut[i][0].tolist() == FakeLib.hits_of(i, int(of[i]))[:2] for i in range(nq))
    # capacity as a first guess: a chunk whose queries have more hits is repeated once with the size it reported
    eng._lib.calls.clear()
    grown = eng.range_each(qs, 1.0, 2, programs, of)
    assert 3 < len(eng._lib.calls) <= 6
    assert all(grown[i][0].tolist() == FakeLib.hits_of(i, int(of[i])) for i in range(nq))
    with pytest.raises(RuntimeError, match="program_of_query"):
        eng.range_each(qs, 1.0, 2, programs, of[:5])


# ---------------------------------------------------------------- Index / QueryProcessor over the oracle engine
def _filled(space="l2", seed=11, n=320, d=8):
    rng = np.random.default_rng(seed)
    index = Index(space=space, engine_factory=EachRangeOracleEngine, attributes=SCHEMA)
    metas = random_metadata(rng, n)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs[:200], "ns")
    index.add(vecs[200:], "ns")
    gone = [v.id for v in vecs[::9]]
    index.remove(gone, "ns")
    return rng, index, vecs, set(gone)


def ids(per_query):
    return [[(h.vector_id, h.score) for h in row] for row in per_query]


@pytest.mark.parametrize("space,radius", [("l2", 14.0), ("cosine", 0.9), ("ip", 0.5)])
def test_index_per_query_range_filters_equal_one_single_dict_call_per_query(space, radius):
    rng, index, vecs, gone = _filled(space)
    live = [v for v in vecs if v.id not in gone]
    nq = 24
    qs = rng.standard_normal((nq, 8)).astype(np.float32)
    fs = [random_filter(rng) for _ in range(8)] + [{"genre": "jazz"}, {"genre": "zydeco"}, {}]
    wheres = [None if i % 5 == 0 else fs[int(rng.integers(len(fs)))] for i in range(nq)]
    some = 0
    for max_results in (3, 1024, None):
        got = index.range_search_many(qs, radius, "ns", space, max_results, where=wheres)
        assert len(got) == nq
        for i, w in enumerate(wheres):
            one = index.range_search_many(qs[i:i + 1], radius, "ns", space, max_results, where=w)
            assert ids(got)[i] == ids(one)[0], (i, w)
            by_id = {v.id: v for v in live}
            assert all(w is None or py_match(w, by_id[h.vector_id].metadata) for h in got[i])
            some += len(got[i])
    assert some > 0
    assert ids(index.range_search_many(qs[:3], radius, "ns", space, where=(None, None, None))) == \
        ids(index.range_search_many(qs[:3], radius, "ns", space))
    # a dict and None behave as before: no batched call
    before = EachRangeOracleEngine.each_calls
    index.range_search_many(qs, radius, "ns", space, where={"genre": "jazz"})
    index.range_search_many(qs, radius, "ns", space)
    index.range_search(VectorDTO(values=qs[0].tolist(), metadata={}), radius, "ns", space, where={"genre": "jazz"})
    assert EachRangeOracleEngine.each_calls == before


def test_refusals_come_before_any_native_call():
    _, index, _, _ = _filled()
    qp = QueryProcessor(InMemoryStorage(), index)
    qs = np.zeros((3, 8), np.float32)
    before = EachRangeOracleEngine.each_calls
    with pytest.raises(ValueError, match="3 queries"):
        index.range_search_many(qs, 1.0, "ns", "l2", where=[{"year": 1}, None])
    with pytest.raises(ValueError, match="dict filters or None"):
        index.range_search_many(qs, 1.0, "ns", "l2", where=[None, lambda m: True, None])
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.range_search_many(qs, 1.0, "ns", "l2", where=[None, {"nope": 1}, None])
    with pytest.raises(ValueError):
        index.range_search_many(qs, 1.0, "ns", "l2", where=[None, {"year": "nineteen-ninety"}, None])
    with pytest.raises(ValueError, match="3 queries"):
        qp.find_in_radius_many(qs, 1.0, "ns", "l2", where=[{"year": 1}])
    with pytest.raises(ValueError, match="host path"):
        qp.find_in_radius_many(qs, 1.0, "ns", "l2", where=[None, lambda m: True, None])
    with pytest.raises(ValueError, match="not a declared attribute"):
        qp.find_in_radius_many(qs, 1.0, "ns", "l2", where=[None, {"nope": 1}, None])
    assert EachRangeOracleEngine.each_calls == before
    assert index.range_search_many(qs, 1.0, "other", "l2", where=[None, {"year": 1}, None]) == [[], [], []]


def test_per_query_range_filters_follow_appends_tombstones_and_compaction():
    rng, index, vecs, gone = _filled(seed=5)
    qs = rng.standard_normal((6, 8)).astype(np.float32)
    wheres = [{"genre": "blues"}, None, {"year": {"$gte": 1990}}, {"genre": "blues"}, {"in_stock": True}, {}]

    def check():
        got = index.range_search_many(qs, 12.0, "ns", "l2", where=wheres)
        assert sum(len(g) for g in got) > 0
        for i, w in enumerate(wheres):
            assert ids(got)[i] == ids(index.range_search_many(qs[i:i + 1], 12.0, "ns", "l2", where=w))[0]

    check()
    index.remove([v.id for v in vecs[1::4]], "ns")
    check()
    index.compact("ns")
    check()


def test_query_processor_find_in_radius_many():
    rng = np.random.default_rng(9)
    index = Index(space="cosine", engine_factory=EachRangeOracleEngine, attributes=SCHEMA)
    qp = QueryProcessor(InMemoryStorage(), index)
    qp.upsert_many([VectorDTO(values=rng.standard_normal(6).tolist(), metadata=m) for m in random_metadata(rng, 90)], "ns")
    q = rng.standard_normal((4, 6))
    wheres = [{"genre": "jazz"}, None, {"year": {"$lt": 1990}}, {"genre": "jazz"}]

    def single(i, w, **kw):
        return qp.find_in_radius(VectorDTO(values=q[i].tolist(), metadata={}), 0.8, "ns", where=w, **kw)

    def same(a, b):
        return [(h["id"], h["score"], h["metadata"], np.asarray(h["values"]).tolist()) for h in a] == \
            [(h["id"], h["score"], h["metadata"], np.asarray(h["values"]).tolist()) for h in b]

    got = qp.find_in_radius_many(q, 0.8, "ns", where=wheres)
    assert sum(len(g) for g in got) > 0
    for i, w in enumerate(wheres):
        assert same(got[i], single(i, w)), i
    assert all(same(a, b) for a, b in zip(qp.find_in_radius_many(q, 0.8, "ns", where=tuple(wheres)), got))
    # the single-filter forms: None, a dict, and a predicate on the host path
    for w in (None, {"genre": "jazz"}, lambda m: m.get("genre") == "jazz"):
        many = qp.find_in_radius_many(q, 0.8, "ns", max_results=5, where=w)
        for i in range(4):
            assert same(many[i], single(i, w, max_results=5)), i
