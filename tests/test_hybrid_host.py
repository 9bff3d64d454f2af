"""Hybrid search without a GPU: the header against the binding, the C entry's refusal of a null handle, ``Index`` /
``QueryProcessor`` on the model engine of tests/hybrid_helpers.py, every refusal before the engine is touched, the default
fetch sizes, and the new kernels' resource report."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mlvectordb_amd
from mlvectordb_amd import _native
from mlvectordb_amd.index import BatchHits, HybridBatchHits, Index
from mlvectordb_amd.interfaces import VectorDTO
from mlvectordb_amd.query_processor import QueryProcessor
from mlvectordb_amd.storage import InMemoryStorage
from mlvectordb_amd.vector import Vector
from tests.hybrid_helpers import METHODS, HybridOracleEngine, fuse_one
from tests.mutate_helpers import UntouchableEngine
from tests.sparse_helpers import dense_scores, random_corpus, random_vector

ROOT = Path(__file__).resolve().parent.parent
SCHEMA = {"lexical": "sparse", "year": "int", "tags": "str[]"}
DIM = 8


# ---------------------------------------------------------------- the C ABI without a device
def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_hybrid.h").read_text(), flags=re.S)


def test_the_entry_is_declared_bound_and_refuses_a_null_handle():
    text = _header()
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(_native.HYBRID_SIGNATURES) == ["mlvdb_search_batch_hybrid"]
    others = [t for n, t in vars(_native).items() if n.endswith("SIGNATURES") and n != "HYBRID_SIGNATURES"]
    assert len(others) >= 14 and not any(set(names) & set(t) for t in others)
    params = re.search(r"mlvdb_search_batch_hybrid\s*\(([^)]*)\)", text).group(1).split(",")
    assert len(params) == len(_native.HYBRID_SIGNATURES["mlvdb_search_batch_hybrid"][1]) == 22
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert {m: int(consts["MLVDB_FUSE_" + m.upper()]) for m in METHODS} == _native.FUSE_CODES == {"rrf": 0, "linear": 1, "relative": 2}
    assert int(consts["MLVDB_HYBRID_MAX_FETCH_DENSE"]) == _native.HYBRID_MAX_FETCH_DENSE == Index._MAX_FETCH_K_HYBRID == 1024
    api = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    assert int(re.search(r"kSparseChunk = (\d+);", (ROOT / "mlvectordb_amd" / "csrc" / "internal.h").read_text()).group(1)) \
        == _native.HYBRID_CHUNK and "kHybridChunk = kSparseChunk" in api
    lib = _native.load()
    assert lib.mlvdb_abi_version() == 7 == _native.ABI_VERSION
    buf = (C.c_int64 * 8)()
    rc = lib.mlvdb_search_batch_hybrid(C.c_void_p(), buf, 0, buf, buf, buf, 1, 1, 1, 1, 0, 1.0, 1.0, 60.0, None, buf, buf, buf,
                                       None, None, None, None)
    assert rc == 1 and b"null index handle" in lib.mlvdb_last_global_error()  # MLVDB_ERR_INVALID_ARG


def test_the_entry_is_guarded_and_the_header_says_what_the_issue_fixes():
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    body = re.search(r"^int mlvdb_search_batch_hybrid\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)
    assert body.lstrip().startswith("return guarded(")
    header = (ROOT / "include" / "mlvdb_hybrid.h").read_text()
    assert "COMPLETED UNION C, not over each leg's own list" in header and "no special case" in header
    assert "HybridBatchHits" in mlvectordb_amd.__all__ and mlvectordb_amd.HybridBatchHits is HybridBatchHits


# ---------------------------------------------------------------- Index and QueryProcessor on the model engine
def _index(engine=HybridOracleEngine, space="l2"):
    return Index(space=space, engine_factory=lambda dim, sp: engine(dim, sp), attributes=SCHEMA)


def _filled(seed=5, n=160, vocab=48):
    rng = np.random.default_rng(seed)
    rows = random_corpus(rng, n, vocab, exact=True)
    metas = [{"lexical": r, "year": 2000 + i % 7, "tags": ["a"] if i % 2 else []} for i, r in enumerate(rows)]
    for m in metas[::13]:
        del m["lexical"]  # a missing key is absent too
    values = rng.integers(-4, 5, (n, DIM)).astype(np.float32)
    vectors = [Vector(values=v.tolist(), metadata=m) for v, m in zip(values, metas)]
    index = _index()
    index.add(vectors[:100], "ns")
    index.add(vectors[100:], "ns")
    return rng, index, vectors, metas, values


def _expect(q, sq, values, metas, live, k, fd, fs, method, weights, c, keep=lambda m: True):
    """The model's answer straight from the rows and the metadata dicts: per query (labels, fused, dd, ss, rd, rs)."""
    rows = [m.get("lexical") for m in metas]
    clean = [None if r is None else {t: w for t, w in r.items() if w != 0} for r in rows]
    scores, _ = dense_scores(sq, clean)
    ok = np.array([live[i] and keep(metas[i]) for i in range(len(metas))], dtype=bool)
    have = ok & np.array([r is not None for r in clean])
    out = []
    for i in range(len(sq)):
        d = ((q[i].astype(np.float64)[None, :] - values.astype(np.float64)) ** 2).sum(axis=1)  # (small integers: exact)
        idx = np.flatnonzero(ok)
        dl = idx[np.lexsort((idx, d[idx]))][:fd]
        idx = np.flatnonzero(have)
        sl = idx[np.lexsort((idx, -scores[i, idx]))][:fs]
        out.append(fuse_one(dl, d[dl], sl, scores[i, sl], lambda lab: d[lab], lambda lab: scores[i, lab], k, method,
                            weights[0], weights[1], c))
    return out


def test_index_search_hybrid_against_the_rows_and_the_metadata():
    rng, index, vectors, metas, values = _filled()
    live = [True] * len(vectors)
    q = rng.integers(-4, 5, (5, DIM)).astype(np.float32)
    sq = [random_vector(rng, n, 48, exact=True) for n in (1, 3, 8, 20)] + [{}]

    def check(method, where=None, keep=lambda m: True, k=10, fetch_k=None, fetch_k_sparse=None, weights=(1.0, 1.0), c=60.0):
        got = index.search_hybrid(q, sq, k, "ns", "l2", "lexical", fusion=method, weights=weights, rrf_k=c, fetch_k=fetch_k,
                                  fetch_k_sparse=fetch_k_sparse, where=where, components=True)
        active = sum(live)
        fd = min(Index._default_fetch_k(k) if fetch_k is None else fetch_k, active)
        fs = min(min(64, max(k, 20)) if fetch_k_sparse is None else fetch_k_sparse, active)
        want = _expect(q, sq, values, metas, live, min(k, active), fd, fs, method, weights, c, keep)
        assert isinstance(got, HybridBatchHits) and got.scores.dtype == np.float64
        for i, (lab, fused, dd, ss, rd, rs) in enumerate(want):
            n = lab.size
            assert got.counts[i] == n and got.labels[i, :n].tolist() == lab.tolist(), (method, i)
            for name, arr in (("scores", fused), ("dense", dd), ("sparse", ss)):
                assert getattr(got, name)[i, :n].tobytes() == arr.tobytes(), (method, i, name)
            assert got.rank_dense[i, :n].tolist() == rd.tolist() and got.rank_sparse[i, :n].tolist() == rs.tolist()
            assert [h.vector_id for h in got[i]] == [vectors[l].id for l in lab.tolist()]
        plain = index.search_hybrid(q, sq, k, "ns", "l2", "lexical", fusion=method, weights=weights, rrf_k=c, fetch_k=fetch_k,
                                    fetch_k_sparse=fetch_k_sparse, where=where)
        assert type(plain) is BatchHits and plain == got and plain.scores.tobytes() == got.scores.tobytes()
        return got

    for method in METHODS:
        check(method)
        check(method, {"year": {"$gte": 2003}}, lambda m: m["year"] >= 2003, weights=(0.5, 2.0), c=1.0)
        check(method, {"tags": "a"}, lambda m: "a" in m["tags"], k=64, fetch_k=30, fetch_k_sparse=40)
        check(method, {"lexical": {"$exists": True}}, lambda m: m.get("lexical") is not None, k=3, fetch_k=2, fetch_k_sparse=1)
    index.remove([v.id for v in vectors[::5]], "ns")
    live = [i % 5 != 0 for i in range(len(vectors))]
    for method in METHODS:
        got = check(method, k=64, fetch_k=1024, fetch_k_sparse=64)  # (clamped to the live rows)
        assert (got.rank_sparse == -1).any() and (got.rank_dense >= 0).all()
    assert index.search_hybrid(np.zeros((0, DIM), np.float32), [], 5, "ns", "l2", "lexical").labels.shape[0] == 0
    assert index.search_hybrid(q, sq, 5, "nowhere", "l2", "lexical") == [[] for _ in sq]
    assert index.search_hybrid(q, sq, 0, "ns", "l2", "lexical", components=True).dense.shape == (5, 0)


def test_the_default_fetch_sizes():
    seen = []

    class Spy(HybridOracleEngine):
        def search_hybrid(self, queries, attr, sparse_queries, k, fetch_dense, fetch_sparse, **kw):
            seen.append((k, fetch_dense, fetch_sparse, kw["method"], kw["weights"], kw["rrf_k"]))
            return super().search_hybrid(queries, attr, sparse_queries, k, fetch_dense, fetch_sparse, **kw)

    index = _index(engine=Spy)
    rng = np.random.default_rng(2)
    index.add([Vector(values=rng.integers(-3, 4, DIM).astype(np.float32).tolist(), metadata={"lexical": {i % 9: 1.0}})
               for i in range(300)], "ns")
    q, sq = np.ones((1, DIM), np.float32), [{1: 1.0}]
    for top_k, want in ((1, (1, 20, 20)), (5, (5, 20, 20)), (10, (10, 40, 20)), (30, (30, 120, 30)), (64, (64, 256, 64))):
        index.search_hybrid(q, sq, top_k, "ns", "l2", "lexical")
        assert seen[-1] == want + ("rrf", (1.0, 1.0), 60.0)
    index.search_hybrid(q, sq, 64, "ns", "l2", "lexical", fetch_k=1024, fetch_k_sparse=64, fusion="linear", weights=(2, 0), rrf_k=0)
    assert seen[-1] == (64, 300, 64, "linear", (2.0, 0.0), 0.0)  # clamped to the live row count
    index.remove([v for v in index._ns["ns"].ids.uuids_at(np.arange(290))], "ns")
    index.search_hybrid(q, sq, 64, "ns", "l2", "lexical")
    assert seen[-1][:3] == (10, 10, 10)
    assert Index._default_fetch_k_sparse(0) == 20 and Index._default_fetch_k_sparse(1000) == 64


def test_every_refusal_happens_before_the_engine_is_touched():
    index = _index(engine=UntouchableEngine)
    index._get_or_create("ns", DIM, "l2")  # a namespace whose engine refuses every call
    q, sq = np.ones((2, DIM), np.float32), [{1: 1.0}, {2: 1.0}]
    bad_q = q.copy()
    bad_q[1, 3] = np.nan
    cases = [
        (dict(by="year"), "needs a sparse attribute"),
        (dict(by="nope"), "not a declared attribute"),
        (dict(by=None), "not a declared attribute"),
        (dict(where=lambda m: True), "one dict filter"),
        (dict(where=[{}]), "one dict filter"),
        (dict(where={"lexical": 3}), "sparse"),
        (dict(fusion="max"), "fusion must be one of"),
        (dict(weights=(-1.0, 1.0)), "finite and >= 0"),
        (dict(weights=(1.0, float("nan"))), "finite and >= 0"),
        (dict(weights=(float("inf"), 1.0)), "finite and >= 0"),
        (dict(weights=(1.0,)), "pair of numbers"),
        (dict(weights="ab"), "pair of numbers"),
        (dict(rrf_k=-1), "rrf_k must be finite"),
        (dict(rrf_k=float("nan")), "rrf_k must be finite"),
        (dict(top_k=65), "top_k must be <= 64"),
        (dict(fetch_k=1025), r"fetch_k must lie in \[1, 1024\]"),
        (dict(fetch_k=0), r"fetch_k must lie in \[1, 1024\]"),
        (dict(fetch_k_sparse=65), r"fetch_k_sparse must lie in \[1, 64\]"),
        (dict(fetch_k_sparse=0), r"fetch_k_sparse must lie in \[1, 64\]"),
        (dict(top_k=10, fetch_k=4, fetch_k_sparse=5), r"top_k must be <= fetch_k \+ fetch_k_sparse"),
        (dict(sparse_queries=sq[:1]), "2 dense queries but 1 sparse queries"),
        (dict(sparse_queries={1: 1.0}), "wrap it in a list"),
        (dict(sparse_queries=[{1: 1.0}, {1: float("nan")}]), "finite"),
        (dict(sparse_queries=[{1: 1.0}, {t: 1.0 for t in range(1025)}]), "1025 nonzeros"),
        (dict(sparse_queries=[{1: 1.0}, {-1: 1.0}]), "outside"),
        (dict(queries=bad_q), "non-finite"),
    ]
    for kw, match in cases:
        args = dict(queries=q, sparse_queries=sq, top_k=3, namespace="ns", metric="l2", by="lexical")
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            index.search_hybrid(**args)
    with pytest.raises(ValueError, match="row-sharded"):
        sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
        sharded.search_hybrid(q, sq, 3, "ns", "l2", "lexical")
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="one dict filter"):
        qp.find_similar_hybrid_many(q, sq, 3, "ns", "l2", "lexical", where=lambda m: True)


def test_query_processor_find_similar_hybrid():
    qp = QueryProcessor(InMemoryStorage(), _index(space="cosine"))
    metas = [{"lexical": {1: 1.0, 2: 0.5}, "year": 1, "note": "x"}, {"lexical": {2: 2.0}, "year": 2}, {"lexical": {}, "year": 3},
             {"year": 4}, {"lexical": {1: -1.0}, "year": 5}]
    rows = np.eye(5, DIM, dtype=np.float32)
    qp.upsert_many([VectorDTO(values=r.tolist(), metadata=m) for r, m in zip(rows, metas)])
    # dense order by distance to e3: year 4 first, then the rest by label; sparse order for {1: 2, 2: 1}: years 1, 2, 3, 5
    got = qp.find_similar_hybrid(VectorDTO(values=rows[3].tolist(), metadata={}), {1: 2.0, 2: 1.0}, 3, by="lexical", rrf_k=0.0)
    want = {1: 1 / 2 + 1 / 1, 2: 1 / 3 + 1 / 2, 3: 1 / 4 + 1 / 3, 4: 1 / 1, 5: 1 / 5 + 1 / 4}
    top = sorted(want, key=lambda y: -want[y])[:3]
    assert [(h["metadata"]["year"], h["score"]) for h in got] == [(y, want[y]) for y in top] and top == [1, 4, 2]
    assert set(got[0]) == {"id", "values", "metadata", "score"} and got[0]["metadata"]["note"] == "x"
    many = qp.find_similar_hybrid_many(rows[:2], [{2: 1.0}, ([1], [1.0])], 2, by="lexical", fusion="linear", weights=(0.0, 1.0),
                                       where={"year": {"$lt": 5}})
    assert [[h["metadata"]["year"] for h in hits] for hits in many] == [[2, 1], [1, 2]]
    assert [[h["score"] for h in hits] for hits in many] == [[2.0, 0.5], [1.0, 0.0]]


# ---------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_hybrid_kernels_compile_for_gfx950_without_scratch(tmp_path):
    """DESIGN 11.14 records the VGPR, SGPR and LDS figures this report gives."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "mlvectordb_amd" / "csrc"
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(csrc / "kernels_hybrid.hip"), "-o",
                          str(tmp_path / "k.o")], capture_output=True, text=True, cwd=csrc, check=True).stderr
    seen, lds, name = {}, {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    for kernel in ("hybrid_union_kernel", "sparse_pair_score_kernel", "hybrid_fuse_kernel"):
        hits = [v for k, v in seen.items() if kernel in k]
        assert hits and all(v == 0 for v in hits), (kernel, seen)
        assert all(v <= 64 * 1024 for k, v in lds.items() if kernel in k), (kernel, lds)
    # the fold and the bitmap are the scan's own: one header, included by both files, defined in neither
    shared = (csrc / "sparse_dpp.h").read_text()
    assert "row16_sum" in shared and "dpp_f64" in shared and "kSparseBitmapBits = 8192" in shared
    for unit in ("kernels_sparse.hip", "kernels_hybrid.hip"):
        text = (csrc / unit).read_text()
        assert '#include "sparse_dpp.h"' in text and "double row16_sum(" not in text and "row16_sum(" in text, unit
