"""Range search over bit codes without a GPU: the header against the binding, the refusal of a null handle, ``Index`` /
``QueryProcessor`` on the model engine, and the kernels' resource report."""
import ctypes as C
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd.index import Index
from mlvectordb_amd.interfaces import VectorDTO
from mlvectordb_amd.query_processor import QueryProcessor
from mlvectordb_amd.storage import InMemoryStorage
from mlvectordb_amd.vector import Vector
from tests.bits_helpers import distances, random_codes
from tests.bits_range_helpers import BitsRangeOracleEngine
from tests.mutate_helpers import UntouchableEngine

ROOT = Path(__file__).resolve().parent.parent
ENTRY = "mlvdb_range_batch_bits"


def test_the_entry_is_declared_bound_guarded_and_refuses_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_bits_range.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == [ENTRY] == sorted(_native.BITS_RANGE_SIGNATURES)
    params = re.search(ENTRY + r"\s*\(([^)]*)\)", text).group(1).split(",")
    assert len(params) == len(_native.BITS_RANGE_SIGNATURES[ENTRY][1]) == 15
    others = [t for n, t in vars(_native).items() if n.endswith("SIGNATURES") and n != "BITS_RANGE_SIGNATURES"]
    assert not any(ENTRY in t for t in others)
    consts = dict(re.findall(r"#define\s+(MLVDB_[A-Z0-9_]+)\s+(-?\d+)", text))
    assert int(consts["MLVDB_BITS_RANGE_MAX_HITS"]) == _native.BITS_RANGE_MAX_HITS == 16384
    api = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    body = re.search(r"^int " + ENTRY + r"\([^)]*\) \{\n(.*?)^\}", api, flags=re.S | re.M).group(1)
    assert body.lstrip().startswith("return guarded(")
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert "kernels_bits_range.hip" in re.search(r"^SRCS = (.*)$", make, flags=re.M).group(1).split()
    assert "../../include/mlvdb_bits_range.h" in make
    lib = _native.load()
    assert lib.mlvdb_abi_version() == 7 == _native.ABI_VERSION
    buf = (C.c_int64 * 4)()
    assert lib.mlvdb_range_batch_bits(C.c_void_p(), 0, buf, 1, 1, 0, 1.0, 1, 1, None, buf, buf, None, buf, buf) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()


# ---------------------------------------------------------------- Index and QueryProcessor on the model engine
def _filled(n=300):
    rng = np.random.default_rng(21)
    codes, base = random_codes(rng, n, 2, alphabet=6)
    metas = [{"sig": c.tobytes(), "year": 2000 + i % 7} for i, c in enumerate(codes)]
    for m in metas[::13]:
        del m["sig"]
    vectors = [Vector(values=rng.standard_normal(8).astype(np.float32).tolist(), metadata=m) for m in metas]
    index = Index(space="cosine", engine_factory=lambda dim, sp: BitsRangeOracleEngine(dim, sp),
                  attributes={"sig": "bits128", "year": "int"})
    index.add(vectors, "ns")
    index.remove([v.id for v in vectors[::5]], "ns")
    rows = [i for i, m in enumerate(metas) if i % 5 and "sig" in m]
    return index, vectors, metas, codes, base, rows


@pytest.mark.parametrize("metric, radius", [("hamming", 60.0), ("hamming", 0), ("jaccard", 0.5), ("jaccard", -1.0)])
def test_index_range_search_bits_against_the_metadata(metric, radius):
    index, vectors, metas, codes, base, rows = _filled()
    queries = np.stack([base[0], base[3], codes[1], codes[2]])
    for where, keep in ((None, lambda m: True), ({"year": {"$gte": 2003}}, lambda m: m["year"] >= 2003)):
        kept = [i for i in rows if keep(metas[i])]
        dist = distances(queries, codes[kept], metric)
        got = index.range_search_bits([q.tobytes() for q in queries], radius, "ns", "sig", metric=metric, where=where)
        counts = index.count_within_bits(queries.view(np.uint8), radius, "ns", "sig", metric=metric, where=where)
        assert counts.dtype == np.int64 and counts.tolist() == [len(hits) for hits in got] == (dist <= radius).sum(axis=1).tolist()
        for q, hits in enumerate(got):
            order = [j for j in np.lexsort((np.array(kept), dist[q])).tolist() if dist[q, j] <= radius]
            assert [(h.vector_id, h.score) for h in hits] == [(vectors[kept[j]].id, float(dist[q, j])) for j in order]
    assert radius < 0 or counts.sum() > 0


def test_overflow_refusals_and_the_query_processor():
    index, vectors, metas, codes, base, rows = _filled()
    q = [base[1].tobytes(), base[0].tobytes()]
    counts = index.count_within_bits(q, 128, "ns", "sig")
    assert counts.tolist() == [len(rows)] * 2
    with pytest.raises(OverflowError, match=f"query 0 has {len(rows)} hits, more than max_hits=50"):
        index.range_search_bits(q, 128, "ns", "sig", max_hits=50)
    assert [len(h) for h in index.range_search_bits(q, 128, "ns", "sig", max_hits=len(rows))] == [len(rows)] * 2
    for radius, kw, match in ((3, dict(by="year"), "needs a bits attribute"), (3, dict(by="nope"), "not a declared attribute"),
                              (3, dict(by="sig", where=[{}]), "one dict filter"),
                              (3, dict(by="sig", metric="l2"), "metric must be one of"),
                              (float("nan"), dict(by="sig"), "radius must be a number"),
                              ("3", dict(by="sig"), "radius must be a number")):
        for entry in (index.range_search_bits, index.count_within_bits):
            with pytest.raises(ValueError, match=match):
                entry(q, radius, "ns", **kw)
    for bad in (0, 16385, True, 2.5):
        with pytest.raises(ValueError, match="max_hits must be an int"):
            index.range_search_bits(q, 3, "ns", "sig", max_hits=bad)
    with pytest.raises(ValueError, match="range_search_bits: query 1: .*8 bytes"):
        index.range_search_bits([q[0], b"\x00" * 8], 3, "ns", "sig")
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    for entry in (sharded.range_search_bits, sharded.count_within_bits):
        with pytest.raises(ValueError, match="row-sharded"):
            entry(q, 3, "ns", "sig")
    assert index.range_search_bits(q, 3, "nowhere", "sig") == [[], []] and not index.count_within_bits(q, 3, "nowhere", "sig").any()
    assert index.range_search_bits([], 3, "ns", "sig") == []
    # QueryProcessor: find_in_radius' return shape
    qp = QueryProcessor(InMemoryStorage(), Index(space="cosine", engine_factory=lambda d, sp: BitsRangeOracleEngine(d, sp),
                                                 attributes={"sig": "bits64", "year": "int"}))
    bits = lambda *on: [int(b in on) for b in range(64)]
    qp.upsert_many([VectorDTO(values=[1.0, float(i)], metadata={"sig": s, "year": i})
                    for i, s in enumerate([bits(0, 1, 2), bits(0, 1), bits(), bits(5, 6, 7, 8)])])
    got = qp.find_in_radius_bits(bits(0, 1, 2), 3, by="sig")
    assert [(h["metadata"]["year"], h["score"]) for h in got] == [(0, 0.0), (1, 1.0), (2, 3.0)]
    assert set(got[0]) == {"id", "values", "metadata", "score"} and list(got[0]["values"]) == [1.0, 0.0]
    many = qp.find_in_radius_bits_many([bits(0, 1), bits()], 0.5, by="sig", metric="jaccard", where={"year": {"$lt": 3}})
    assert [[(h["metadata"]["year"], h["score"]) for h in hits] for hits in many] == [[(1, 0.0), (0, 1 / 3)], [(2, 0.0)]]
    with pytest.raises(ValueError, match="one dict filter"):
        qp.find_in_radius_bits(bits(), 3, by="sig", where=lambda m: True)
    with pytest.raises(OverflowError, match="query 0 has 4 hits"):
        qp.find_in_radius_bits(bits(), 64, by="sig", max_hits=3)


# ---------------------------------------------------------------- the kernels' resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_bits_range_kernels_use_no_scratch(tmp_path):
    """DESIGN 11.22 records the VGPR, SGPR and LDS figures this report gives."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = ROOT / "mlvectordb_amd" / "csrc"
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950",
                          "-Rpass-analysis=kernel-resource-usage", "-c", str(csrc / "kernels_bits_range.hip"), "-o",
                          str(tmp_path / "k.o")], capture_output=True, text=True, cwd=csrc, check=True).stderr
    seen, name = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    hits = {k: v for k, v in seen.items() if "bits_range_" in k}
    # the walk: five group sizes with the queries in registers and one through LDS, each counting and filling; plan; sort
    assert len(hits) == 14 and sum("bits_range_kernel" in k for k in hits) == 12 and not any(hits.values()), seen
