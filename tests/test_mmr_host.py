"""Diversified kNN (include/mlvdb_mmr.h) without a GPU: the NumPy greedy against the definition, the refusals of
``Index.search_many(mmr_lambda=...)`` / ``QueryProcessor.find_similar_many(mmr_lambda=...)``, the default ``fetch_k`` and the
clamps over an oracle engine, and the C ABI's shape."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, VectorDTO, _native
from oracle import exact_scan
from tests.mmr_helpers import MmrOracleEngine, mmr_select, mmr_select_brute, oracle_index
from tests.where_helpers import WhereOracleEngine

ROOT = Path(__file__).resolve().parents[1]
SCHEMA = {"doc": "int", "flag": "bool"}


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_greedy_equals_the_brute_force_enumeration(space):
    rng = np.random.default_rng(5)
    for m, d in ((1, 3), (2, 3), (7, 2), (12, 5)):
        rows = rng.standard_normal((m, d)).astype(np.float32)
        rows[m // 2] = rows[0]  # an exact duplicate
        q = rng.standard_normal((1, d)).astype(np.float32)
        dq = np.sort(exact_scan.exact_distances(q, rows, space)[0], kind="stable")
        order = np.argsort(exact_scan.exact_distances(q, rows, space)[0], kind="stable")
        P = exact_scan.exact_distances(rows[order], rows[order], space)
        for k in (1, 2, m, m + 3):
            for lam in (0.0, 0.3, 0.7, 1.0):
                picks, objs, gap = mmr_select(dq, P, k, lam)
                want_picks, want_objs = mmr_select_brute(dq, P, k, lam)
                assert picks.tolist() == want_picks and objs.tolist() == want_objs
                assert picks.size == min(k, m) == np.unique(picks).size and gap >= 0.0
                assert picks.size == 0 or (picks[0] == 0 and objs[0] == lam * dq[0])
                # a callable P is asked for picked rows only and gives the same answer
                asked = []
                lazy = mmr_select(dq, lambda s: (asked.append(s), P[s])[1], k, lam)
                assert lazy[0].tolist() == want_picks and asked == want_picks[:max(len(want_picks) - 1, 0)]


def test_lambda_one_gives_the_prefix_and_reports_the_gaps():
    rng = np.random.default_rng(6)
    dq = np.sort(rng.random(40))
    P = rng.random((40, 40))
    picks, objs, gap = mmr_select(dq, P, 9, 1.0)
    assert picks.tolist() == list(range(9)) and objs.tolist() == dq[:9].tolist()
    assert gap == np.min(np.diff(dq)[:8])
    assert mmr_select(dq[:1], P[:1, :1], 5, 0.5)[2] == np.inf  # no step ever had a runner-up


def test_duplicates_tie_to_the_lower_position():
    # positions 1 and 2 are copies of each other (equal dq, equal rows of P): the lower one is picked first
    dq = np.array([0.0, 1.0, 1.0, 1.5])
    P = np.array([[0.0, 2.0, 2.0, 1.0], [2.0, 0.0, 0.0, 3.0], [2.0, 0.0, 0.0, 3.0], [1.0, 3.0, 3.0, 0.0]])
    for lam in (0.0, 0.5, 1.0):
        picks, _, gap = mmr_select(dq, P, 2, lam)
        assert picks.tolist() == [0, 1] and gap == 0.0
    # lambda = 0: the copy of a picked row has mind = 0, the worst objective there is: it goes last
    assert mmr_select(dq, P, 4, 0.0)[0].tolist() == [0, 1, 3, 2]


# ---------------------------------------------------------------- refusals, before the engine is touched
class UntouchableEngine(WhereOracleEngine):
    """Fails the test if a search of any kind reaches the engine."""

    def search(self, *a, **kw):
        raise AssertionError("the engine was touched")

    search64 = search_distinct = search_each = search_mmr = search


def _filled(factory=MmrOracleEngine, n=300, d=8, seed=1, space="l2", **kw):
    rng = np.random.default_rng(seed)
    index = Index(space=space, engine_factory=factory, attributes=SCHEMA, **kw)
    metas = [{"doc": int(rng.integers(0, 40)), "flag": bool(i % 2)} for i in range(n)]
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata=m) for r, m in zip(rows, metas)]
    index.add(vecs, "ns")
    return rng, index, vecs, rows, metas


def test_mmr_refusals_are_value_errors_before_the_engine_is_touched():
    _, index, vecs, _, _ = _filled(UntouchableEngine)
    qs = np.zeros((3, 8), np.float32)
    for lam in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"mmr_lambda must lie in \[0, 1\]"):
            index.search_many(qs, 5, "ns", "l2", mmr_lambda=lam)
    with pytest.raises(ValueError, match="top_k must be <= 64"):
        index.search_many(qs, 65, "ns", "l2", mmr_lambda=0.5)
    with pytest.raises(ValueError, match="fetch_k must be <= 1024"):
        index.search_many(qs, 5, "ns", "l2", mmr_lambda=0.5, fetch_k=1025)
    with pytest.raises(ValueError, match="fetch_k must be >= top_k"):
        index.search_many(qs, 5, "ns", "l2", mmr_lambda=0.5, fetch_k=4)
    with pytest.raises(ValueError, match="fetch_k is the candidate count of mmr_lambda"):
        index.search_many(qs, 5, "ns", "l2", fetch_k=20)
    with pytest.raises(ValueError, match="distinct= cannot be combined"):
        index.search_many(qs, 5, "ns", "l2", mmr_lambda=0.5, distinct="doc")
    with pytest.raises(ValueError, match="give a dict where"):
        index.search_many(qs, 5, "ns", "l2", mmr_lambda=0.5, allowed_ids=[vecs[0].id])
    with pytest.raises(ValueError, match="per-query where list"):
        index.search_many(qs, 5, "ns", "l2", mmr_lambda=0.5, where=[None, {"doc": 1}, None])
    with pytest.raises(ValueError, match="not a declared attribute"):
        index.search_many(qs, 5, "ns", "l2", mmr_lambda=0.5, where={"nope": 1})
    qp = QueryProcessor(InMemoryStorage(), index)
    with pytest.raises(ValueError, match="give a dict where"):
        qp.find_similar_many(qs, 5, "ns", mmr_lambda=0.5, where=lambda m: True)
    with pytest.raises(ValueError, match="top_k must be <= 64"):
        qp.find_similar_many(qs, 100, "ns", mmr_lambda=0.5)
    with pytest.raises(ValueError, match="fetch_k is the candidate count of mmr_lambda"):
        qp.find_similar_many(qs, 5, "ns", fetch_k=20)
    with pytest.raises(ValueError, match="distinct= cannot be combined"):
        qp.find_similar_many(qs, 5, "ns", mmr_lambda=0.5, distinct="doc")


def test_mmr_on_a_row_sharded_index_is_refused():
    sharded = Index(space="l2", devices=[0, 0], engine_factory=UntouchableEngine)
    with pytest.raises(ValueError, match="row-sharded"):
        sharded.search_many(np.zeros((1, 4), np.float32), 3, "ns", "l2", mmr_lambda=0.5)


# ---------------------------------------------------------------- Index / QueryProcessor over the oracle engine
class RecordingEngine(MmrOracleEngine):
    calls = []

    def search_mmr(self, queries, k, fetch_k, lam, where=None, want64=False):
        RecordingEngine.calls.append((k, fetch_k, lam, where is not None))
        return super().search_mmr(queries, k, fetch_k, lam, where=where, want64=want64)


def test_default_fetch_k_and_the_clamps_to_the_live_count():
    assert [Index._default_fetch_k(k) for k in (1, 4, 5, 6, 64)] == [20, 20, 20, 24, 256]
    assert Index._default_fetch_k(300) == 1024
    rng, index, vecs, rows, _ = _filled(RecordingEngine, n=30)
    qs = rng.standard_normal((2, 8)).astype(np.float32)
    RecordingEngine.calls.clear()
    index.search_many(qs, 3, "ns", "l2", mmr_lambda=0.25)              # default 20 <= 30 live
    index.search_many(qs, 10, "ns", "l2", mmr_lambda=0.25)             # default 40 -> 30 live
    index.search_many(qs, 10, "ns", "l2", mmr_lambda=0.25, fetch_k=12)
    index.search_many(qs, 64, "ns", "l2", mmr_lambda=1, fetch_k=1024)  # both clamp to the live count
    index.remove([v.id for v in vecs[:25]], "ns")
    got = index.search_many(qs, 10, "ns", "l2", mmr_lambda=0.25, where={"flag": True})
    assert RecordingEngine.calls == [(3, 20, 0.25, False), (10, 30, 0.25, False), (10, 12, 0.25, False),
                                     (30, 30, 1.0, False), (5, 5, 0.25, True)]
    assert got.counts.tolist() == [3, 3]  # of the live rows 25..29 the odd ones match: the padding says how many
    assert [len(hits) for hits in index.search_many(qs, 10, "other", "l2", mmr_lambda=0.5)] == [0, 0]
    assert [len(hits) for hits in index.search_many(qs, 0, "ns", "l2", mmr_lambda=0.5)] == [0, 0]


def test_index_mmr_returns_the_greedy_picks_in_pick_order_with_the_plain_scores():
    rng, index, vecs, rows, metas = _filled(space="cosine")
    qs = rng.standard_normal((5, 8)).astype(np.float32)
    plain = index.search_many(qs, 40, "ns", "cosine")
    score_of = [{h.vector_id: h.score for h in hits} for hits in plain]
    for where, allowed in ((None, np.ones(len(metas), bool)), ({"flag": True}, np.array([m["flag"] for m in metas]))):
        got = index.search_many(qs, 6, "ns", "cosine", mmr_lambda=0.3, fetch_k=40, where=where)
        sub = np.flatnonzero(allowed)
        dist = exact_scan.exact_distances(qs, rows[sub], "cosine")
        for i, hits in enumerate(got):
            order = np.lexsort((sub, dist[i]))[:40]
            P = exact_scan.exact_distances(rows[sub[order]], rows[sub[order]], "cosine")
            picks, _, _ = mmr_select(dist[i, order], P, 6, 0.3)
            assert [h.vector_id for h in hits] == [vecs[j].id for j in sub[order][picks]]
            if where is None:
                assert [h.score for h in hits] == [score_of[i][h.vector_id] for h in hits]
    # lambda = 1 is the plain search; without mmr_lambda nothing changed
    one = index.search_many(qs, 6, "ns", "cosine", mmr_lambda=1.0, fetch_k=40)
    assert np.array_equal(one.labels, plain.labels[:, :6]) and np.array_equal(one.scores, plain.scores[:, :6])


def test_query_processor_mmr_returns_enriched_hits_in_pick_order():
    rng = np.random.default_rng(4)
    qp = QueryProcessor(InMemoryStorage(), oracle_index({"doc": "int"}, space="cosine"))
    qp.upsert_many([VectorDTO(values=rng.standard_normal(6).tolist(), metadata={"doc": int(i % 9), "i": i})
                    for i in range(120)], "ns")
    qs = rng.standard_normal((4, 6))
    out = qp.find_similar_many(qs, 5, "ns", mmr_lambda=0.2, fetch_k=30)
    plain = qp.find_similar_many(qs, 30, "ns")
    for hits, near in zip(out, plain):
        assert len(hits) == 5 == len({h["id"] for h in hits}) and hits[0]["id"] == near[0]["id"]
        scores = {h["id"]: h["score"] for h in near}
        assert all(h["score"] == scores[h["id"]] for h in hits)
    only = qp.find_similar_many(qs, 5, "ns", mmr_lambda=0.2, where={"doc": 3})
    assert all(h["metadata"]["doc"] == 3 for hits in only for h in hits) and all(len(hits) == 5 for hits in only)


# ---------------------------------------------------------------- C ABI
def _header_text():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_mmr.h").read_text(), flags=re.S)


def test_mmr_header_declares_what_the_binding_binds():
    lib = _native.load()
    names = sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", _header_text())))
    assert names == ["mlvdb_search_batch_mmr"] == sorted(_native.MMR_SIGNATURES)
    assert hasattr(lib, names[0])
    known = (set(_native.SIGNATURES) | set(_native.WHERE_SIGNATURES) | set(_native.WHERE_EACH_SIGNATURES) |
             set(_native.DISTINCT_SIGNATURES) | set(_native.FACET_SIGNATURES) | set(_native.ORDER_SIGNATURES))
    assert not set(names) & known
    params = re.search(r"mlvdb_search_batch_mmr\((.*?)\);", _header_text(), flags=re.S).group(1).split(",")
    restype, argtypes = _native.MMR_SIGNATURES[names[0]]
    assert len(params) == len(argtypes) == 13 and restype is C.c_int
    assert argtypes[3:6] == [C.c_int32, C.c_int32, C.c_double] and "double lambda" in params[5]
    assert int(re.search(r"#define MLVDB_MMR_MAX_FETCH (\d+)", _header_text()).group(1)) == _native.MMR_MAX_FETCH == 1024
    assert lib.mlvdb_abi_version() == 7


def _entry_body():
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    return re.search(r"^int mlvdb_search_batch_mmr\([^)]*\) \{\n(.*?)^\}", text, flags=re.S | re.M).group(1)


def test_mmr_entry_refuses_a_null_handle_inside_the_exception_guard():
    lib = _native.load()
    buf = (C.c_double * 4)()
    assert lib.mlvdb_search_batch_mmr(C.c_void_p(), buf, 1, 1, 1, 0.5, None, buf, buf, buf, buf, buf, buf) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    assert _entry_body().lstrip().startswith("return guarded(")


def test_the_source_shows_every_validation_before_the_first_launch():
    body = _entry_body()
    first_launch = min(body.index(word) for word in ("where_run(", "mmr_impl(", "with_row_mask("))
    checks = ["check_handle(h)", "nq < 0", "k < 1", "k > MLVDB_MAX_TOPK", "fetch_k < k", "fetch_k > kMmrMaxFetch",
              "!(lambda >= 0.0 && lambda <= 1.0)", "mmr_select_lds(h->ld, fetch_k) > 64 * 1024", "!queries || !out_labels"]
    at = [body.index(c) for c in checks]
    assert at == sorted(at) and at[-1] < first_launch
    unsupported = [line.split("return fail")[0].strip() for line in body.replace("\n        return", " return").splitlines()
                   if "MLVDB_ERR_UNSUPPORTED" in line]
    assert [u[4:-1] for u in unsupported] == ["k > MLVDB_MAX_TOPK", "fetch_k > kMmrMaxFetch",
                                                "mmr_select_lds(h->ld, fetch_k) > 64 * 1024"]
    text = (ROOT / "mlvectordb_amd" / "csrc" / "api.hip").read_text()
    impl = re.search(r"^int mmr_impl\(.*?^\}", text, flags=re.S | re.M).group(0)
    assert "hipLaunchKernelGGL" not in body and "<<<" not in body
    assert impl.index("search_device_impl(") < impl.index("launch_mmr_select(") < impl.index("copy_down(")
    down = re.search(r"^int copy_down\(.*?^\}", text, flags=re.S | re.M).group(0)  # wait, copy each output down, wait
    assert down.index("hipStreamSynchronize") < down.index("hipMemcpyDeviceToHost")
    assert down.rindex("hipMemcpyDeviceToHost") < down.rindex("hipStreamSynchronize")
    assert "const double one_minus_lambda = 1.0 - lambda;" in impl  # formed once, on the host


def test_the_mmr_kernel_and_header_are_in_the_build():
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bkernels_mmr\.hip\b", make, flags=re.M)
    assert "mlvdb_mmr.h" in make and "-ffp-contract=off" in make
    kern = (ROOT / "mlvectordb_amd" / "csrc" / "kernels_mmr.hip").read_text()
    assert "accumulate_rows<SPACE, 1, 1, 8>" in kern and "query_aux_from_sums" in kern
    assert "atomicAdd" not in kern and "atomicMin" not in kern and "atomicCAS" not in kern
    layout = (ROOT / "mlvectordb_amd" / "csrc" / "kernels_layout.hip").read_text()
    assert "query_aux_from_sums(red, space)" in layout  # the query prep and the selection share one norm term
