"""Diversified kNN on the MI355X (include/mlvdb_mmr.h).
1. Replay: the greedy of tests/mmr_helpers.py run on the device's own bits -- the candidate list of ``search64`` at fetch_k and
   D(s, i) from ``pair_distances(get_rows_at(cands), cands)`` -- must reproduce ``search_mmr`` bit for bit (labels, ranks,
   counts, objectives, and the candidate list's distances).  No tolerance: it holds for any input, near-ties included.
2. Against the NumPy oracle (``exact_scan.exact_distances`` for both distances): equal picks, under the precondition --
   asserted on the CPU for every query -- that no step's best and runner-up objectives are closer than 1e-9.
3. Structure: lambda = 1, fetch_k = k, duplicates, where programs, mutations, more queries than one chunk.
4. The Index / QueryProcessor surface.
Rows are Gaussian; exact duplicates are copies of rows."""
import functools

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, VectorDTO, _native
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.conftest import dump_mismatch
from tests.helpers import SCORE_ATOL
from tests.mmr_helpers import D64_BOUND, GAP_MIN, mmr_from_candidates, mmr_select
from tests.where_helpers import SCHEMA, py_match, random_filter, random_metadata

pytestmark = pytest.mark.gpu

LAMBDAS = (0.0, 0.3, 1.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def _device_pairs(eng, cl, cc):
    """P[q][s][i] = D(s, i) by the device: the stored values of candidate s as the query, candidate i as the row."""
    out = {}
    for i in range(cl.shape[0]):
        m = int(cc[i])
        if m:
            cands = cl[i, :m]
            out[i] = eng.pair_distances(eng.get_rows_at(cands), np.broadcast_to(cands, (m, m)))[0]
    return out


def _replay(eng, qs, k, fetch_k, lams, tag, where=None):
    """``search_mmr`` against the greedy replayed on the device's own candidate lists and pair distances."""
    cl, cd32, cc, cd64 = eng.search64(qs, fetch_k, where=where)
    P = _device_pairs(eng, cl, cc)
    names = ("labels", "dist", "counts", "d64", "rank", "objective")
    got = None
    for lam in lams:
        got = eng.search_mmr(qs, k, fetch_k, lam, where=where, want64=True)
        want, _ = mmr_from_candidates(cl, cd32, cc, cd64, lambda i, _: P[i], k, lam)
        for name, g, w in zip(names, got, want):
            if g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
                dump_mismatch(f"mmr_{tag}_{lam}", **{f"got_{n}": a for n, a in zip(names, got)},
                              **{f"want_{n}": a for n, a in zip(names, want)}, cl=cl, cd64=cd64, cc=cc)
                bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))
                raise AssertionError(f"{tag} lambda={lam}: {name} differs in {bad.size} queries, first {bad[0]}: "
                                     f"got {g[bad[0]]} want {w[bad[0]]}")
        assert np.array_equal(got[2], np.minimum(cc, k))
        without = eng.search_mmr(qs, k, fetch_k, lam, where=where)
        assert without[3] is None and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(without[:3], got[:3]))
    return got


# ---------------------------------------------------------------- 1. replay of the device's own bits
SIZES = (1, 5, 17, 1000, 5000)
# every (k, fetch_k) of the contract's edges with a batch size: 1 / 9 / 70 queries; the quadratic pair matrices of the long
# lists stay at 9 queries
SHAPES = (((1, 1), 1), ((2, 2), 9), ((1, 17), 70), ((16, 16), 9), ((17, 63), 70), ((64, 64), 9), ((63, 65), 1),
          ((10, 255), 70), ((64, 257), 9), ((64, 1024), 9))


@pytest.mark.parametrize("d", [3, 64, 200])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_search_mmr_equals_the_greedy_replayed_on_the_devices_own_bits(space, d):
    rng = np.random.default_rng(2000 * d + len(space))
    qs = rng.standard_normal((70, d), dtype=np.float32)
    for n in SIZES:
        rows = rng.standard_normal((n, d), dtype=np.float32)
        tomb = rng.random(n) < 0.10
        tomb[0] = False  # (a live row is left at every size)
        eng = HipScanEngine(d, space, device=0)
        try:
            eng.append(rows)
            if tomb.any():
                eng.tombstone(np.flatnonzero(tomb))
            live = int((~tomb).sum())
            for (k, fetch_k), nq in SHAPES:
                got = _replay(eng, qs[:nq], k, fetch_k, LAMBDAS, f"replay_{space}_{d}_n{n}_q{nq}_k{k}_f{fetch_k}")
                assert got[2].tolist() == [min(k, live)] * nq  # m < fetch_k whenever the index is short
                assert not tomb[got[0][got[0] >= 0]].any()
        finally:
            eng.close()


# ---------------------------------------------------------------- 2. against the NumPy oracle
ORACLE_LAMBDAS = (0.0, 0.3, 0.7)


@functools.lru_cache(maxsize=None)
def _oracle_case(space, d):
    """rows, queries and, per lambda, the oracle's six outputs and per-query gaps -- all on the CPU, computed once."""
    rng = np.random.default_rng(7 * d + len(space))
    n, nq, fetch_k, k = 5000, 24, 1024, 64
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    dist = exact_scan.exact_distances(qs, rows, space)
    labels = np.arange(n)
    cl = np.stack([np.lexsort((labels, dist[i]))[:fetch_k] for i in range(nq)]).astype(np.int64)
    cd64 = np.take_along_axis(dist, cl, axis=1)
    cc = np.full(nq, fetch_k, np.int32)
    memo = {}

    def pair_rows(i, cands):
        def row(s):  # D(s, .): candidate s as the query -- asked for picked rows only
            key = (i, int(s))
            if key not in memo:
                memo[key] = exact_scan.exact_distances(rows[cands[s]][None, :], rows[cands], space)[0]
            return memo[key]
        return row

    out = {}
    for lam in ORACLE_LAMBDAS:
        out[lam] = mmr_from_candidates(cl, cd64.astype(np.float32), cc, cd64, pair_rows, k, lam)
    return rows, qs, fetch_k, k, out


@pytest.mark.parametrize("d", [3, 64, 200])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_search_mmr_equals_the_numpy_oracle_where_no_step_is_a_near_tie(space, d):
    rows, qs, fetch_k, k, oracle = _oracle_case(space, d)
    # the precondition, for every query of the case, before the device is asked anything
    for lam in ORACLE_LAMBDAS:
        gaps = oracle[lam][1]
        print(f"{space} d={d} lambda={lam}: smallest objective gap {gaps.min():.3e}")
        assert gaps.shape == (qs.shape[0],) and (gaps >= GAP_MIN).all(), (lam, gaps.min())
    eng = HipScanEngine(d, space, device=0)
    try:
        eng.append(rows)
        for lam in ORACLE_LAMBDAS:
            (wl, _, wc, wd64, wrank, _), _ = oracle[lam]
            lab, dist, cnt, d64, rank, obj = eng.search_mmr(qs, k, fetch_k, lam, want64=True)
            if not (np.array_equal(lab, wl) and np.array_equal(rank, wrank) and np.array_equal(cnt, wc)):
                dump_mismatch(f"mmr_oracle_{space}_{d}_{lam}", lab=lab, wl=wl, rank=rank, wrank=wrank, d64=d64, wd64=wd64)
                bad = np.flatnonzero((lab != wl).any(axis=1))
                raise AssertionError(f"lambda={lam}: picks differ in {bad.size} queries, first {bad[0]}: got {rank[bad[0]]} "
                                     f"want {wrank[bad[0]]}")
            err = float(np.abs(d64 - wd64).max())
            print(f"{space} d={d} lambda={lam}: max |d64 - oracle| = {err:.3e}")
            assert err <= D64_BOUND, err  # the premise of GAP_MIN's derivation
            assert err <= SCORE_ATOL
            # (the fp32 output is the fp64 distance rounded once; an absolute 1e-5 cannot be asked of fp32 itself beyond 128)
            assert np.array_equal(_bits(dist), _bits(d64.astype(np.float32)))
    finally:
        eng.close()


# ---------------------------------------------------------------- 3. structure
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_lambda_one_is_the_prefix_and_fetch_k_equal_k_a_permutation_of_the_plain_search(space):
    rng = np.random.default_rng(31)
    d, n, nq = 40, 3000, 20
    eng = HipScanEngine(d, space, device=0)
    try:
        eng.append(rng.standard_normal((n, d), dtype=np.float32))
        eng.tombstone(rng.choice(n, n // 10, replace=False))
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        for k, fetch_k in ((1, 1), (7, 100), (64, 64), (64, 1024)):
            pl, pd32, pc, pd64 = eng.search64(qs, fetch_k)
            lab, dist, cnt, d64, rank, obj = eng.search_mmr(qs, k, fetch_k, 1.0, want64=True)
            assert np.array_equal(lab, pl[:, :k]) and np.array_equal(cnt, np.minimum(pc, k))
            assert np.array_equal(_bits(dist), _bits(pd32[:, :k])) and np.array_equal(_bits(d64), _bits(pd64[:, :k]))
            assert np.array_equal(rank, np.broadcast_to(np.arange(k, dtype=np.int32), (nq, k)))
            assert np.array_equal(_bits(obj), _bits(pd64[:, :k]))  # 1.0 * dq - 0.0 * mind
        for k in (2, 17, 64):
            pl, _, _, pd64 = eng.search64(qs, k)
            for lam in (0.0, 0.5):
                lab, _, cnt, d64, rank, _ = eng.search_mmr(qs, k, k, lam, want64=True)
                assert cnt.tolist() == [k] * nq and np.array_equal(np.sort(lab, axis=1), np.sort(pl, axis=1))
                assert np.array_equal(np.sort(rank, axis=1), np.broadcast_to(np.arange(k, dtype=np.int32), (nq, k)))
                assert np.array_equal(_bits(d64), _bits(np.take_along_axis(pd64, rank.astype(np.int64), axis=1)))
    finally:
        eng.close()


def test_a_copy_of_a_picked_row_is_picked_after_every_other_row_and_ties_go_to_the_lower_rank():
    rng = np.random.default_rng(32)
    d, base, nq = 24, 40, 9
    rows = rng.standard_normal((base, d), dtype=np.float32)
    copies = np.array([3, 3, 11, 20, 20, 20, 39])  # rows 40..46 are copies of these
    rows = np.vstack([rows, rows[copies]])
    n = rows.shape[0]
    first = np.concatenate([np.arange(base), copies])  # the first occurrence of each row's values
    eng = HipScanEngine(d, "l2", device=0)
    try:
        eng.append(rows)
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        lab, _, cnt, d64, rank, obj = _replay(eng, qs, n, n, (0.0,), "dup")
        assert cnt.tolist() == [n] * nq
        for i in range(nq):
            seen, is_copy = set(), []
            for l in lab[i]:
                is_copy.append(int(first[l]) in seen)
                seen.add(int(first[l]))
            # lambda = 0, l2: a copy of a picked row has mind = 0, objective 0 -- every other candidate's is negative
            assert is_copy == [False] * base + [True] * copies.size
            assert (obj[i, 1:base] < 0).all() and (obj[i, base:] == 0).all()
            assert (np.diff(rank[i, base:]) > 0).all()  # the tied copies: the lower rank first
        # a copy ranks right behind its original in the candidate list (equal distance, higher label): with any lambda the
        # pair is told apart by position alone
        _replay(eng, qs, 20, n, (0.3, 1.0), "dup_lam")
    finally:
        eng.close()


def test_a_where_program_equals_search_mmr_over_an_index_of_the_matching_rows_alone():
    rng = np.random.default_rng(33)
    n, d, nq, k, fetch_k = 2000, 16, 9, 10, 60
    metas = random_metadata(rng, n)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    idx = Index(space="cosine", attributes=SCHEMA)
    try:
        idx.add_arrays(rows, "ns", attributes=idx.extract_attributes(metas))
        eng = idx._ns["ns"].engine
        gone = rng.choice(n, n // 10, replace=False)
        eng.tombstone(gone)
        live = np.ones(n, bool)
        live[gone] = False
        empty = 0
        for f in [random_filter(rng) for _ in range(6)] + [{}, {"genre": "zydeco"}]:
            sub = np.flatnonzero(live & np.array([py_match(f, m) for m in metas]))
            program = idx._compile("ns", f)
            got = eng.search_mmr(qs, k, fetch_k, 0.3, where=program, want64=True)
            if sub.size == 0:  # matches nothing (the unseen genre, at the least): counts 0 and full padding
                empty += 1
                assert got[2].tolist() == [0] * nq and (got[0] == -1).all() and (got[4] == -1).all()
                assert np.isinf(got[1]).all() and np.isinf(got[3]).all() and np.isinf(got[5]).all()
                continue
            alone = HipScanEngine(d, "cosine", device=0)
            try:
                alone.append(rows[sub])
                want = alone.search_mmr(qs, k, fetch_k, 0.3, want64=True)
            finally:
                alone.close()
            assert np.array_equal(got[0], np.where(want[0] >= 0, sub[np.maximum(want[0], 0)], -1)), f
            for g, w in zip(got[1:], want[1:]):
                assert np.array_equal(_bits(g), _bits(w)), f
            assert got[2].tolist() == [min(k, sub.size)] * nq
            _replay(eng, qs, k, fetch_k, (0.3,), "where", where=program)
        assert empty >= 1
    finally:
        idx.close()


def test_the_answer_follows_appends_tombstones_and_compaction():
    rng = np.random.default_rng(34)
    d = 48
    rows = rng.standard_normal((3000, d), dtype=np.float32)
    qs = rng.standard_normal((9, d), dtype=np.float32)
    eng = HipScanEngine(d, "l2", device=0)
    try:
        eng.append(rows)
        eng.tombstone(rng.choice(3000, 700, replace=False))
        old = eng.compact()
        rows = rows[old]
        more = rng.standard_normal((500, d), dtype=np.float32)
        eng.append(more)
        rows = np.vstack([rows, more])
        gone = rng.choice(rows.shape[0], 200, replace=False)
        eng.tombstone(gone)
        lab, _, cnt, d64, _, _ = _replay(eng, qs, 12, 100, LAMBDAS, "mutations")
        assert cnt.tolist() == [12] * 9 and not np.isin(lab, gone).any()
        want = np.take_along_axis(exact_scan.exact_distances(qs, rows, "l2"), lab, axis=1)
        assert np.abs(d64 - want).max() <= SCORE_ATOL  # the labels are those of the rows as they stand now
    finally:
        eng.close()


def test_one_query_more_than_the_entrys_chunk():
    rng = np.random.default_rng(35)
    d, n, nq = 8, 17, _native.MMR_CHUNK + 1
    eng = HipScanEngine(d, "cosine", device=0)
    try:
        eng.append(rng.standard_normal((n, d), dtype=np.float32))
        eng.tombstone(np.array([4]))
        qs = rng.standard_normal((nq, d), dtype=np.float32)
        got = _replay(eng, qs, 5, 17, (0.3,), "chunk")
        assert got[2].tolist() == [5] * nq
        got = eng.search_mmr(qs, 17, 17, 0.3, want64=True)  # m = 16 < fetch_k = k: one padded entry per query
        assert got[2].tolist() == [16] * nq and (got[0][:, 16] == -1).all() and (got[4][:, 16] == -1).all()
        assert np.isinf(got[5][:, 16]).all() and (np.sort(got[4][:, :16], axis=1) == np.arange(16)).all()
    finally:
        eng.close()


# ---------------------------------------------------------------- 4. surface
def test_index_and_query_processor_return_the_engines_picks_as_ids_in_pick_order():
    rng = np.random.default_rng(36)
    d, n, nq, k, fetch_k = 32, 900, 5, 8, 50
    idx = Index(space="cosine", attributes={"doc": "int"})
    qp = QueryProcessor(InMemoryStorage(), idx)
    try:
        dtos = [VectorDTO(values=rng.standard_normal(d).tolist(), metadata={"doc": int(i % 31), "i": i}) for i in range(n)]
        qp.upsert_many(dtos, "ns")
        qs = rng.standard_normal((nq, d)).astype(np.float32)
        eng = idx._ns["ns"].engine
        for where in (None, {"doc": {"$lt": 20}}):
            program = None if where is None else idx._compile("ns", where)
            lab, dist, cnt, _, _, _ = eng.search_mmr(qs, k, fetch_k, 0.25, where=program)
            bh = idx.search_many(qs, k, "ns", "cosine", mmr_lambda=0.25, fetch_k=fetch_k, where=where)
            out = qp.find_similar_many(qs, k, "ns", mmr_lambda=0.25, fetch_k=fetch_k, where=where)
            plain = idx.search_many(qs, fetch_k, "ns", "cosine", where=where)
            assert np.array_equal(bh.labels, lab) and np.array_equal(bh.counts, cnt) and cnt.tolist() == [k] * nq
            for i in range(nq):
                assert [h["metadata"]["i"] for h in out[i]] == lab[i].tolist()  # (vector i was stored as row i)
                assert [r.vector_id for r in bh[i]] == [h["id"] for h in out[i]]
                score_of = {r.vector_id: r.score for r in plain[i]}
                assert [r.score for r in bh[i]] == [score_of[r.vector_id] for r in bh[i]] == [h["score"] for h in out[i]]
                if where is not None:
                    assert all(h["metadata"]["doc"] < 20 for h in out[i])
        # the default fetch_k, and a call without mmr_lambda runs what it ran before
        assert np.array_equal(idx.search_many(qs, k, "ns", "cosine", mmr_lambda=0.25).labels,
                              eng.search_mmr(qs, k, 32, 0.25)[0])
        assert np.array_equal(idx.search_many(qs, k, "ns", "cosine").labels, eng.search(qs, k)[0])
    finally:
        idx.close()


# ---------------------------------------------------------------- the C ABI's limits
def test_the_entry_validates_its_limits_and_serves_the_empty_cases():
    eng = HipScanEngine(8, "l2", device=0)
    try:
        qs = np.zeros((2, 8), np.float32)
        lab, dist, cnt, d64, rank, obj = eng.search_mmr(qs, 3, 5, 0.5, want64=True)  # an empty index: only padding
        assert cnt.tolist() == [0, 0] and (lab == -1).all() and (rank == -1).all()
        assert np.isinf(dist).all() and np.isinf(d64).all() and np.isinf(obj).all()
        eng.append(np.eye(8, dtype=np.float32))
        with pytest.raises(RuntimeError, match=r"failed \(6\).*MLVDB_MAX_TOPK"):
            eng.search_mmr(qs, 65, 100, 0.5)
        with pytest.raises(RuntimeError, match=r"failed \(6\).*MLVDB_MMR_MAX_FETCH"):
            eng.search_mmr(qs, 3, 1025, 0.5)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*fetch_k below k"):
            eng.search_mmr(qs, 3, 2, 0.5)
        with pytest.raises(RuntimeError, match=r"failed \(1\).*k must be >= 1"):
            eng.search_mmr(qs, 0, 2, 0.5)
        for lam in (-0.5, 1.5, float("nan")):
            with pytest.raises(RuntimeError, match=r"failed \(1\).*lambda"):
                eng.search_mmr(qs, 3, 5, lam)
        assert eng.search_mmr(qs[:0], 3, 5, 0.5)[0].shape == (0, 3)  # nq = 0: success, nothing written
        eng.tombstone(np.arange(8))
        assert eng.search_mmr(qs, 3, 5, 0.5)[2].tolist() == [0, 0]  # every row tombstoned
    finally:
        eng.close()
    wide = HipScanEngine(5700, "l2", device=0)  # 5712 x 8 + 1024 x 20 bytes > 64 KiB of LDS; 512 candidates fit
    try:
        wide.append(np.ones((3, 5700), np.float32))
        q = np.zeros((1, 5700), np.float32)
        with pytest.raises(RuntimeError, match=r"failed \(6\).*64 KiB of LDS"):
            wide.search_mmr(q, 2, 1024, 0.5)
        assert wide.search_mmr(q, 2, 512, 0.5)[0].tolist() == [[0, 1]]
    finally:
        wide.close()
