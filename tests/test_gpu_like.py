"""Search by stored examples on the MI355X (include/mlvdb_like.h).
1. The synthesised queries against the NumPy restatement of the rule (tests/like_helpers.py): bit for bit on l2 and ip; on
   cosine, where the helper sums the norm in another order, within one float32 spacing + 1e-12 * sum_j |t_j x_jc| (one
   fp32 rounding; fp64 rounding of at most 64 terms).  No accessor shows the norm term the device gives a row taken as a
   query -- ``pair_distances`` returns distances, not the term -- so inv_j itself is held to that tolerance only.
2. The hits against the device's own plain search of ``out_queries`` at k + M, stripped on the host: no tolerance.
3. Against the NumPy oracle with the example rows masked out: equal ids, distances within SCORE_ATOL.
4. ``where`` programs, mutations, the C entry's refusals, the Index / QueryProcessor surface.
Rows are Gaussian; exact duplicates are copies of rows."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, VectorDTO, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.conftest import dump_mismatch
from tests.helpers import SCORE_ATOL
from tests.like_helpers import cosine_query_bound, example_sets, like_queries, like_strip, most_examples
from tests.where_helpers import SCHEMA, py_match, random_filter, random_metadata

pytestmark = pytest.mark.gpu

NAMES = ("labels", "dist", "counts", "d64")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def _flat(groups, weights=None):
    """Per-query label lists (and weight lists; default 1 / count) as the three flat arrays of the C entry."""
    labels = np.array([l for g in groups for l in g], np.int64)
    if weights is None:
        weights = [[1.0 / max(len(g), 1)] * len(g) for g in groups]
    w = np.array([x for g in weights for x in g], np.float64)
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return labels, w, offsets


def _same(tag, got, want):
    for name, g, w in zip(NAMES, got, want):
        if g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
            dump_mismatch(f"like_{tag}", **{f"got_{n}": a for n, a in zip(NAMES, got)},
                          **{f"want_{n}": a for n, a in zip(NAMES, want)})
            bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))
            raise AssertionError(f"{tag}: {name} differs in {bad.size} queries, first {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


def _check_hits(eng, labels, weights, offsets, k, tag, base=None, where=None):
    """``search_like`` against the device's own plain search of ``out_queries`` at k + M, stripped by the helper."""
    lab, d32, cnt, d64, qs = eng.search_like(labels, weights, offsets, k, base=base, where=where, want64=True, want_queries=True)
    most = most_examples(labels, offsets)
    plain = eng.search64(qs, k + most, where=where)
    _same(tag, (lab, d32, cnt, d64), like_strip(*plain, example_sets(labels, offsets), k))
    kept = eng.search_like(labels, weights, offsets, k, base=base, where=where, exclude=False, want64=True, want_queries=True)
    assert np.array_equal(_bits(kept[4]), _bits(qs))
    _same(tag + "_kept", kept[:4], eng.search64(qs, k, where=where))
    lean = eng.search_like(labels, weights, offsets, k, base=base, where=where)
    assert lean[3] is None and lean[4] is None
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(lean[:3], (lab, d32, cnt)))
    return (lab, d32, cnt, d64, qs), plain


# ---------------------------------------------------------------- 1. the queries against NumPy
@pytest.mark.parametrize("d", [3, 20, 64, 300, 768])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_the_synthesised_queries_equal_the_numpy_rule(space, d):
    rng = np.random.default_rng(100 * d + len(space))
    n = 1000
    rows = rng.standard_normal((n, d), dtype=np.float32)
    groups = [[],                                                          # no example: the base row
              [0],
              [15, 16],                                                    # the last row of a panel, the first of the next
              [n - 1] + rng.choice(n - 1, 62, replace=False).tolist(),     # 63
              [0, 15, 16, n - 1] + rng.choice(np.arange(17, n - 1), 60, replace=False).tolist(),  # 64: one per lane
              [5, 900, 5, 5],                                              # a repeated label
              [7, 500],                                                    # tombstoned labels
              [100, 200, 300],
              [42, 42]]                                                    # once for, once against: all zero
    weights = [[], [1.0], [0.5, 0.5], rng.standard_normal(63).tolist(), rng.standard_normal(64).tolist(),
               [0.25, 0.5, 0.125, 1 / 3], [0.5, 0.5], [-0.5, -1.25, -2.0], [1.0, -1.0]]
    base = rng.standard_normal((len(groups), d), dtype=np.float32)
    eng = HipScanEngine(d, space, device=0)
    try:
        eng.append(rows)
        eng.tombstone(np.array([7, 500]))
        for b, first in ((base, 0), (None, 1)):
            labels, w, offsets = _flat(groups[first:], weights[first:])
            got = eng.search_like(labels, w, offsets, 5, base=None if b is None else b[first:], want_queries=True)[4]
            want, scale = like_queries(rows, labels, w, offsets, space, None if b is None else b[first:])
            assert got.dtype == np.float32 and got.shape == want.shape
            if space != "cosine":
                if not np.array_equal(_bits(got), _bits(want)):
                    dump_mismatch(f"like_queries_{space}_{d}_{first}", got=got, want=want)
                    bad = np.argwhere(_bits(got) != _bits(want))
                    raise AssertionError(f"{bad.shape[0]} components differ, first {bad[0]}: {got[tuple(bad[0])]!r} "
                                         f"want {want[tuple(bad[0])]!r}")
            else:
                err = np.abs(got.astype(np.float64) - want.astype(np.float64))
                bound = cosine_query_bound(want, scale)
                print(f"{space} d={d}: worst error / bound {float((err / bound).max()):.3f}")
                assert (err <= bound).all(), float((err / bound).max())
            if b is None:
                assert not got[-1].any()  # t x - t x is exactly zero in every space
            else:
                assert np.array_equal(_bits(got[0]), _bits(b[0]))
    finally:
        eng.close()


# ---------------------------------------------------------------- 2. the hits against the device's own plain search
def _ragged(lo, hi, nq):
    return [lo + i % (hi - lo + 1) for i in range(nq)]


HIT_SHAPES = ((1, [1], 1), (10, _ragged(0, 5, 9), 9), (10, [64] * 3, 3), (64, _ragged(1, 3, 70), 70), (63, [1], 1), (960, [64], 2))


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_the_hits_are_the_plain_search_of_the_synthesised_queries_without_the_examples(space):
    d = 20
    rng = np.random.default_rng(7 + len(space))
    for n in (1, 5, 17, 1000):
        rows = rng.standard_normal((n, d), dtype=np.float32)
        tomb = rng.random(n) < 0.10
        tomb[0] = False  # (a live row is left at every size)
        live = int((~tomb).sum())
        eng = HipScanEngine(d, space, device=0)
        try:
            eng.append(rows)
            if tomb.any():
                eng.tombstone(np.flatnonzero(tomb))
            padded = False
            for k, counts, nq in HIT_SHAPES:
                counts = counts * nq if len(counts) == 1 else counts  # (one count: the same for every query)
                groups = [rng.choice(n, c, replace=c > n).tolist() for c in counts]
                labels, w, offsets = _flat(groups)
                base = rng.standard_normal((nq, d), dtype=np.float32) if 0 in counts else None
                (lab, _, cnt, _, _), plain = _check_hits(eng, labels, w, offsets, k, f"hits_{space}_n{n}_k{k}_q{nq}", base=base)
                sets = example_sets(labels, offsets)
                want_cnt = [min(k, live - int((~tomb[list(s)]).sum())) for s in sets]
                assert cnt.tolist() == want_cnt and not tomb[lab[lab >= 0]].any()
                assert all(not (set(lab[i, :cnt[i]].tolist()) & sets[i]) for i in range(nq))
                padded |= k + most_examples(labels, offsets) > live and (lab[:, -1] == -1).any()
            assert padded  # k + M above the live count: padding and short counts were exercised
        finally:
            eng.close()


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_examples_at_ranks_0_63_and_64_are_compacted_across_the_chunks_of_the_list(space):
    d, n, nq = 20, 1000, 6
    rng = np.random.default_rng(11)
    eng = HipScanEngine(d, space, device=0)
    try:
        eng.append(rng.standard_normal((n, d), dtype=np.float32))
        eng.tombstone(rng.choice(n, 100, replace=False))
        base = rng.standard_normal((nq, d), dtype=np.float32)
        first = eng.search64(base, 80)[0]
        # examples of weight zero leave the base rows as they are, so the ranks of the preliminary search hold
        picks = [[0, 63, 64], [63], [64], [0, 64], [62, 63, 64, 65], [0, 1, 2, 63]]
        groups = [first[i, p].tolist() for i, p in enumerate(picks)]
        labels, w, offsets = _flat(groups, [[0.0] * len(g) for g in groups])
        for k in (60, 61, 62, 70):  # k + M = 64, 65, 66, 74 entries: one chunk, and a second one of 1, 2 and 10
            (lab, _, cnt, _, qs), plain = _check_hits(eng, labels, w, offsets, k, f"ranks_{space}_k{k}", base=base)
            assert np.array_equal(_bits(qs), _bits(base)) and cnt.tolist() == [k] * nq
            for i, p in enumerate(picks):
                assert lab[i].tolist() == np.delete(first[i], p)[:k].tolist()
    finally:
        eng.close()


def test_one_query_more_than_the_entrys_chunk():
    rng = np.random.default_rng(12)
    d, n, nq = 16, 500, _native.LIKE_CHUNK + 6
    eng = HipScanEngine(d, "cosine", device=0)
    try:
        eng.append(rng.standard_normal((n, d), dtype=np.float32))
        eng.tombstone(rng.choice(n, 50, replace=False))
        counts = _ragged(0, 4, nq)
        groups = [rng.choice(n, c, replace=False).tolist() for c in counts]
        labels, w, offsets = _flat(groups)
        base = rng.standard_normal((nq, d), dtype=np.float32)
        (lab, _, cnt, _, qs), _ = _check_hits(eng, labels, w, offsets, 5, "chunks", base=base)
        assert cnt.tolist() == [5] * nq
        want, scale = like_queries(eng.get_rows(0, n), labels, w, offsets, "cosine", base)
        err = np.abs(qs.astype(np.float64) - want.astype(np.float64))
        assert (err <= np.spacing(np.abs(want)).astype(np.float64) + 1e-12 * scale).all()
    finally:
        eng.close()


# ---------------------------------------------------------------- 3. against the NumPy oracle
@pytest.mark.parametrize("n,d", [(4096, 128), (2048, 768)])
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_the_hits_equal_the_numpy_oracle_with_the_example_rows_masked_out(space, n, d):
    rng = np.random.default_rng(n + d + len(space))
    nq, k = 16, 10
    rows = rng.standard_normal((n, d), dtype=np.float32)
    tomb = np.zeros(n, bool)
    tomb[rng.choice(n, n // 10, replace=False)] = True
    groups = [rng.choice(n, 1 + i % 5, replace=False).tolist() for i in range(nq)]
    labels, w, offsets = _flat(groups)
    eng = HipScanEngine(d, space, device=0)
    try:
        eng.append(rows)
        eng.tombstone(np.flatnonzero(tomb))
        lab, d32, cnt, d64, qs = eng.search_like(labels, w, offsets, k, want64=True, want_queries=True)
    finally:
        eng.close()
    assert cnt.tolist() == [k] * nq
    full = exact_scan.exact_distances(qs, rows, space)
    for i in range(nq):
        gone = tomb.copy()
        gone[groups[i]] = True
        wl, _, wc = exact_scan.knn(qs[i], rows, k, space, deleted=gone)
        if not np.array_equal(lab[i], wl[0]):
            dump_mismatch(f"like_oracle_{space}_{n}_{d}", lab=lab, want=wl, query=np.int64(i), d64=d64)
            raise AssertionError(f"query {i}: got {lab[i]} want {wl[0]}")
    err = float(np.abs(d64 - np.take_along_axis(full, lab, axis=1)).max())
    print(f"{space} n={n} d={d}: max |d64 - oracle| = {err:.3e}")
    assert err <= SCORE_ATOL
    # (the fp32 output is the fp64 distance rounded once; an absolute 1e-5 cannot be asked of fp32 itself beyond 128)
    assert np.array_equal(_bits(d32), _bits(d64.astype(np.float32)))


@pytest.mark.parametrize("space", ["l2", "cosine"])
def test_an_exact_copy_of_an_example_survives_the_strip(space):
    rng = np.random.default_rng(13)
    n, d, k = 300, 24, 5
    rows = rng.standard_normal((n, d), dtype=np.float32)
    rows[n - 1] = rows[3]
    rows[150] = rows[3]
    eng = HipScanEngine(d, space, device=0)
    try:
        eng.append(rows)
        labels, w, offsets = _flat([[3], [150, 3]])
        (lab, _, cnt, d64, qs), plain = _check_hits(eng, labels, w, offsets, k, f"copy_{space}")
    finally:
        eng.close()
    assert plain[0][0, :3].tolist() == [3, 150, n - 1] and lab[0, :2].tolist() == [150, n - 1]  # ties go by label
    assert lab[1, 0] == n - 1 and cnt.tolist() == [k, k]
    for i, named in enumerate(([3], [150, 3])):
        gone = np.zeros(n, bool)
        gone[named] = True
        assert np.array_equal(lab[i], exact_scan.knn(qs[i], rows, k, space, deleted=gone)[0][0])
    assert np.abs(d64 - np.take_along_axis(exact_scan.exact_distances(qs, rows, space), lab, axis=1)).max() <= SCORE_ATOL


# ---------------------------------------------------------------- 4. where programs
def test_a_where_program_restricts_the_rows_searched_and_not_the_examples():
    rng = np.random.default_rng(14)
    n, d, nq, k = 2000, 16, 9, 10
    metas = random_metadata(rng, n)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    idx = Index(space="cosine", attributes=SCHEMA)
    try:
        idx.add_arrays(rows, "ns", attributes=idx.extract_attributes(metas))
        eng = idx._ns["ns"].engine
        gone = rng.choice(n, n // 10, replace=False)
        eng.tombstone(gone)
        live = np.ones(n, bool)
        live[gone] = False
        few = None  # a filter that matches some rows, fewer than k
        for year in range(1950, 2025):
            f = {"year": year, "genre": "jazz"}
            c = int((live & np.array([py_match(f, m) for m in metas])).sum())
            if 0 < c < k:
                few = f
                break
        assert few is not None
        outside = short = empty = 0
        for f in [random_filter(rng) for _ in range(6)] + [{}, {"genre": "zydeco"}, few]:
            match = np.array([py_match(f, m) for m in metas])
            sub = np.flatnonzero(live & match)
            program = idx._compile("ns", f)
            groups = [rng.choice(n, 1 + i % 4, replace=False).tolist() for i in range(nq)]
            if (~match).sum() >= 3:  # query 0: none of its examples matches, so the strip removes nothing
                groups[0] = rng.choice(np.flatnonzero(~match), 3, replace=False).tolist()
            if sub.size >= 2:        # query 1: all of its examples match
                groups[1] = rng.choice(sub, 2, replace=False).tolist()
            labels, w, offsets = _flat(groups)
            (lab, d32, cnt, d64, qs), plain = _check_hits(eng, labels, w, offsets, k, "where", where=program)
            sets = example_sets(labels, offsets)
            assert cnt.tolist() == [min(k, sub.size - len(s & set(sub.tolist()))) for s in sets], f
            assert np.isin(lab[lab >= 0], sub).all()
            if (~match).sum() >= 3:
                outside += 1
                assert np.array_equal(lab[0], plain[0][0, :k]) and np.array_equal(_bits(d64[0]), _bits(plain[3][0, :k]))
            short += 0 < sub.size < k
            empty += sub.size == 0
            if sub.size == 0:
                assert (lab == -1).all() and np.isinf(d32).all() and np.isinf(d64).all()
        assert outside >= 1 and short >= 1 and empty >= 1
    finally:
        idx.close()


# ---------------------------------------------------------------- 5. mutations
def test_the_answer_follows_appends_tombstones_and_compaction():
    rng = np.random.default_rng(15)
    d, k = 48, 12
    rows = rng.standard_normal((3000, d), dtype=np.float32)
    eng = HipScanEngine(d, "l2", device=0)
    try:
        eng.append(rows)
        groups = [rng.choice(3000, 1 + i % 4, replace=False).tolist() for i in range(9)]
        labels, w, offsets = _flat(groups)
        _check_hits(eng, labels, w, offsets, k, "before")
        more = rng.standard_normal((500, d), dtype=np.float32)
        eng.append(more)
        rows = np.vstack([rows, more])
        groups[0] = [3100, 3499]  # examples among the appended rows
        groups[1] = groups[1] + [3000]
        labels, w, offsets = _flat(groups)
        named = np.unique(labels)
        gone = rng.choice(np.setdiff1d(np.arange(3500), named), 400, replace=False)
        eng.tombstone(gone)
        (lab0, _, _, _, qs0), _ = _check_hits(eng, labels, w, offsets, k, "appended")
        assert np.array_equal(_bits(qs0), _bits(like_queries(rows, labels, w, offsets, "l2")[0]))
        # a tombstoned example still contributes its stored values, and no longer needs stripping
        eng.tombstone(np.array([groups[2][0]]))
        (lab, _, cnt, d64, qs), _ = _check_hits(eng, labels, w, offsets, k, "tombstoned")
        assert np.array_equal(_bits(qs), _bits(qs0)) and cnt.tolist() == [k] * 9 and not np.isin(lab, gone).any()
        # compaction: the same rows under their new labels give the same answer
        keep = [i for i in range(9) if groups[2][0] not in groups[i]]
        assert 2 not in keep and len(keep) >= 7
        labels, w, offsets = _flat([groups[i] for i in keep])
        before = eng.search_like(labels, w, offsets, k, want64=True, want_queries=True)
        old = eng.compact()
        new_of = np.full(3500, -1, np.int64)
        new_of[old] = np.arange(old.size)
        assert (new_of[labels] >= 0).all()
        (lab, d32, cnt, d64, qs), _ = _check_hits(eng, new_of[labels], w, offsets, k, "compacted")
        assert np.array_equal(_bits(qs), _bits(before[4])) and np.array_equal(cnt, before[2])
        assert np.array_equal(old[lab], before[0]) and np.array_equal(_bits(d64), _bits(before[3]))
        want = np.take_along_axis(exact_scan.exact_distances(qs, rows[old], "l2"), lab, axis=1)
        assert np.abs(d64 - want).max() <= SCORE_ATOL
    finally:
        eng.close()


# ---------------------------------------------------------------- 6. the C entry's refusals
INVALID, UNSUPPORTED = 1, 6  # MLVDB_ERR_INVALID_ARG, MLVDB_ERR_UNSUPPORTED


def _raw(eng, groups, k, weights=None, nq=None, base=None, exclude=1, where=None, offsets=None, null=()):
    """The C entry itself, with sentinel-filled outputs: (status, the outputs untouched?)."""
    labels, w, off = _flat(groups, weights)
    if offsets is not None:
        off = np.asarray(offsets, np.int64)
    n = len(groups) if nq is None else nq
    rows = max(n, 1) * max(k, 1)
    out = {"labels": np.full(rows, -7, np.int64), "dist": np.full(rows, -7, np.float32), "counts": np.full(max(n, 1), -7, np.int32),
           "d64": np.full(rows, -7, np.float64), "queries": np.full(max(n, 1) * eng.dim, -7, np.float32)}
    ins = {"ex_labels": labels, "ex_weights": w, "ex_offsets": off}
    ptr = lambda name, a: None if name in null else a.ctypes.data
    keep = None
    wp = None
    if where is not None:
        wstruct, keep = eng._where(where)
        wp = C.byref(wstruct)
    rc = eng._lib.mlvdb_search_batch_like(
        eng._h, ptr("ex_labels", labels), ptr("ex_weights", w), ptr("ex_offsets", off), None if base is None else base.ctypes.data,
        n, k, exclude, wp, ptr("labels", out["labels"]), ptr("dist", out["dist"]), ptr("counts", out["counts"]),
        ptr("d64", out["d64"]), ptr("queries", out["queries"]))
    return rc, all((a == -7).all() for a in out.values()), out


def test_the_entry_validates_everything_before_it_writes_anything():
    d = 8
    eng = HipScanEngine(d, "l2", device=0)
    try:
        base2 = np.ones((2, d), np.float32)
        # an empty index: base-only queries succeed with padding, any label is out of range
        rc, _, out = _raw(eng, [[], []], 3, base=base2)
        assert rc == 0 and out["counts"][:2].tolist() == [0, 0] and (out["labels"][:6] == -1).all()
        assert np.isinf(out["dist"][:6]).all() and np.isinf(out["d64"][:6]).all() and (out["queries"] == 1).all()
        assert _raw(eng, [[0]], 3)[:2] == (INVALID, True)
        eng.append(np.eye(d, dtype=np.float32)[np.arange(100) % d] + np.arange(100, dtype=np.float32)[:, None])
        ok = [[0, 1], [2]]
        assert _raw(eng, ok, 3)[0] == 0
        assert _raw(eng, [], 3, nq=0, offsets=[0])[:2] == (0, True)  # nq = 0: success, nothing written
        wide = [list(range(64))]
        for what, args, status in (
                ("k = 0", dict(groups=ok, k=0), INVALID),
                ("k < 0", dict(groups=ok, k=-1), INVALID),
                ("k + M above the fetch limit", dict(groups=wide, k=961), UNSUPPORTED),
                ("k + M above it without exclusion", dict(groups=wide, k=961, exclude=0), UNSUPPORTED),
                ("k alone above it", dict(groups=ok, k=1025), UNSUPPORTED),
                ("65 examples", dict(groups=[list(range(65))], k=3), UNSUPPORTED),
                ("65 repeated examples", dict(groups=[[4] * 65], k=3), UNSUPPORTED),
                ("offsets not from 0", dict(groups=ok, k=3, offsets=[1, 2, 3]), INVALID),
                ("offsets descending", dict(groups=ok, k=3, offsets=[0, 2, 1]), INVALID),
                ("label = total", dict(groups=[[0, 100]], k=3), INVALID),
                ("label < 0", dict(groups=[[0], [-1]], k=3), INVALID),
                ("weight nan", dict(groups=ok, k=3, weights=[[1.0, float("nan")], [1.0]]), INVALID),
                ("weight inf", dict(groups=ok, k=3, weights=[[1.0, 1.0], [float("-inf")]]), INVALID),
                ("no example, no base", dict(groups=[[0], []], k=3), INVALID),
                ("null offsets", dict(groups=ok, k=3, null=("ex_offsets",)), INVALID),
                ("null labels", dict(groups=ok, k=3, null=("ex_labels",)), INVALID),
                ("null weights", dict(groups=ok, k=3, null=("ex_weights",)), INVALID),
                ("null out_labels", dict(groups=ok, k=3, null=("labels",)), INVALID),
                ("null out_dist", dict(groups=ok, k=3, null=("dist",)), INVALID),
                ("null out_counts", dict(groups=ok, k=3, null=("counts",)), INVALID),
                ("nq < 0", dict(groups=ok, k=3, nq=-1), INVALID),
                ("a bad program", dict(groups=ok, k=3, where=W.Program(np.array([(W.AND, 0, 0, 0)], W.OP_DTYPE),
                                                                        np.zeros(0, np.int64))), INVALID)):
            rc, untouched, _ = _raw(eng, **args)
            assert (rc, untouched) == (status, True), what
        # the limits themselves are served: 64 examples at k = 960, optional outputs left out
        rc, _, out = _raw(eng, wide, 960, null=("d64", "queries"))
        assert rc == 0 and out["counts"][0] == 36 and (out["d64"] == -7).all() and (out["queries"] == -7).all()
        assert sorted(out["labels"][:36].tolist()) == list(range(64, 100)) and (out["labels"][36:960] == -1).all()
        eng.tombstone(np.arange(100))
        rc, _, out = _raw(eng, ok, 3)  # every row tombstoned: the examples still count, nothing is found
        assert rc == 0 and out["counts"][:2].tolist() == [0, 0] and (out["labels"][:6] == -1).all()
        assert np.array_equal(out["queries"][:d], np.float32(0.5) * (eng.get_rows(0, 1)[0] + eng.get_rows(1, 1)[0]))
    finally:
        eng.close()


# ---------------------------------------------------------------- 7. the surface
def test_index_and_query_processor_return_the_engines_hits_without_the_examples():
    rng = np.random.default_rng(16)
    d, n, k = 32, 900, 8
    idx = Index(space="cosine", attributes={"doc": "int"})
    qp = QueryProcessor(InMemoryStorage(), idx)
    try:
        dtos = [VectorDTO(values=rng.standard_normal(d).tolist(), metadata={"doc": int(i % 31), "i": i}) for i in range(n)]
        qp.upsert_many(dtos, "ns")
        rows = np.array([v.values for v in dtos], np.float32)
        ids = [v["id"] for v in sorted(qp.get_namespace_vectors("ns"), key=lambda v: v["metadata"]["i"])]  # (vector i is row i)
        pos = [[3], [10, 11, 12], [40, 41], [7, 7, 8]]
        neg = [[], [20], [50, 51, 52], [9]]
        groups, weights = [], []
        for p, m in zip(pos, neg):
            wp, wn = Index.like_weights(len(p), len(m))
            groups.append(p + m)
            weights.append([wp] * len(p) + [wn] * len(m))
        labels, w, offsets = _flat(groups, weights)
        base = rng.standard_normal((4, d)).astype(np.float32)
        for b in (None, base):
            for where in (None, {"doc": {"$lt": 20}}):
                qs, _ = like_queries(rows, labels, w, offsets, "cosine", b)
                bh = idx.search_like([[ids[j] for j in p] for p in pos], k, "ns", "cosine",
                                     negative=[[ids[j] for j in m] for m in neg], queries=b, where=where)
                # the device's queries may differ from the helper's in the last bit (cosine): ask the device for its own
                program = None if where is None else idx._compile("ns", where)
                dev = idx._ns["ns"].engine.search_like(labels, w, offsets, k, base=b, where=program, want_queries=True)
                assert np.array_equal(bh.labels, dev[0]) and np.array_equal(bh.counts, dev[2]) and bh.counts.tolist() == [k] * 4
                plain = idx.search_many(dev[4], k + 5, "ns", "cosine", where=where)
                for i in range(4):
                    named = {ids[j] for j in groups[i]}
                    want = [h for h in plain[i] if h.vector_id not in named][:k]
                    assert [(h.vector_id, h.score) for h in bh[i]] == [(h.vector_id, h.score) for h in want]
                assert np.abs(dev[4].astype(np.float64) - qs).max() <= 1e-6
        hits = qp.find_similar_to([ids[j] for j in pos[1]], k, "ns", negative_ids=[ids[j] for j in neg[1]])
        bh = idx.search_like([[ids[j] for j in pos[1]]], k, "ns", "cosine", negative=[[ids[j] for j in neg[1]]])
        assert [(h["id"], h["score"]) for h in hits] == [(r.vector_id, r.score) for r in bh[0]] and len(hits) == k
        assert not {h["id"] for h in hits} & {ids[j] for j in groups[1]}
        assert all(h["metadata"]["i"] == ids.index(h["id"]) and np.array_equal(h["values"], rows[h["metadata"]["i"]]) for h in hits)
        only = qp.find_similar_to([ids[3]], k, "ns", where={"doc": {"$lt": 20}}, query=VectorDTO(values=rows[5].tolist()))
        assert len(only) == k and all(h["metadata"]["doc"] < 20 for h in only) and ids[3] not in [h["id"] for h in only]
        idx.remove([ids[11]], "ns")
        with pytest.raises(ValueError, match=f"{ids[11]} is unknown or removed"):
            idx.search_like([[ids[10], ids[11]]], k, "ns", "cosine")
        with pytest.raises(ValueError, match=f"{ids[11]} is unknown or removed"):
            qp.find_similar_to([ids[11]], k, "ns")
    finally:
        idx.close()
