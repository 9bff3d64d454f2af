"""Row moments on the MI355X (include/mlvdb_moments.h), at the engine level through the C ABI and once through ``Index``: the
count, the sums and the Gram matrix equal the NumPy model of tests/moments_helpers.py byte for byte.  No tolerance."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from mlvectordb_amd.moments import pca_from_moments
from tests.moments_helpers import SLAB, model_moments

pytestmark = pytest.mark.gpu

TAG = 0
TILE = 128  # kMomentsTile (internal.h)
INVALID_ARG = 1  # MLVDB_ERR_INVALID_ARG


def _engine(space, rows):
    eng = HipScanEngine(rows.shape[1], space, device=0)
    eng.append(rows)
    return eng


def _same(got, want):
    return got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()


# (dim, rows): the smallest index; padding columns; exactly one tile; a second tile pair that is ragged; a pair (0, 2) that
# touches no diagonal; three slabs, the last ragged
SHAPES = [(1, 1), (17, 15), (TILE, 16), (TILE + 1, SLAB), (2 * TILE + 16, SLAB + 4), (20, 2 * SLAB + 37)]


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
@pytest.mark.parametrize("dim,n", SHAPES)
def test_the_moments_equal_the_model_byte_for_byte(space, dim, n):
    eng = _engine(space, np.random.default_rng(dim + n).standard_normal((n, dim), dtype=np.float32) + np.float32(0.25))
    try:
        got = eng.row_moments()
        assert _same(got, model_moments(eng.get_rows(0, n))) and np.array_equal(got[2], got[2].T)
    finally:
        eng.close()


def test_only_the_candidates_are_summed_and_never_multiplied_by_zero():
    n, dim = 3 * SLAB + 5, 20
    rows = np.random.default_rng(4).standard_normal((n, dim), dtype=np.float32)
    rows[[7, 9]] = np.inf          # 7 is tombstoned, 9 filtered out: 0 * inf would be NaN
    rows[[8, 10], ::2] = 3e38
    tag = np.arange(n, dtype=np.int64) % 5
    tag[SLAB:2 * SLAB] = 9         # slab 1 holds no candidate of the filter
    tag[[9, 10]] = 9
    tomb = np.concatenate(([7, 8], np.arange(3, n, 11)))
    eng = _engine("l2", rows)
    try:
        eng.define_attr(TAG, "int64")
        eng.set_attr(TAG, 0, tag)
        eng.tombstone(tomb)
        live = ~np.isin(np.arange(n), tomb)
        where = W.Program(np.array([(W.IN, TAG, 0, 2)], dtype=W.OP_DTYPE), np.array([1, 3], dtype=np.int64))
        cand = live & np.isin(tag, [1, 3])
        got = eng.row_moments(where)
        assert got[0] == cand.sum() > 0 and _same(got, model_moments(rows, cand)) and np.isfinite(got[2]).all()
        assert _same(eng.row_moments(where), got)  # a second call: the same bytes
        none = W.Program(np.array([(W.IN, TAG, 0, 1)], dtype=W.OP_DTYPE), np.array([77], dtype=np.int64))
        empty = eng.row_moments(none)
        assert empty[0] == 0 and empty[1].tobytes() == bytes(8 * dim) and empty[2].tobytes() == bytes(8 * dim * dim)
    finally:
        eng.close()


def test_integer_rows_against_an_exact_int64_matmul():
    dim, n = 2 * TILE + 16, SLAB + 4
    rows = np.random.default_rng(6).integers(-8, 9, (n, dim))
    eng = _engine("l2", rows.astype(np.float32))
    try:
        count, sums, gram = eng.row_moments()
        assert count == n and np.array_equal(sums, rows.sum(axis=0)) and np.array_equal(gram, rows.T @ rows)
        eng.tombstone(np.arange(5, n, 7))  # without a filter: the norms alone say which rows count
        rows[5::7] = 0
        count, sums, gram = eng.row_moments()
        assert count == n - len(range(5, n, 7)) and np.array_equal(sums, rows.sum(axis=0)) and np.array_equal(gram, rows.T @ rows)
    finally:
        eng.close()


def test_every_refusal_leaves_the_outputs_untouched():
    eng = _engine("l2", np.ones((3, 4), np.float32))
    try:
        lib, h, n = eng._lib, eng._h, C.c_int64(-5)
        sums, gram = np.full(4, 7.0), np.full((4, 4), 7.0)
        bad_where = _native.Where(None, 0, None, 0)
        calls = {"a null count": (None, None, sums.ctypes.data, gram.ctypes.data),
                 "null sums": (None, C.byref(n), None, gram.ctypes.data),
                 "a null matrix": (None, C.byref(n), sums.ctypes.data, None),
                 "a bad program": (C.byref(bad_where), C.byref(n), sums.ctypes.data, gram.ctypes.data)}
        for what, args in calls.items():
            assert lib.mlvdb_row_moments(h, *args) == INVALID_ARG, what
        assert n.value == -5 and (sums == 7.0).all() and (gram == 7.0).all()
        assert eng.row_moments()[2].tolist() == [[3.0] * 4] * 4
    finally:
        eng.close()


def test_pca_planes_binarize_and_find_each_row_first():
    rng = np.random.default_rng(8)
    rows = (rng.standard_normal((500, 32)) * np.geomspace(4.0, 0.5, 32) + 1.5).astype(np.float32)
    vecs = [Vector(values=r, metadata={"tag": i % 5}) for i, r in enumerate(rows)]
    index = Index(space="l2", attributes={"tag": "int", "sig": "bits64"})
    try:
        index.add(vecs, "ns")
        where = {"tag": {"$in": [0, 2, 3]}}
        cand = np.isin(np.arange(500) % 5, [0, 2, 3])
        stored = index.fetch_values("ns", np.arange(500))
        assert _same(index.moments("ns", where), model_moments(stored, cand))
        p, want = index.pca("ns", 32, where=where), pca_from_moments(*model_moments(stored, cand), 32)
        assert p.count == 300 and p.components.tobytes() == want.components.tobytes() and np.array_equal(p.thresholds, want.thresholds)
        with pytest.raises(ValueError):
            index.pca("ns", 2, where={"tag": 77})  # no candidate: nothing to centre
        planes, thr = np.tile(p.components, (2, 1)), np.tile(p.thresholds, 2)
        assert index.binarize("ns", "sig", planes=planes, thresholds=thr) == 500
        picks = [0, 7, 128, 499]
        hits = index.search_bits(index.binarize_queries(stored[picks], "sig", planes=planes, thresholds=thr), 1, "ns", "sig")
        assert [h[0].vector_id for h in hits] == [vecs[i].id for i in picks] and [h[0].score for h in hits] == [0.0] * 4
    finally:
        index.close()
