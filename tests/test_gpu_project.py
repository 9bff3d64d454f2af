"""Bit codes from the stored rows on the MI355X (include/mlvdb_project.h), at the engine level through the C ABI and once
through ``Index``: the codes ``mlvdb_bits_get`` returns equal the NumPy model of tests/project_helpers.py.  No tolerance."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.project_helpers import model_codes, pack

pytestmark = pytest.mark.gpu

SIG, TAG = 0, 1
TILE, ROW_BLOCK = 64, 128  # kProjectPlaneTile, kProjectRowBlock (internal.h)
INVALID_ARG = 1  # MLVDB_ERR_INVALID_ARG


def _engine(space, rows, tomb=()):
    eng = HipScanEngine(rows.shape[1], space, device=0)
    eng.append(rows)
    eng.define_attr(SIG, "bits")
    eng.define_attr(TAG, "int64")
    eng.set_attr(TAG, 0, np.arange(rows.shape[0], dtype=np.int64) % 5)
    if len(tomb):
        eng.tombstone(np.asarray(tomb))
    return eng


def _codes(eng, n):
    """(widths [n], codes as a list of per-row word lists) of the whole column."""
    widths, flat = eng.bits_get(SIG, 0, n)
    return widths, np.split(flat, np.cumsum(widths)[:-1])


def _gauss(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


# (rows, dim, nbits): one panel and one group; ragged everything; several row blocks and three tiles; the flagship width;
# one tile above TILE with a ragged second row block; two tiles plus 64 with an odd number of column groups
SHAPES = [(1, 16, 64), (17, 20, 128), (1000, 100, 192), (300, 768, 64), (ROW_BLOCK + 1, 36, TILE + 64), (200, 48, 2 * TILE + 64)]


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
@pytest.mark.parametrize("n,dim,nbits", SHAPES)
def test_the_codes_equal_the_model_bit_for_bit(space, n, dim, nbits):
    eng = _engine(space, _gauss((n, dim), n + dim))
    try:
        stored = eng.get_rows(0, n)
        planes, thr = _gauss((nbits, dim), nbits), 0.5 * _gauss(nbits, 3).astype(np.float64)
        assert eng.bits_project(SIG, planes, nbits, thr) == n
        widths, flat = eng.bits_get(SIG, 0, n)
        want = model_codes(stored, planes, nbits, thr)
        assert (widths == nbits // 64).all() and (flat.reshape(n, -1) == want).all()
        # the query side: the same vectors give the stored codes
        assert (eng.bits_project_vectors(stored, planes, nbits, thr) == want).all()
    finally:
        eng.close()


def test_strict_compare_and_packing_against_an_integer_matmul():
    rng = np.random.default_rng(5)
    n, dim, nbits = 300, 40, 128
    rows, planes = rng.integers(-3, 4, (n, dim)), rng.integers(-3, 4, (nbits, dim))
    dots = rows.astype(np.int64) @ planes.astype(np.int64).T
    thr = np.median(dots, axis=0).round()  # integers that many projections hit exactly
    assert (dots == thr).sum() > n and (dots > thr).any()
    eng = _engine("l2", rows.astype(np.float32))
    try:
        assert eng.bits_project(SIG, planes.astype(np.float32), nbits, thr) == n
        assert (eng.bits_get(SIG, 0, n)[1].reshape(n, -1) == pack(dots > thr)).all()
    finally:
        eng.close()


@pytest.mark.parametrize("dim", [20, 64, 100, 768])
def test_sign_mode(dim):
    n, nbits = 150, (dim + 63) // 64 * 64
    rows = _gauss((n, dim), dim)
    thr = 0.3 * _gauss(nbits, 1).astype(np.float64)
    thr[:dim:3] = thr[:dim:3].astype(np.float32)  # (an fp32 value) ...
    rows[::7, ::3] = thr[:dim:3]                   # ... that some rows equal: not above it, bit 0
    eng = _engine("l2", rows)
    try:
        assert eng.bits_project(SIG, None, nbits, thr) == n
        got = eng.bits_get(SIG, 0, n)[1].reshape(n, -1)
        want = model_codes(rows, None, nbits, thr)
        assert (got == want).all() and (rows[::7, ::3].astype(np.float64) == thr[:dim:3]).all()
        if dim % 64:
            assert (got[:, -1] >> np.uint64(dim % 64) == 0).all()  # the padding bits
        assert (eng.bits_project_vectors(rows, None, nbits, thr) == want).all()
        nan_row = rows[:1].copy()
        nan_row[0, 1] = np.nan
        assert (eng.bits_project_vectors(nan_row, None, nbits, thr)[0] == model_codes(nan_row, None, nbits, thr)[0]).all()
        assert (eng.bits_project_vectors(nan_row, _gauss((nbits, dim), 2), nbits) == 0).all()  # a NaN projection gives 0
    finally:
        eng.close()


def test_only_the_candidates_are_written():
    n, dim, nbits = 700, 24, 128
    rows = _gauss((n, dim), 9)
    tomb = np.arange(3, n, 11)
    eng = _engine("cosine", rows)
    try:
        old = np.random.default_rng(2).integers(0, 2 ** 63, (n, 3)).astype(np.uint64)
        eng.bits_set(SIG, 0, W.BitsColumn(old[:200, :2], np.ones(200, np.uint8)))           # the call's width
        eng.bits_set(SIG, 200, W.BitsColumn(old[200:400], np.ones(200, np.uint8)))          # another width
        eng.tombstone(tomb)
        where = W.Program(np.array([(W.IN, TAG, 0, 2)], dtype=W.OP_DTYPE), np.array([1, 3], dtype=np.int64))
        cand = np.isin(np.arange(n) % 5, [1, 3]) & ~np.isin(np.arange(n), tomb)
        planes = _gauss((nbits, dim), 4)
        want = model_codes(eng.get_rows(0, n), planes, nbits)
        assert eng.bits_project(SIG, planes, nbits, where=where) == cand.sum()
        widths, codes = _codes(eng, n)
        for i in range(n):
            keep = [] if i >= 400 else old[i, :2] if i < 200 else old[i]
            assert codes[i].tolist() == (want[i].tolist() if cand[i] else list(keep)), i
        assert eng.bits_project(SIG, planes, nbits, where=where) == cand.sum()  # a second call: the same bytes
        again = _codes(eng, n)
        assert (again[0] == widths).all() and all((a == b).all() for a, b in zip(again[1], codes))
        # rows without a code yet: EXISTS is read before anything is written
        fresh = W.Program(np.array([(W.EXISTS, SIG, 0, 0), (W.NOT, 0, 0, 0)], dtype=W.OP_DTYPE), np.array([], dtype=np.int64))
        assert eng.bits_project(SIG, planes, nbits, where=fresh) == (~cand[400:] & ~np.isin(np.arange(400, n), tomb)).sum()
        before = _codes(eng, n)
        live = ~np.isin(np.arange(n), tomb)
        eng.compact()
        after = _codes(eng, int(live.sum()))
        assert (after[0] == before[0][live]).all()
        assert all((a == b).all() for a, b in zip(after[1], [c for c, l in zip(before[1], live) if l]))
    finally:
        eng.close()


def test_every_refusal_writes_nothing():
    n, dim = 40, 20
    eng = _engine("l2", _gauss((n, dim), 1))
    try:
        good = _gauss((64, dim), 2)
        eng.bits_project(SIG, good, 64)
        before = eng.bits_get(SIG, 0, n)
        inf = good.copy()
        inf[63, dim - 1] = np.inf
        nan_thr = np.zeros(64)
        nan_thr[5] = np.nan
        lib, h, m = eng._lib, eng._h, C.c_int64(0)
        bad_where = _native.Where(None, 0, None, 0)
        calls = {"not a bits column": (TAG, good.ctypes.data, 64, None, None, C.byref(m)),
                 "nbits no multiple of 64": (SIG, good.ctypes.data, 96, None, None, C.byref(m)),
                 "nbits = 0": (SIG, good.ctypes.data, 0, None, None, C.byref(m)),
                 "nbits above the widest code": (SIG, good.ctypes.data, 64 * 256, None, None, C.byref(m)),
                 "sign mode with another nbits": (SIG, None, 128, None, None, C.byref(m)),
                 "a non-finite plane": (SIG, inf.ctypes.data, 64, None, None, C.byref(m)),
                 "a NaN threshold": (SIG, good.ctypes.data, 64, nan_thr.ctypes.data, None, C.byref(m)),
                 "a null output": (SIG, good.ctypes.data, 64, None, None, None),
                 "a bad program": (SIG, good.ctypes.data, 64, None, C.byref(bad_where), C.byref(m))}
        for what, args in calls.items():
            assert lib.mlvdb_bits_project(h, *args) == INVALID_ARG, what
        out = np.zeros(1, np.uint64)
        assert lib.mlvdb_bits_project_vectors(h, good.ctypes.data, 1, good.ctypes.data, 64, None, None) == INVALID_ARG
        assert lib.mlvdb_bits_project_vectors(h, good.ctypes.data, 1, inf.ctypes.data, 64, None, out.ctypes.data) == INVALID_ARG
        after = eng.bits_get(SIG, 0, n)
        assert (after[0] == before[0]).all() and after[1].tobytes() == before[1].tobytes() and out[0] == 0
    finally:
        eng.close()


def test_binarize_then_search_finds_each_row_at_distance_zero():
    rows = _gauss((500, 32), 8)
    vecs = [Vector(values=r, metadata={"tag": i % 5}) for i, r in enumerate(rows)]
    index = Index(space="cosine", attributes={"tag": "int", "sig": "bits128"})
    try:
        index.add(vecs, "ns")
        assert index.binarize("ns", "sig", seed=3, where={"tag": {"$in": [0, 2]}}) == 200
        assert index.binarize("ns", "sig", seed=3, where={"sig": {"$exists": False}}) == 300
        picks = [0, 7, 128, 499]
        stored = index.fetch_values("ns", np.array(picks))
        hits = index.search_bits(index.binarize_queries(stored, "sig", seed=3), 1, "ns", "sig")
        assert [h[0].vector_id for h in hits] == [vecs[i].id for i in picks] and [h[0].score for h in hits] == [0.0] * 4
    finally:
        index.close()
