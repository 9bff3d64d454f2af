"""Linear maps of the stored rows on the MI355X (include/mlvdb_transform.h), at the engine level through the C ABI and once
through ``Index``: the images equal the NumPy model of tests/transform_helpers.py byte for byte.  No tolerance."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.transform_helpers import model_transform

pytestmark = pytest.mark.gpu

TAG = 0
INVALID_ARG, OVERFLOW = 1, 7  # MLVDB_ERR_INVALID_ARG, MLVDB_ERR_OVERFLOW


def _gauss(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)


def _pair(space, rows, out_dim):
    """(the source engine holding ``rows`` with tag = label, an empty engine of dim ``out_dim``)."""
    eng, dst = HipScanEngine(rows.shape[1], space, device=0), HipScanEngine(out_dim, space, device=0)
    eng.append(rows)
    eng.define_attr(TAG, "int64")
    eng.set_attr(TAG, 0, np.arange(rows.shape[0], dtype=np.int64))
    return eng, dst


# one row, padding columns, one column of a tile; exactly one tile each way and one 32-column chunk; a ragged second candidate
# block with dim no multiple of 16; an odd number of column groups and a second tile of one column; three tiles, the last ragged
SHAPES = [(1, 1, 1), (128, 32, 64), (130, 20, 3), (300, 48, 65), (257, 100, 130)]


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
@pytest.mark.parametrize("n,dim,out_dim", SHAPES)
def test_the_images_equal_the_model_byte_for_byte(space, n, dim, out_dim):
    eng, dst = _pair(space, _gauss((n, dim), n + dim), out_dim)
    try:
        stored = eng.get_rows(0, n)
        matrix, shift = _gauss((out_dim, dim), out_dim), 0.5 * _gauss(out_dim, 3).astype(np.float64)
        want = model_transform(stored, matrix, shift)
        labels, rows, first = eng.rows_transform(matrix, shift, dst=dst)
        assert first == 0 and labels.tolist() == list(range(n)) and dst.counts() == (n, 0)
        assert rows.tobytes() == want.tobytes() and dst.get_rows(0, n).tobytes() == want.tobytes()
        # the query side: the stored rows as vectors get the stored images, and a second call the same bytes
        again = eng.rows_transform_vectors(stored, matrix, shift)
        assert again.tobytes() == want.tobytes() == eng.rows_transform_vectors(stored, matrix, shift).tobytes()
    finally:
        eng.close()
        dst.close()


@pytest.mark.parametrize("tomb", [(), (5, 131, 449)])
def test_tombstones_and_a_filter_compact_the_candidates(tomb):
    n, dim, out_dim = 600, 24, 70
    rows, matrix = _gauss((n, dim), 11), _gauss((out_dim, dim), 12)
    rows[:, 0], matrix[0, 0] = 0.0, 3e38
    rows[200, 0] = 2.0  # no candidate of the filter: its image overflows and must not trip the flag
    eng, dst = _pair("l2", rows, out_dim)
    try:
        eng.tombstone(np.asarray(tomb + (300,)))
        # labels 128..255 hold no candidate; the 130 others before 400 straddle the first block boundary of the list
        keep = [l for l in range(400) if not 128 <= l < 256]
        program = W.Program(np.array([(W.IN, TAG, 0, len(keep))], dtype=W.OP_DTYPE), np.array(keep, dtype=np.int64))
        expect = np.array([l for l in keep if l not in tomb + (300,)])
        labels, got, first = eng.rows_transform(matrix, None, where=program, dst=dst)
        assert labels.tolist() == expect.tolist() and first == 0 and dst.counts() == (expect.size, 0)
        want = model_transform(rows[expect], matrix)
        assert got.tobytes() == want.tobytes() == dst.get_rows(0, expect.size).tobytes()
        if tomb:  # tombstones alone: the list is the live rows, and row 200's image is refused with nothing appended
            with pytest.raises(RuntimeError, match="a transformed value is not finite"):
                eng.rows_transform(matrix, None, dst=dst)
            assert dst.counts() == (expect.size, 0)
    finally:
        eng.close()
        dst.close()


def test_small_integers_equal_an_int64_matmul():
    rng = np.random.default_rng(5)
    rows, matrix = rng.integers(-9, 10, (261, 37)), rng.integers(-9, 10, (67, 37))
    shift = rng.integers(-50, 51, 67)
    eng = HipScanEngine(37, "ip", device=0)
    try:
        eng.append(rows.astype(np.float32))
        labels, got, _ = eng.rows_transform(matrix.astype(np.float32), shift.astype(np.float64))
        assert labels.size == 261 and (got.astype(np.int64) == rows @ matrix.T - shift[None, :]).all()
    finally:
        eng.close()


def test_the_refusals_leave_both_handles_and_the_outputs_as_they_were():
    rows = np.ones((140, 8), np.float32)
    rows[139, 3] = 2.0
    matrix = np.ones((2, 8), np.float32)
    eng, dst = _pair("ip", rows, 2)
    wide = HipScanEngine(3, "ip", device=0)
    try:
        lib, out, lab = eng._lib, np.full((140, 2), 7.0, np.float32), np.full(140, 7, np.int64)
        matched, first = C.c_int64(-7), C.c_int64(-7)

        def call(m, dst_h, capacity):
            return lib.mlvdb_rows_transform(eng._h, m.ctypes.data, 2, None, None, dst_h, capacity, out.ctypes.data,
                                            lab.ctypes.data, C.byref(matched), C.byref(first))

        huge = matrix.copy()
        huge[1, 3] = 3e38  # times the 2.0 of the last row of the second block
        assert call(huge, dst._h, 140) == INVALID_ARG
        assert b"transform: a transformed value is not finite" in lib.mlvdb_last_error(eng._h)
        assert call(matrix, eng._h, 140) == INVALID_ARG and call(matrix, wide._h, 140) == INVALID_ARG
        assert (out == 7.0).all() and (lab == 7).all() and first.value == -7
        assert call(matrix, dst._h, 139) == OVERFLOW and matched.value == 140
        assert (out == 7.0).all() and (lab == 7).all() and dst.counts() == wide.counts() == (0, 0) and eng.counts() == (140, 0)
        with pytest.raises(RuntimeError, match="a transformed value is not finite"):
            eng.rows_transform_vectors(rows, huge)
        assert call(matrix, dst._h, 140) == 0 and first.value == 0 and out[139].tolist() == [9.0, 9.0]
    finally:
        eng.close()
        dst.close()
        wide.close()


def test_a_pca_reduced_namespace_finds_every_row_by_its_own_image():
    rng = np.random.default_rng(9)
    rows = (rng.standard_normal((150, 4)) @ rng.standard_normal((4, 24)) + 0.01 * rng.standard_normal((150, 24))).astype(np.float32)
    index = Index(space="l2", device=0)
    vecs = [Vector(values=r) for r in rows]
    index.add(vecs, "ns")
    p = index.pca("ns", 4)
    assert index.transform("ns", p.components, shift=p.thresholds, to="pca") == 150
    assert index.namespace_counts("pca") == (150, 0)
    queries = index.transform_queries(rows, p.components, shift=p.thresholds)
    ids, images = index.transform("ns", p.components, shift=p.thresholds)
    assert ids.tolist() == [v.id for v in vecs] and images.tobytes() == queries.tobytes()
    hits = index.search_many(queries, 1, "pca", "l2")
    assert hits.ids()[:, 0].tolist() == [v.id for v in vecs] and (hits.scores[:, 0] == 0.0).all()
    with pytest.raises(ValueError, match="already holds ids"):
        index.transform("ns", p.components, shift=p.thresholds, to="pca")
