"""Linear maps of the stored rows (include/mlvdb_transform.h) without a GPU: the NumPy model on rows worked by hand, the
header against the binding and the Makefile, a null handle, the refusals of ``Index.transform`` / ``transform_queries``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector, _native
from tests.cluster_helpers import ClusterOracleEngine
from tests.test_cluster_host import Untouchable
from tests.transform_helpers import model_transform

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"mlvdb_rows_transform": 11, "mlvdb_rows_transform_vectors": 7}


def test_the_model_on_two_rows_worked_by_hand():
    rows, matrix = np.zeros((2, 20), np.float32), np.zeros((3, 20), np.float32)
    rows[0, [0, 1, 4, 16]] = [2.0 ** 27, 1.0, 0.5, -2.0 ** 27]
    rows[1, [0, 16, 17]] = [1.0, 2.0 ** -24, 2.0 ** -40]
    matrix[0, [0, 1, 4, 16]] = [2.0 ** 27, 1.0, 1.0, 2.0 ** 27]
    matrix[1:, [0, 16, 17]] = 1.0
    got = model_transform(rows, matrix, [0.25, 0.0, 2.0 ** -40])
    # row 0, column 0: S0 = 2^54, + 1 rounds back to 2^54, - 2^54 = 0 (the real sum keeps the 1); S1 = 0.5; - 0.25
    # row 1, columns 1 and 2: S0 = 1 + 2^-24 + 2^-40 is exact in fp64.  Above the tie of fp32 it rounds up to 1 + 2^-23; with
    # the 2^-40 subtracted first it is the tie itself, which goes to the even 1.0
    assert got.dtype == np.float32 and got[0, 0] == 0.25
    assert got[1, 1:].tolist() == [1.0 + 2.0 ** -23, 1.0]


def test_the_entries_are_declared_bound_built_and_refuse_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_transform.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == sorted(ENTRIES) == sorted(_native.TRANSFORM_SIGNATURES)
    for entry, count in ENTRIES.items():
        params = re.search(entry + r"\((.*?)\);", text, flags=re.S).group(1).split(",")
        assert len(params) == len(_native.TRANSFORM_SIGNATURES[entry][1]) == count
        assert _native.TRANSFORM_SIGNATURES[entry][0] is C.c_int
    others = [t for name, t in vars(_native).items() if name.endswith("SIGNATURES") and name != "TRANSFORM_SIGNATURES"]
    assert len(others) > 20 and not any(e in t for e in ENTRIES for t in others)
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert "kernels_transform.hip" in make[make.index("SRCS ="):make.index("OBJS =")].split()
    assert "../../include/mlvdb_transform.h" in make[make.index("HDRS ="):make.index("# the filter scan's body")].split()
    lib = _native.load()
    buf = (C.c_int64 * 8)(*([7] * 8))
    ptr = C.cast(buf, C.POINTER(C.c_int64))
    assert lib.mlvdb_rows_transform(C.c_void_p(), buf, 1, None, None, None, 1, buf, buf, ptr, ptr) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    assert lib.mlvdb_rows_transform_vectors(C.c_void_p(), buf, 1, buf, 1, None, buf) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error() and list(buf) == [7] * 8


BAD = {"a matrix of another width": dict(matrix=np.ones((2, 5), np.float32)), "a flat matrix": dict(matrix=np.ones(6, np.float32)),
       "no output column": dict(matrix=np.ones((0, 6), np.float32)), "4097 output columns": dict(matrix=np.ones((4097, 6), np.float32)),
       "a non-finite matrix": dict(matrix=np.full((2, 6), np.inf, np.float32)), "a matrix of words": dict(matrix=[["a"] * 6] * 2),
       "a shift of another length": dict(shift=np.zeros(3)), "a NaN shift": dict(shift=[0.0, np.nan]),
       "an infinite shift": dict(shift=[np.inf, 0.0])}


def _index():
    index = Index(space="l2", engine_factory=ClusterOracleEngine, attributes={"tag": "int"})
    vecs = [Vector(values=np.full(6, i, np.float32), metadata={"tag": i}) for i in range(4)]
    index.add(vecs, "ns")
    index.add(vecs[:1], "low")
    for name in ("ns", "low"):
        index._ns[name].engine = Untouchable(6, "l2")
    return index


@pytest.mark.parametrize("what", BAD)
def test_a_bad_matrix_or_shift_is_a_value_error_before_the_engine_is_touched(what):
    index = _index()
    for call in (lambda m, **kw: index.transform("ns", m, **kw),
                 lambda m, **kw: index.transform_queries(np.ones((2, 6), np.float32), m, **kw)):
        kw = {"matrix": np.ones((2, 6), np.float32), **BAD[what]}
        with pytest.raises(ValueError):
            call(kw.pop("matrix"), **kw)


def test_the_other_refusals_are_value_errors_before_the_engine_is_touched():
    index, good = _index(), np.ones((2, 6), np.float32)
    for where in (lambda m: True, [{"tag": 1}], {"nope": 1}):
        with pytest.raises(ValueError):
            index.transform("ns", good, where=where)
    # an unknown namespace, itself as the sink, a sink of another dim, a sink that holds a candidate's id
    for args, kw in ((("nope", good), {}), (("ns", good), dict(to="ns")), (("ns", good), dict(to="low")),
                     (("ns", np.ones((6, 6), np.float32)), dict(to="low"))):
        with pytest.raises(ValueError):
            index.transform(*args, **kw)
    with pytest.raises(ValueError):  # no namespace of that dimensionality to compute on
        index.transform_queries(np.ones((2, 7), np.float32), np.ones((2, 7), np.float32))
    with pytest.raises(ValueError, match="row-sharded"):
        Index(space="l2", devices=[0, 1]).transform("ns", good)
    assert index.namespace_counts("low") == (1, 0) and "nope" not in index._ns
