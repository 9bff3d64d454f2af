"""Bit codes from the stored rows (include/mlvdb_project.h) without a GPU: the NumPy model on an example worked by hand, the
header against the binding and the Makefile, a null handle, the refusals of ``Index.binarize`` / ``binarize_queries``."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector, _native
from tests.cluster_helpers import ClusterOracleEngine
from tests.project_helpers import model_codes, proj
from tests.test_cluster_host import Untouchable

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ["mlvdb_bits_project", "mlvdb_bits_project_vectors"]


def test_the_model_on_two_rows_worked_by_hand():
    rows, planes, thr = np.zeros((2, 20), np.float32), np.zeros((64, 20), np.float32), np.zeros(64)
    rows[0] = 1.0
    rows[1, [0, 1, 4, 16]] = [2.0 ** 27, 1.0, 0.5, -2.0 ** 27]
    planes[0] = 1.0
    planes[5, [0, 1, 4, 16]] = [2.0 ** 27, 1.0, 1.0, 2.0 ** 27]
    planes[63, 19] = -1.0
    thr[[0, 5, 63]] = [1.5, 1.0, -0.5]
    p = proj(planes, rows)
    # plane 0: row 0 sums to 20; row 1: S0 = 2^27 + 1 - 2^27 = 1 (columns 0, 1, 16), S1 = 0.5 -> 1.5, not > 1.5
    # plane 5, row 1: S0 = 2^54, + 1 rounds back to 2^54, - 2^54 = 0 (the real sum keeps the 1); S1 = 0.5 -> 0.5, not > 1
    # plane 5, row 0: S0 = 2^27 + 1 + 2^27, S1 = 1.  plane 63: -1 for row 0, 0 > -0.5 for row 1.  Every other plane: 0 > 0 fails
    assert p[:, [0, 5, 63]].tolist() == [[20.0, 2.0 ** 28 + 2.0, -1.0], [1.5, 0.5, 0.0]]
    assert model_codes(rows, planes, 64, thr).tolist() == [[0b100001], [1 << 63]]
    assert model_codes(rows, None, 64, np.full(64, 0.75)).tolist() == [[(1 << 20) - 1], [0b11]]  # sign mode: 0.5 is not > 0.75


def test_the_entries_are_declared_bound_built_and_refuse_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_project.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == ENTRIES == sorted(_native.PROJECT_SIGNATURES)
    for entry in ENTRIES:
        params = re.search(entry + r"\((.*?)\);", text, flags=re.S).group(1).split(",")
        assert len(params) == len(_native.PROJECT_SIGNATURES[entry][1]) == 7 and _native.PROJECT_SIGNATURES[entry][0] is C.c_int
    others = [t for name, t in vars(_native).items() if name.endswith("SIGNATURES") and name != "PROJECT_SIGNATURES"]
    assert len(others) > 20 and not any(e in t for e in ENTRIES for t in others)
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert "kernels_project.hip" in make[make.index("SRCS ="):make.index("OBJS =")].split()
    assert "../../include/mlvdb_project.h" in make[make.index("HDRS ="):make.index("# the filter scan's body")].split()
    lib = _native.load()
    buf = (C.c_int64 * 8)()
    assert lib.mlvdb_bits_project(C.c_void_p(), 0, None, 64, None, None, C.cast(buf, C.POINTER(C.c_int64))) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()
    assert lib.mlvdb_bits_project_vectors(C.c_void_p(), buf, 1, None, 64, None, buf) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()


BAD = {"an undeclared attribute": dict(to="nope"), "an attribute that is no bits attribute": dict(to="tag"),
       "planes of the wrong width": dict(planes=np.ones((64, 5), np.float32)),
       "planes of the wrong count": dict(planes=np.ones((128, 6), np.float32)),
       "a non-finite plane": dict(planes=np.full((64, 6), np.inf, np.float32)), "planes a word": dict(planes="signs"),
       "sign with N != dim rounded up to 64": dict(to="wide", planes="sign"),
       "a NaN threshold": dict(thresholds=np.where(np.arange(64) == 7, np.nan, 0.0)),
       "thresholds of the wrong length": dict(thresholds=np.zeros(63)), "a negative seed": dict(seed=-1)}


@pytest.mark.parametrize("what", BAD)
def test_every_refusal_is_a_value_error_before_the_engine_is_touched(what):
    index = Index(space="l2", engine_factory=ClusterOracleEngine, attributes={"tag": "int", "sig": "bits64", "wide": "bits128"})
    index.add([Vector(values=np.full(6, i, np.float32), metadata={"tag": i}) for i in range(4)], "ns")
    index._ns["ns"].engine = Untouchable(6, "l2")
    kw = {"to": "sig", **BAD[what]}
    with pytest.raises(ValueError):
        index.binarize("ns", kw.pop("to"), **kw)
    kw = {"to": "sig", **BAD[what]}
    with pytest.raises(ValueError):
        index.binarize_queries(np.ones((2, 6), np.float32), kw.pop("to"), **kw)
    for where in (lambda m: True, [{"tag": 1}], {"nope": 1}):
        with pytest.raises(ValueError):
            index.binarize("ns", "sig", where=where)
