"""Row moments and PCA (include/mlvdb_moments.h) without a GPU: the NumPy model on a case worked by hand, the header against
the binding and the Makefile, a null handle, the refusals of ``Index.pca``, ``pca_from_moments`` against an SVD."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, PcaResult, QueryProcessor, Vector, _native
from mlvectordb_amd.moments import pca_from_moments
from tests.cluster_helpers import ClusterOracleEngine
from tests.moments_helpers import SLAB, model_moments
from tests.test_cluster_host import Untouchable

ROOT = Path(__file__).resolve().parents[1]


def test_the_model_on_rows_worked_by_hand():
    rows, cand = np.zeros((SLAB + 1, 2), np.float32), np.zeros(SLAB + 1, bool)
    rows[[0, 1, 3, SLAB]] = [[1, 1], [1, 1], [2.0 ** 27, 2.0 ** 26], [1, 1]]
    rows[2] = 5.0  # no candidate
    cand[[0, 1, 3, SLAB]] = True
    count, sums, gram = model_moments(rows, cand)
    # [0][1]: slab 0 is (1 + 1) + 2^53 = 2^53 + 2, exact; slab 1 is 1; 2^53 + 3 is a tie and rounds to the even 2^53 + 4.
    # The descending order 2^53 + 1 + 1 + 1 stays at 2^53 (every + 1 is a tie towards the even 2^53).
    assert count == 4 and gram[0, 1] == gram[1, 0] == 2.0 ** 53 + 4.0 and ((2.0 ** 53 + 1.0) + 1.0) + 1.0 == 2.0 ** 53
    assert gram[0, 0] == 2.0 ** 54 and gram[1, 1] == 2.0 ** 52 + 3.0  # 2 + 2^54 is a tie -> 2^54, + 1 stays; [1][1] is exact
    assert sums.tolist() == [2.0 ** 27 + 3.0, 2.0 ** 26 + 3.0]
    empty = model_moments(rows, np.zeros(SLAB + 1, bool))
    assert empty[0] == 0 and not empty[1].any() and not empty[2].any() and not np.signbit(empty[2]).any()


def test_the_entry_is_declared_bound_built_and_refuses_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_moments.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == ["mlvdb_row_moments"] == sorted(_native.MOMENTS_SIGNATURES)
    params = re.search(r"mlvdb_row_moments\((.*?)\);", text, flags=re.S).group(1).split(",")
    assert len(params) == len(_native.MOMENTS_SIGNATURES["mlvdb_row_moments"][1]) == 5
    assert f"#define MLVDB_MOMENTS_SLAB {SLAB}\n" in text and SLAB == _native.MOMENTS_SLAB
    others = [t for name, t in vars(_native).items() if name.endswith("SIGNATURES") and name != "MOMENTS_SIGNATURES"]
    assert len(others) > 20 and not any("mlvdb_row_moments" in t for t in others)
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert "kernels_moments.hip" in make[make.index("SRCS ="):make.index("OBJS =")].split()
    assert "../../include/mlvdb_moments.h" in make[make.index("HDRS ="):make.index("# the filter scan's body")].split()
    out = np.full(6, 7.0)
    n = C.c_int64(7)
    assert _native.load().mlvdb_row_moments(C.c_void_p(), None, C.byref(n), out.ctypes.data, out[2:].ctypes.data) == 1
    assert b"null index handle" in _native.load().mlvdb_last_global_error() and n.value == 7 and (out == 7.0).all()


@pytest.mark.parametrize("kw", [dict(n_components=0), dict(n_components=7), dict(n_components=2.0), dict(n_components=True),
                                dict(where=lambda m: True), dict(where=[{"tag": 1}]), dict(where={"nope": 1}),
                                dict(namespace="nowhere")])
def test_every_refusal_is_a_value_error_before_the_engine_is_touched(kw):
    index = Index(space="l2", engine_factory=ClusterOracleEngine, attributes={"tag": "int"})
    index.add([Vector(values=np.full(6, i, np.float32), metadata={"tag": i}) for i in range(4)], "ns")
    index._ns["ns"].engine = Untouchable(6, "l2")
    kw = {"namespace": "ns", "n_components": 2, **kw}
    with pytest.raises(ValueError):
        index.pca(kw.pop("namespace"), kw.pop("n_components"), **kw)
    if "where" in kw or kw.get("namespace") == "nowhere":
        with pytest.raises(ValueError):
            index.moments(kw.get("namespace", "ns"), **{k: v for k, v in kw.items() if k == "where"})
    if callable(kw.get("where")):
        with pytest.raises(ValueError):
            QueryProcessor(None, index).fit_pca(2, "ns", where=kw["where"])
    sharded = Index(space="l2", devices=[0, 0], engine_factory=ClusterOracleEngine)
    with pytest.raises(ValueError, match="row-sharded"):
        sharded.pca("ns", 2)


def test_pca_from_moments_against_the_svd_of_the_centred_rows():
    rng = np.random.default_rng(11)
    n, dim = 2000, 12
    scales = np.geomspace(8.0, 0.25, dim)
    basis = np.linalg.qr(rng.standard_normal((dim, dim)))[0]
    rows = ((rng.standard_normal((n, dim)) * scales) @ basis + rng.uniform(-3, 3, dim)).astype(np.float32)
    p = pca_from_moments(*model_moments(rows), 5)
    X = rows.astype(np.float64)
    _, s, vt = np.linalg.svd(X - X.mean(axis=0), full_matrices=False)
    variance = s ** 2 / (n - 1)
    assert isinstance(p, PcaResult) and p.components.dtype == np.float32 and p.components.shape == (5, dim) and p.count == n
    assert np.abs(p.explained_variance / variance[:5] - 1.0).max() < 1e-9
    assert np.abs(p.explained_variance_ratio / (variance[:5] / variance.sum()) - 1.0).max() < 1e-9
    axes = p.components.astype(np.float64)
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)  # (float32 rows are unit to 6e-8; the angle is what is compared)
    # float32 components keep 24 bits: the cosine of the rounding angle is 1 - O(2^-48) ~ 1 - 4e-15
    assert (np.abs(np.sum(axes * vt[:5], axis=1)) > 1.0 - 1e-9).all()
    assert (p.components[np.arange(5), np.abs(p.components).argmax(axis=1)] > 0).all()
    assert np.abs(np.linalg.norm(p.components.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert np.array_equal(p.thresholds, p.components.astype(np.float64) @ p.mean) and np.allclose(p.mean, X.mean(axis=0), rtol=1e-12)
    assert np.allclose(p.transform(rows[:7]), (X[:7] - X.mean(axis=0)) @ p.components.astype(np.float64).T, atol=1e-9)
    raw = pca_from_moments(*model_moments(rows), 3, center=False)
    assert np.allclose(raw.explained_variance, np.linalg.eigvalsh(X.T @ X / n)[::-1][:3], rtol=1e-9) and not raw.mean.any()
    with pytest.raises(ValueError):
        pca_from_moments(1, rows[0].astype(np.float64), np.outer(rows[0], rows[0]).astype(np.float64), 2)  # one row, centred
