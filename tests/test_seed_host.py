"""k-means++ seeding (include/mlvdb_seed.h) without a GPU: the NumPy model on an example worked by hand, the header against
the binding and the Makefile, a null handle, ``Index.cluster(init="k-means++")`` / ``cluster_seeds`` over the model engine."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from mlvectordb_amd import Index, InMemoryStorage, QueryProcessor, Vector, _native
from tests.seed_helpers import SeedOracleEngine, draw, model_seed, seed_u, tree
from tests.test_cluster_host import Untouchable

ROOT = Path(__file__).resolve().parents[1]
ENTRY = "mlvdb_kmeans_seed"


def test_the_model_on_six_rows_worked_by_hand():
    # weights 0 2 0 0 1 3: pairs 2 0 4 0, fours 2 4, root 6, and b == 0 -> left all the way down from level 8
    T = tree([0.0, 2.0, 0.0, 0.0, 1.0, 3.0])
    assert len(T) == 9 and T[0].size == 256 and T[-1][0] == 6.0 and T[1][:4].tolist() == [2.0, 0.0, 4.0, 0.0]
    assert draw(T, 0.25) == 1   # r = 1.5 < 2: left; b == 0: left; a == 0: right
    assert draw(T, 0.375) == 4  # r = 2.25 >= 2: r = 0.25, right; b == 0: left; r < 1: left
    assert draw(T, 0.5) == 5    # r = 3 >= 2: r = 1, right; b == 0: left; r = 1 >= 1: r = 0, right
    assert len(tree(np.ones(257))) == 10 and tree(np.ones(257))[-1][0] == 257.0
    # six rows on a line, row 4 no candidate; squared distances
    x = np.array([0.0, 0.0, 4.0, 4.0, 10.0, 7.0])
    live = np.array([True, True, True, True, False, True])
    u = np.array([[0.5, 0.0], [0.5, 0.9], [0.1, 0.2], [0.0, 0.99]])
    labels, potentials, candidates = model_seed(lambda s: (x - x[s]) ** 2, live, 4, u)
    # step 0: r = 2.5 in T1 (pairs 2 2 1 0) -> row 2; best = 16 16 0 0 . 9, root 41
    # step 1: r = 20.5 -> row 1, p = 0 0 0 0 . 9, phi 9;  r = 36.9 -> row 5, phi 32: the first trial wins
    # step 2: both draws can only reach row 5; phi 0 twice, the lower trial wins
    # step 3: root(B) == 0, the draws fall back to T1: r = 0 -> row 0 (a duplicate of pick 1's vector), r = 4.95 -> row 5
    assert labels.tolist() == [2, 1, 5, 0] and potentials.tolist() == [41.0, 9.0, 0.0, 0.0] and candidates == 5


def test_the_entry_is_declared_bound_built_and_refuses_a_null_handle():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mlvdb_seed.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(mlvdb_[a-z0-9_]+)\s*\(", text))) == [ENTRY] == sorted(_native.SEED_SIGNATURES)
    params = [p.strip() for p in re.search(ENTRY + r"\((.*?)\);", text, flags=re.S).group(1).split(",")]
    restype, argtypes = _native.SEED_SIGNATURES[ENTRY]
    assert len(params) == len(argtypes) == 8 and restype is C.c_int
    for p, ctype in zip(params, argtypes):
        want = (C.POINTER(_native.Where) if "mlvdb_where" in p else C.POINTER(C.c_int64) if p.endswith("matched")
                else C.c_void_p) if "*" in p else C.c_int32
        assert ctype is want, p
    consts = dict(re.findall(r"#define\s+MLVDB_(SEED_[A-Z_]+)\s+(\d+)", text))
    assert {k: int(v) for k, v in consts.items()} == {"SEED_MAX_TRIALS": _native.SEED_MAX_TRIALS, "SEED_BLOCK": _native.SEED_BLOCK}
    make = (ROOT / "mlvectordb_amd" / "csrc" / "Makefile").read_text()
    assert "kernels_seed.hip" in make[make.index("SRCS ="):make.index("OBJS =")].split()
    assert "../../include/mlvdb_seed.h" in make[make.index("HDRS ="):make.index("# the filter scan's body")].split()
    lib = _native.load()
    buf = (C.c_int64 * 4)()
    assert lib.mlvdb_kmeans_seed(C.c_void_p(), 1, 1, buf, None, buf, buf, C.cast(buf, C.POINTER(C.c_int64))) == 1
    assert b"null index handle" in lib.mlvdb_last_global_error()


def _index(space="l2", n=300, d=5):
    rng = np.random.default_rng(7)
    rows = (rng.standard_normal((n, d)) + 6.0 * rng.integers(0, 2, (n, d))).astype(np.float32)
    vecs = [Vector(values=r, metadata={"tag": i % 3}) for i, r in enumerate(rows)]
    index = Index(space=space, engine_factory=SeedOracleEngine, attributes={"tag": "int"})
    index.add(vecs, "ns")
    return index, vecs, rows


@pytest.mark.parametrize("space", ["l2", "cosine"])
def test_index_seeds_and_clusters_over_the_model_engine(space):
    index, vecs, rows = _index(space)
    eng = index._ns["ns"].engine
    index.remove([vecs[4].id], "ns")
    live = np.arange(300) != 4
    dist = lambda s: eng._distances(rows[s:s + 1])[0]  # noqa: E731
    # (k, seed, trials, the default's value, where)
    for k, seed, trials, t, where in ((6, 3, None, 3, None), (4, 1, 2, 2, {"tag": 1}), (1, 0, None, 2, None), (9, 2, 8, 8, None)):
        cand = live & (np.arange(300) % 3 == 1) if where else live
        want_labels, want_pot, _ = model_seed(dist, cand, k, seed_u(seed, k, t))
        ids, pot = index.cluster_seeds("ns", space, k, where=where, seed=seed, trials=trials)
        assert ids == [vecs[i].id for i in want_labels] and pot.tobytes() == want_pot.tobytes()
        again = index.cluster_seeds("ns", space, k, where=where, seed=seed, trials=trials)
        assert again[0] == ids and again[1].tobytes() == pot.tobytes()
        # the clustering starts from exactly these rows, in pick order, and equals the run from their ids
        eng.started = ()
        got = index.cluster("ns", space, k, where=where, init="k-means++", seed=seed, trials=trials, max_iterations=3)
        by_ids = index.cluster("ns", space, k, where=where, init=ids, max_iterations=3)
        assert eng.started == (want_labels.tolist(), want_labels.tolist())
        assert got.centroids.tobytes() == by_ids.centroids.tobytes() and np.array_equal(got.sizes, by_ids.sizes)
    eng.started = ()
    QueryProcessor(InMemoryStorage(), index).cluster_vectors(6, "ns", space, init="k-means++", seed=3, trials=2, max_iterations=1)
    assert eng.started == (model_seed(dist, live, 6, seed_u(3, 6, 2))[0].tolist(),)


def test_every_refusal_is_a_value_error_before_the_engine_is_touched():
    index, vecs, rows = _index(n=30)
    index._ns["ns"].engine = Untouchable(5, "l2")
    bad = {"k = 0": dict(k=0), "k = 1025": dict(k=1025), "k a float": dict(k=2.0), "metric ip": dict(metric="ip"),
           "another space": dict(metric="cosine"), "a predicate": dict(where=lambda m: True), "a where list": dict(where=[{"tag": 1}]),
           "a bad filter": dict(where={"nope": 1}), "a negative seed": dict(seed=-1), "seed a float": dict(seed=1.5),
           "trials = 0": dict(trials=0), "trials = 9": dict(trials=9), "trials a bool": dict(trials=True),
           "more seeds than live rows": dict(k=31), "an unknown namespace": dict(namespace="none")}
    for what, kw in bad.items():
        args = {"namespace": "ns", "metric": "l2", "k": 3, **kw}
        for entry, more in ((index.cluster_seeds, {}), (index.cluster, {"init": "k-means++"})):
            with pytest.raises(ValueError):
                entry(args["namespace"], args["metric"], args["k"], **{a: v for a, v in args.items() if a in ("where", "seed", "trials")}, **more)
                pytest.fail(f"{entry.__name__} accepted {what}")
    with pytest.raises(ValueError, match="row-sharded"):
        Index(space="l2", devices=[0, 1], attributes={"tag": "int"}).cluster_seeds("ns", "l2", 2)
    # a filter that leaves fewer candidates than k: known after the engine's one count
    with pytest.raises(ValueError, match="k = 11 centroids but only 10 candidate"):
        _index(n=30)[0].cluster_seeds("ns", "l2", 11, where={"tag": 1})
