"""ctypes binding of ``libmlvdb_hip.so`` (C ABI declared in include/mlvdb_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C mlvectordb_amd/csrc``.
Loading fails loudly: there is no CPU fallback behind this module.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_LIB_NAME = "libmlvdb_hip.so"
_LIB_PATH = Path(__file__).resolve().parent / "csrc" / _LIB_NAME

OK = 0
ERR_OVERFLOW = 7
SPACE_CODES = {"l2": 0, "cosine": 1, "ip": 2}
STRATEGY_CODES = {"auto": 0, "exact": 1, "filter": 2}
MAX_TOPK = 64
MAX_TOPK_PAGED = 16384
ABI_VERSION = 7


class Stats(C.Structure):
    _fields_ = [
        ("strategy_used", C.c_int32),
        ("scan_launches", C.c_int32),
        ("rows_scanned", C.c_int64),
        ("candidates_rescored", C.c_int64),
        ("fallback_queries", C.c_int64),
        ("scan_ms", C.c_double),
        ("total_ms", C.c_double),
        ("bound_dtype", C.c_int32),
        ("reserved", C.c_int32),
    ]


# name -> (restype, argtypes); every symbol include/mlvdb_hip.h declares
_P = C.c_void_p
SIGNATURES = {
    "mlvdb_abi_version": (C.c_int, []),
    "mlvdb_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mlvdb_last_global_error": (C.c_char_p, []),
    "mlvdb_index_create": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, C.POINTER(_P)]),
    "mlvdb_index_destroy": (C.c_int, [_P]),
    "mlvdb_last_error": (C.c_char_p, [_P]),
    "mlvdb_index_append": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mlvdb_index_append_device": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mlvdb_index_tombstone": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mlvdb_index_compact": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mlvdb_index_counts": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mlvdb_index_reset": (C.c_int, [_P, C.c_int32]),
    "mlvdb_index_get_rows": (C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    "mlvdb_index_get_rows_at": (C.c_int, [_P, _P, C.c_int64, _P]),
    "mlvdb_search_batch": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P]),
    "mlvdb_search_batch_filtered": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "mlvdb_search_batch_ex": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P, _P]),
    "mlvdb_search_batch_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P, _P]),
    "mlvdb_range_batch": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_int64, _P, _P, _P]),
    "mlvdb_range_batch_packed": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "mlvdb_pair_distances": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, _P]),
    "mlvdb_index_set_strategy": (C.c_int, [_P, C.c_int32]),
    "mlvdb_index_set_tuning": (C.c_int, [_P, C.c_char_p]),
    "mlvdb_index_get_tuning": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int32)]),
    "mlvdb_index_set_profiling": (C.c_int, [_P, C.c_int32]),
    "mlvdb_index_last_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "mlvdb_layout_offset": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "mlvdb_layout_ld": (C.c_int32, [C.c_int32]),
}

# include/mlvdb_where.h: metadata filters on the device (bound in their own table: SIGNATURES mirrors mlvdb_hip.h alone)
ATTR_INT64 = 1
ATTR_FLOAT64 = 2
ATTR_CODES = {"int64": ATTR_INT64, "float64": ATTR_FLOAT64}


class Where(C.Structure):
    _fields_ = [("ops", C.c_void_p), ("n_ops", C.c_int32), ("set", C.c_void_p), ("n_set", C.c_int64)]


WHERE_SIGNATURES = {
    "mlvdb_attr_define": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "mlvdb_attr_set": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P]),
    "mlvdb_attr_get": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P]),
    "mlvdb_where_count": (C.c_int, [_P, C.POINTER(Where), C.POINTER(C.c_int64)]),
    "mlvdb_where_labels": (C.c_int, [_P, C.POINTER(Where), _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mlvdb_search_batch_where": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(Where), _P, _P, _P, _P]),
    "mlvdb_range_batch_packed_where": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_int64, C.c_int64, C.POINTER(Where),
                                                 _P, _P, _P, _P]),
}

# include/mlvdb_where_each.h: per-query filters in one batched kNN call (their own table, like WHERE_SIGNATURES)
WHERE_EACH_MAX_PROGRAMS = 64
WHERE_EACH_MAX_OPS = 1024
ROUTE_NONE = 0
ROUTE_SCAN = 1
ROUTE_GATHER = 2
ROUTE_NAMES = {ROUTE_NONE: "none", ROUTE_SCAN: "scan", ROUTE_GATHER: "gather"}

WHERE_EACH_SIGNATURES = {
    "mlvdb_search_batch_where_each": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(Where), C.c_int32, _P,
                                                _P, _P, _P, _P, _P]),
    "mlvdb_where_count_each": (C.c_int, [_P, C.POINTER(Where), C.c_int32, _P]),
}

# include/mlvdb_where_each_range.h: per-query filters in one batched range call
WHERE_EACH_RANGE_LIST = 8192
WHERE_EACH_RANGE_SIGNATURES = {
    "mlvdb_range_batch_packed_where_each": (C.c_int, [_P, _P, C.c_int64, C.c_float, C.c_int64, C.c_int64, C.POINTER(Where),
                                                      C.c_int32, _P, _P, _P, _P, _P, _P]),
}

# include/mlvdb_distinct.h: the nearest row of each of the k nearest groups of an int64 attribute column
DISTINCT_SIGNATURES = {
    "mlvdb_search_batch_distinct": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(Where),
                                              _P, _P, _P, _P, _P]),
}

# include/mlvdb_grouped.h: the nearest rows of each of the k nearest groups
GROUPED_MAX_SIZE = 64
GROUPED_SIGNATURES = {
    "mlvdb_search_batch_grouped": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(Where),
                                             _P, _P, _P, _P, _P, _P]),
}

# include/mlvdb_facet.h: facet counts and histograms of attribute columns
FACET_MAX_VALUES = 1 << 20
FACET_MAX_EDGES = 4096
FACET_SIGNATURES = {
    "mlvdb_facet_values": (C.c_int, [_P, C.c_int32, C.POINTER(Where), C.c_int64, _P, _P, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mlvdb_facet_bins": (C.c_int, [_P, C.c_int32, C.POINTER(Where), _P, C.c_int32, _P, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64)]),
}

# include/mlvdb_order.h: the top rows by an attribute column, ranked on the device
ORDER_MAX_ROWS = 4096
ORDER_SIGNATURES = {
    "mlvdb_where_ordered": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(Where), C.c_int64, C.c_int64, _P, _P,
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}

# include/mlvdb_mmr.h: diversified kNN -- greedy maximal-marginal-relevance selection over the plain search's candidates
MMR_MAX_FETCH = 1024
MMR_CHUNK = 1024  # queries per round of plain search + selection inside one native call (api.hip: kMmrChunk)
MMR_SIGNATURES = {
    "mlvdb_search_batch_mmr": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.POINTER(Where),
                                         _P, _P, _P, _P, _P, _P]),
}

# include/mlvdb_like.h: search by stored examples -- queries built from stored rows, the examples stripped from the hits
LIKE_MAX_FETCH = 1024
LIKE_MAX_EXAMPLES = 64
LIKE_CHUNK = 1024  # queries per round of synthesis + plain search + strip inside one native call (api.hip: kLikeChunk)
LIKE_SIGNATURES = {
    "mlvdb_search_batch_like": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(Where),
                                          _P, _P, _P, _P, _P]),
}

# include/mlvdb_maxsim.h: late-interaction search -- documents ranked by the summed best-row distance of a query's tokens
MAXSIM_MAX_TOKENS = 128
MAXSIM_MAX_GROUPS = FACET_MAX_VALUES
MAXSIM_SIGNATURES = {
    "mlvdb_search_batch_maxsim": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(Where),
                                            _P, _P, _P, _P, _P, _P]),
}

# include/mlvdb_mutate.h: attribute values set by label, rows updated / tombstoned by filter
SET_ASSIGN = 0
SET_ADD = 1
ASSIGN_DTYPE = [("attr", "<i4"), ("op", "<i4"), ("a", "<i8")]  # mlvdb_assign
MUTATE_SIGNATURES = {
    "mlvdb_attr_set_at": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P, C.POINTER(C.c_int64)]),
    "mlvdb_attr_update_where": (C.c_int, [_P, C.POINTER(Where), _P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mlvdb_tombstone_where": (C.c_int, [_P, C.POINTER(Where), _P, C.c_int64, C.POINTER(C.c_int64)]),
}

# include/mlvdb_list.h: list-valued attribute columns -- a set of int64 per row, written, read back, filtered and faceted
ATTR_INT64_LIST = 3
LIST_ATTR_CODES = {"int64_list": ATTR_INT64_LIST}
LIST_MAX_LEN = 255
LIST_SIGNATURES = {
    "mlvdb_attr_list_set": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, _P, _P]),
    "mlvdb_attr_list_set_at": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P, _P, _P, C.POINTER(C.c_int64)]),
    "mlvdb_attr_list_get": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mlvdb_attr_list_update_where": (C.c_int, [_P, C.POINTER(Where), C.c_int32, _P, C.c_int32, C.c_int32,
                                               C.POINTER(C.c_int64)]),
    "mlvdb_attr_list_stats": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mlvdb_facet_list_values": (C.c_int, [_P, C.c_int32, C.POINTER(Where), C.c_int64, _P, _P, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}

# include/mlvdb_sparse.h: sparse vector columns -- (term, weight) pairs per row in the list column's storage, and their
# exact top-k inner product with a batch of sparse queries
ATTR_SPARSE = 4
LIST_ATTR_CODES["sparse"] = ATTR_SPARSE
SPARSE_MAX_NNZ = 255
SPARSE_MAX_QUERY_TERMS = 1024
SPARSE_SIGNATURES = {
    "mlvdb_sparse_set": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "mlvdb_sparse_set_at": (C.c_int, [_P, C.c_int32, _P, C.c_int64, _P, _P, _P, _P, C.POINTER(C.c_int64)]),
    "mlvdb_sparse_get": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, _P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mlvdb_search_batch_sparse": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int64, C.c_int32, C.POINTER(Where), _P, _P, _P, _P]),
}

# include/mlvdb_bits.h: binary vector columns -- one fixed-width bit code per row in the list column's storage, and their
# exact top-k Hamming / Jaccard distance to a batch of codes
ATTR_BITS = 6
LIST_ATTR_CODES["bits"] = ATTR_BITS
BITS_MAX_WORDS = 255
BITS_HAMMING = 0
BITS_JACCARD = 1
BITS_METRIC_CODES = {"hamming": BITS_HAMMING, "jaccard": BITS_JACCARD}
BITS_SIGNATURES = {
    "mlvdb_bits_set": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _P, _P]),
    "mlvdb_bits_set_at": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int32, _P, _P, C.POINTER(C.c_int64)]),
    "mlvdb_bits_get": (C.c_int, [_P, C.c_int32, C.c_int64, C.c_int64, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "mlvdb_search_batch_bits": (C.c_int, [_P, C.c_int32, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Where),
                                          _P, _P, _P, _P]),
}

# include/mlvdb_hybrid.h: hybrid search -- a dense and a sparse kNN answer fused into one ranked list on the device
FUSE_CODES = {"rrf": 0, "linear": 1, "relative": 2}
HYBRID_MAX_FETCH_DENSE = 1024
HYBRID_CHUNK = 256  # queries per round of the two legs + union + completion + fusion inside one native call (api.hip: kHybridChunk)
HYBRID_SIGNATURES = {
    "mlvdb_search_batch_hybrid": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_double, C.c_double, C.c_double, C.POINTER(Where),
                                            _P, _P, _P, _P, _P, _P, _P]),
}

# include/mlvdb_geo.h: geo attribute columns -- a location per row, radius / box filters, nearest by distance
ATTR_GEO = 5
ATTR_CODES["geo"] = ATTR_GEO
WHERE_GEO_BOX = 16
WHERE_GEO_RADIUS = 17
GEO_SIGNATURES = {
    "mlvdb_geo_nearest": (C.c_int, [_P, C.c_int32, C.c_int64, C.POINTER(Where), C.c_int64, C.c_int64, _P, _P, _P,
                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}

# include/mlvdb_stats.h: min, max, sum and count of an attribute column per group of a second one
STATS_SIGNATURES = {
    "mlvdb_attr_stats": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(Where), C.c_int64, _P, _P, _P, _P, _P, _P, _P,
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}

# include/mlvdb_score.h: scored kNN -- rows ranked by a formula of the distance and the attribute columns
SCORE_MAX_OPS = 32
SCORE_MAX_DEPTH = 8
SCORE_MAX_CONDS = 8
SCORE_CONST, SCORE_DIST, SCORE_ATTR, SCORE_MATCH = 0, 1, 2, 3
SCORE_ADD, SCORE_SUB, SCORE_MUL, SCORE_DIV, SCORE_MIN, SCORE_MAX = 4, 5, 6, 7, 8, 9
SCORE_NEG, SCORE_ABS = 10, 11


class Score(C.Structure):
    _fields_ = [("ops", C.c_void_p), ("n_ops", C.c_int32), ("conds", C.POINTER(Where)), ("n_conds", C.c_int32)]


SCORE_SIGNATURES = {
    "mlvdb_search_batch_scored": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.POINTER(Score), C.POINTER(Where),
                                            _P, _P, _P, _P]),
}

# include/mlvdb_examples.h: recommend / discover -- rows ranked against a set of examples, each judged on its own
EXAMPLES_MAX = 64
EXAMPLES_BEST, EXAMPLES_DISCOVER, EXAMPLES_CONTEXT = 0, 1, 2
EXAMPLE_POS, EXAMPLE_NEG, EXAMPLE_TARGET = 0, 1, 2

EXAMPLES_SIGNATURES = {
    "mlvdb_search_batch_examples": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32,
                                              C.POINTER(Where), _P, _P, _P, _P]),
}

# include/mlvdb_join.h: similarity join -- the stored rows within a radius of given stored rows, the queries gathered on the device
JOIN_OTHERS, JOIN_LATER = 0, 1
JOIN_WAVE = 256  # left rows per pass of the range chain inside one native call (internal.h: kJoinWave)
JOIN_MAX_CAPACITY = MAX_TOPK_PAGED - JOIN_WAVE
JOIN_SIGNATURES = {
    "mlvdb_join_within": (C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_float, C.c_int64, C.c_int64, C.POINTER(Where),
                                    _P, _P, _P, _P]),
}

# include/mlvdb_cluster.h: nearest-centroid assignment and k-means over the stored rows, the cluster id into an int64 column
CLUSTER_MAX = 1024
CLUSTER_SEGMENT = 256
CLUSTER_MAX_ITERATIONS = 1000
CLUSTER_SIGNATURES = {
    "mlvdb_assign_nearest": (C.c_int, [_P, _P, _P, C.c_int32, C.POINTER(Where), C.c_int32, _P, _P, C.POINTER(C.c_int64)]),
    "mlvdb_kmeans": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.POINTER(Where), C.c_int32, _P, _P, _P,
                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
}

_lib = None


def library_path() -> Path:
    return Path(os.environ.get("MLVDB_HIP_LIBRARY", _LIB_PATH))


def load() -> C.CDLL:
    """Load the shared library and type every entry point; raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64
    # (SONAME libamdhip64.so.7, the name this library links).  If torch is importable, load it first
    # so that the dynamic linker resolves our dependency to the runtime torch already initialised --
    # two runtimes in one process leave the second without a GPU, and device pointers / streams
    # handed over from torch must belong to the runtime that launches our kernels.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not path.exists():
        raise RuntimeError(
            f"{path} not found: the HIP scan library is not built. Run "
            f"`python -c 'import __graft_entry__ as g; g.build()'` or `make -C mlvectordb_amd/csrc`. "
            f"There is no CPU fallback for the search path.")
    lib = C.CDLL(str(path))
    for name, (restype, argtypes) in {**SIGNATURES, **WHERE_SIGNATURES, **WHERE_EACH_SIGNATURES,
                                      **WHERE_EACH_RANGE_SIGNATURES, **DISTINCT_SIGNATURES, **GROUPED_SIGNATURES, **FACET_SIGNATURES,
                                      **ORDER_SIGNATURES, **MMR_SIGNATURES, **LIKE_SIGNATURES, **MAXSIM_SIGNATURES,
                                      **MUTATE_SIGNATURES, **LIST_SIGNATURES, **SPARSE_SIGNATURES, **BITS_SIGNATURES,
                                      **HYBRID_SIGNATURES,
                                      **GEO_SIGNATURES, **STATS_SIGNATURES, **SCORE_SIGNATURES,
                                      **EXAMPLES_SIGNATURES, **JOIN_SIGNATURES, **CLUSTER_SIGNATURES}.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.mlvdb_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {got}, binding expects {ABI_VERSION}")
    _lib = lib
    return lib
