"""The C ABI's refusals and empty answers, pinned call by call: which status and which mlvdb_last_error text an entry gives
for a bad argument, which refusal wins when a call has two faults, and what every output array holds when there is
nothing to find.  The expectations are read off api.hip; the calls go through ctypes, nothing of the Python layer is
involved, and nothing is launched but index creation's fills and the searches of six tombstoned rows."""
import ctypes as C

import numpy as np
import pytest

from mlvectordb_amd import _native

pytestmark = pytest.mark.gpu

OK, INV, UNS = 0, 1, 6  # MLVDB_OK, MLVDB_ERR_INVALID_ARG, MLVDB_ERR_UNSUPPORTED
DIM, ROWS, NQ, K = 4, 6, 2, 3
A_INT, A_F64, A_LIST, A_SPARSE, A_BITS, A_GEO, A_NONE = 0, 1, 2, 3, 4, 5, 7  # the columns of every index of this module
I64_MIN = np.iinfo(np.int64).min
INF = np.inf

NOT_DEFINED = "attribute not defined"
LIST_COL = "a list column: this entry needs a scalar column (see mlvdb_list.h)"
GEO_COL = "a geo column: this entry needs an int64 or float64 value column (see mlvdb_geo.h)"
RANGE = "row range out of bounds"
NULLBUF = "null buffer"
NQ_BAD, K_MIN = "nq out of range", "k must be >= 1"
WHERE_NULL = "where is null"
BAD_PROGRAM = "a program holds 1..MLVDB_WHERE_MAX_OPS ops"
MAX_VALUES = "max_values must be in 1..MLVDB_FACET_MAX_VALUES"
WINDOW = "offset >= 0, limit >= 1 and offset + limit <= MLVDB_ORDER_MAX_ROWS"
LABEL_RANGE, LABEL_TWICE = "label outside [0, total)", "a label appears twice"
DECREASE = "sparse offsets must not decrease"


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def where(ops):
    """A mlvdb_where over (op, attr, a, b) rows; the arrays ride along so that they outlive the call."""
    arr = np.array(ops, dtype=[("op", "<i4"), ("attr", "<i4"), ("a", "<i8"), ("b", "<i8")])
    w = _native.Where(p(arr), len(ops), None, 0)
    w.keep = arr
    return w


class Handles:
    def __init__(self):
        self.lib = lib = _native.load()
        self.filled, self.dead, self.empty = (self._create() for _ in range(3))
        rows = np.arange(ROWS * DIM, dtype=np.float32).reshape(ROWS, DIM)
        first = C.c_int64(-1)
        for h in (self.filled, self.dead):
            assert lib.mlvdb_index_append(h, p(rows), ROWS, C.byref(first)) == OK and first.value == 0
        gone, every = C.c_int64(0), np.arange(ROWS, dtype=np.int64)
        assert lib.mlvdb_index_tombstone(self.dead, p(every), ROWS, C.byref(gone)) == OK
        assert gone.value == ROWS

    def _create(self):
        h = C.c_void_p()
        assert self.lib.mlvdb_index_create(0, DIM, _native.SPACE_CODES["l2"], 0, C.byref(h)) == OK, \
            self.lib.mlvdb_last_global_error()
        for attr, type_ in ((A_INT, _native.ATTR_INT64), (A_F64, _native.ATTR_FLOAT64), (A_LIST, _native.ATTR_INT64_LIST),
                            (A_SPARSE, _native.ATTR_SPARSE), (A_BITS, _native.ATTR_BITS), (A_GEO, _native.ATTR_GEO)):
            assert self.lib.mlvdb_attr_define(h, attr, type_) == OK
        return h

    def close(self):
        for h in (self.filled, self.dead, self.empty):
            assert self.lib.mlvdb_index_destroy(h) == OK


@pytest.fixture(scope="module")
def hs():
    handles = Handles()
    yield handles
    handles.close()


# ---------------------------------------------------------------- refusals
B = np.zeros(64, np.int64)  # any non-null buffer: a refused call reads and writes none of it
Q = np.zeros(NQ * DIM, np.float32)
Z = C.c_int64(0)
R = C.byref(Z)
TRUE = where([(0, 0, 0, 0)])
NO_OPS = _native.Where(None, 0, None, 0)
PROGS = (_native.Where * 1)(TRUE)
POQ, POQ_BAD = np.zeros(NQ, np.int32), np.ones(NQ, np.int32)
L6, L00, L0 = np.array([6], np.int64), np.array([0, 0], np.int64), np.array([0], np.int64)
OFF01, OFF_START1, OFF_DOWN = np.array([0, 1], np.int64), np.array([1, 1], np.int64), np.array([0, -1], np.int64)
OFF_LONG = np.array([0, 1025], np.int64)
BAD_POINT = np.array([1_000_000_000 << 32], np.int64)
NAN_Q = np.full(DIM, np.nan, np.float32)
ONE_SET = np.array([(A_INT, 0, 1)], dtype=_native.ASSIGN_DTYPE)
b, q = p(B), p(Q)

# (entry, arguments behind the handle, status, mlvdb_last_error); rows of one entry in the order of its checks, a row with two
# faults named by "A + B -> A"
REFUSALS = [
    # ---- rows and plain searches
    ("mlvdb_index_append", (None, 1, None), INV, "bad rows / n"),
    ("mlvdb_index_append_device", (None, 1, None), INV, "bad rows / n"),
    ("mlvdb_index_tombstone", (None, 1, None), INV, "bad labels / n"),
    ("mlvdb_index_compact", (None, 0, None), INV, "old_labels too small"),
    ("mlvdb_index_counts", (R, R), OK, None),  # (nothing to refuse but a null handle: test_abi.py)
    ("mlvdb_index_reset", (3,), INV, "space must be < 0 (keep) or a MLVDB_SPACE_* value"),
    ("mlvdb_index_get_rows", (5, 2, b), INV, RANGE),
    ("mlvdb_index_get_rows_at", (None, 1, b), INV, "bad labels / n / out_rows"),
    ("mlvdb_index_get_rows_at", (p(L6), 1, b), INV, "label out of range"),
    ("mlvdb_search_batch", (q, -1, 0, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch", (None, 1, 0, b, b, b), INV, K_MIN),  # k + null buffer -> k
    ("mlvdb_search_batch", (None, 1, 16385, b, b, b), UNS, "k above MLVDB_MAX_TOPK_PAGED"),  # k + null buffer -> k
    ("mlvdb_search_batch", (None, 1, 1, b, b, b), INV, NULLBUF),
    ("mlvdb_search_batch_filtered", (q, -1, 1, b, b, b, b), INV, NQ_BAD),
    ("mlvdb_search_batch_filtered", (q, 1, 0, b, b, b, b), INV, K_MIN),
    ("mlvdb_search_batch_ex", (q, 1 << 25, 1, None, b, b, b, b), INV, NQ_BAD),
    ("mlvdb_search_batch_ex", (q, 1, 16385, None, b, b, b, b), UNS, "k above MLVDB_MAX_TOPK_PAGED"),
    ("mlvdb_search_batch_device", (None, -1, 0, None, None, None, None, None), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_device", (None, 1, 0, None, None, None, None, None), INV, K_MIN),  # k + null buffer -> k
    ("mlvdb_search_batch_device", (None, 1, 16385, None, None, None, None, None), UNS, "k above MLVDB_MAX_TOPK_PAGED"),
    ("mlvdb_search_batch_device", (None, 1, 1, None, None, None, None, None), INV, NULLBUF),
    ("mlvdb_range_batch", (q, -1, 1.0, 0, b, b, b), INV, NQ_BAD),  # nq + capacity -> nq
    ("mlvdb_range_batch", (q, 1, 1.0, 0, b, b, b), INV, "capacity must be >= 1"),
    ("mlvdb_range_batch_packed", (q, -1, 1.0, 1, 1, b, b, None, b), INV, NULLBUF),  # out_offsets + nq -> out_offsets
    ("mlvdb_range_batch_packed", (q, -1, 1.0, 1, 1, b, b, b, b), INV, NQ_BAD),
    ("mlvdb_range_batch_packed", (q, 1, 1.0, 1, -1, b, b, b, b), INV, "total_capacity must be >= 0"),
    ("mlvdb_pair_distances", (q, -1, b, 1, b, b), INV, "nq / m out of range"),
    ("mlvdb_index_set_strategy", (7,), INV, "unknown strategy"),
    ("mlvdb_index_set_tuning", (b"nokey",), INV, "tuning assignment must be KEY=VALUE"),
    ("mlvdb_index_get_tuning", (None, None), INV, "null key / value"),
    ("mlvdb_index_set_profiling", (0,), OK, None),  # (nothing to refuse but a null handle)
    ("mlvdb_index_last_stats", (None,), INV, "out is null"),
    # ---- columns and programs
    ("mlvdb_attr_define", (16, 99), INV, "attribute index out of range"),  # index + type -> index
    ("mlvdb_attr_define", (8, 99), INV, "unknown attribute type"),
    ("mlvdb_attr_define", (A_INT, _native.ATTR_FLOAT64), INV, "attribute already defined with another type"),
    ("mlvdb_attr_set", (A_NONE, 5, 2, b), INV, NOT_DEFINED),  # column + range -> column
    ("mlvdb_attr_set", (A_LIST, 5, 2, b), INV, LIST_COL),  # column type + range -> column type
    ("mlvdb_attr_set", (A_INT, 5, 2, b), INV, RANGE),
    ("mlvdb_attr_set", (A_INT, 0, 1, None), INV, RANGE),
    ("mlvdb_attr_set", (A_GEO, 5, 2, p(BAD_POINT)), INV, RANGE),  # range + value -> range
    ("mlvdb_attr_set", (A_GEO, 0, 1, p(BAD_POINT)), INV, "a geo value outside lat_e7 in [-9e8, 9e8], lon_e7 in [-18e8, 18e8]"),
    ("mlvdb_attr_get", (A_SPARSE, 5, 2, b), INV, "a sparse column: this entry needs a scalar column (see mlvdb_sparse.h)"),
    ("mlvdb_attr_get", (A_INT, -1, 1, b), INV, RANGE),
    ("mlvdb_attr_get", (A_INT, 0, 1, None), INV, RANGE),
    ("mlvdb_where_count", (None, None), INV, "matches is null"),  # matches + program -> matches
    ("mlvdb_where_count", (None, R), INV, WHERE_NULL),
    ("mlvdb_where_count", (C.byref(NO_OPS), R), INV, BAD_PROGRAM),
    ("mlvdb_where_labels", (None, None, 1, R), INV, "bad output buffers"),  # buffers + program -> buffers
    ("mlvdb_where_labels", (None, b, 1, R), INV, WHERE_NULL),
    ("mlvdb_search_batch_where", (q, -1, 0, None, b, b, b, b), INV, WHERE_NULL),  # program + nq -> program
    ("mlvdb_search_batch_where", (q, -1, 0, C.byref(TRUE), b, b, b, b), INV, NQ_BAD),
    ("mlvdb_range_batch_packed_where", (q, -1, 1.0, 0, 1, None, b, b, b, b), INV, WHERE_NULL),  # program + nq -> program
    ("mlvdb_range_batch_packed_where", (q, -1, 1.0, 0, 1, C.byref(TRUE), b, b, b, b), INV, NQ_BAD),
    # ---- per-query programs
    ("mlvdb_where_count_each", (PROGS, 65, None), INV, "n_programs outside 0..MLVDB_WHERE_EACH_MAX_PROGRAMS"),
    ("mlvdb_where_count_each", (None, 1, None), INV, "programs is null"),  # programs + out_matches -> programs
    ("mlvdb_where_count_each", (PROGS, 1, None), INV, "out_matches is null"),
    ("mlvdb_search_batch_where_each", (q, -1, 0, PROGS, 65, p(POQ), b, b, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_where_each", (q, NQ, 0, PROGS, 65, p(POQ), b, b, b, b, b), INV, K_MIN),  # k + programs -> k
    ("mlvdb_search_batch_where_each", (q, NQ, 16385, PROGS, 65, p(POQ), b, b, b, b, b), UNS, "k above MLVDB_MAX_TOPK_PAGED"),
    ("mlvdb_search_batch_where_each", (q, NQ, K, PROGS, 65, None, b, b, b, b, b), INV,
     "n_programs outside 0..MLVDB_WHERE_EACH_MAX_PROGRAMS"),  # programs + null buffer -> programs
    ("mlvdb_search_batch_where_each", (q, NQ, K, PROGS, 1, None, b, b, b, b, b), INV, NULLBUF),
    ("mlvdb_search_batch_where_each", (q, NQ, K, PROGS, 1, p(POQ_BAD), b, b, b, b, b), INV,
     "program_of_query entry outside [-1, n_programs)"),
    ("mlvdb_range_batch_packed_where_each", (q, -1, 1.0, 1, 1, PROGS, 1, p(POQ), b, b, None, b, b), INV, NULLBUF),  # + nq
    ("mlvdb_range_batch_packed_where_each", (q, -1, 1.0, 0, 1, PROGS, 1, p(POQ), b, b, b, b, b), INV, NQ_BAD),  # nq + capacity
    ("mlvdb_range_batch_packed_where_each", (q, NQ, 1.0, 0, -1, PROGS, 1, p(POQ), b, b, b, b, b), INV, "capacity must be >= 1"),
    ("mlvdb_range_batch_packed_where_each", (q, NQ, 1.0, 1, -1, PROGS, 65, p(POQ), b, b, b, b, b), INV,
     "total_capacity must be >= 0"),  # total_capacity + programs -> total_capacity
    # ---- distinct, grouped, mmr, like, maxsim
    ("mlvdb_search_batch_distinct", (q, -1, K, A_NONE, 0, None, b, b, b, b, b), INV, NOT_DEFINED),  # column + nq -> column
    ("mlvdb_search_batch_distinct", (q, -1, K, A_GEO, 0, None, b, b, b, b, b), INV, GEO_COL),
    ("mlvdb_search_batch_distinct", (q, -1, K, A_F64, 0, None, b, b, b, b, b), INV, "distinct needs an int64 column"),
    ("mlvdb_search_batch_distinct", (q, -1, 0, A_INT, 0, None, b, b, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_distinct", (q, NQ, 0, A_INT, -1, None, b, b, b, b, b), INV, K_MIN),  # k + max_groups -> k
    ("mlvdb_search_batch_distinct", (q, NQ, 65, A_INT, -1, None, b, b, b, b, b), UNS, "distinct: k above MLVDB_MAX_TOPK"),
    ("mlvdb_search_batch_distinct", (None, NQ, K, A_INT, -1, None, b, b, b, b, b), INV, "max_groups < 0"),  # + null buffer
    ("mlvdb_search_batch_distinct", (None, NQ, K, A_INT, 0, C.byref(NO_OPS), b, b, b, b, b), INV, NULLBUF),  # + program
    ("mlvdb_search_batch_distinct", (q, NQ, K, A_INT, 0, C.byref(NO_OPS), b, b, b, b, b), INV, BAD_PROGRAM),
    ("mlvdb_search_batch_grouped", (q, -1, K, 2, A_F64, 0, None, b, b, b, b, b, b), INV, "grouped needs an int64 column"),
    ("mlvdb_search_batch_grouped", (q, -1, 0, 2, A_INT, 0, None, b, b, b, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_grouped", (q, NQ, 0, 0, A_INT, 0, None, b, b, b, b, b, b), INV, K_MIN),  # k + group_size -> k
    ("mlvdb_search_batch_grouped", (q, NQ, 65, 0, A_INT, 0, None, b, b, b, b, b, b), INV, "group_size must be >= 1"),
    ("mlvdb_search_batch_grouped", (q, NQ, 65, 65, A_INT, 0, None, b, b, b, b, b, b), UNS, "grouped: k above MLVDB_MAX_TOPK"),
    ("mlvdb_search_batch_grouped", (q, NQ, K, 65, A_INT, -1, None, b, b, b, b, b, b), UNS,
     "grouped: group_size above MLVDB_GROUPED_MAX_SIZE"),  # group_size + max_groups -> group_size
    ("mlvdb_search_batch_grouped", (q, NQ, K, 2, A_INT, -1, None, b, b, b, None, b, b), INV, "max_groups < 0"),
    ("mlvdb_search_batch_grouped", (q, NQ, K, 2, A_INT, 0, None, b, b, b, None, b, b), INV, NULLBUF),
    ("mlvdb_search_batch_mmr", (q, -1, 0, 1, 0.5, None, b, b, b, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_mmr", (q, NQ, 0, -1, 0.5, None, b, b, b, b, b, b), INV, K_MIN),  # k + fetch_k -> k
    ("mlvdb_search_batch_mmr", (q, NQ, 65, 1, 0.5, None, b, b, b, b, b, b), UNS, "mmr: k above MLVDB_MAX_TOPK"),  # + fetch_k
    ("mlvdb_search_batch_mmr", (q, NQ, K, 2, 2.0, None, b, b, b, b, b, b), INV, "mmr: fetch_k below k"),  # + lambda
    ("mlvdb_search_batch_mmr", (q, NQ, K, 1025, 2.0, None, b, b, b, b, b, b), UNS, "mmr: fetch_k above MLVDB_MMR_MAX_FETCH"),
    ("mlvdb_search_batch_mmr", (None, NQ, K, K, 2.0, None, b, b, b, b, b, b), INV, "mmr: lambda outside [0, 1]"),
    ("mlvdb_search_batch_like", (b, b, b, q, -1, 0, 0, None, b, b, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_like", (b, b, None, q, NQ, 0, 0, None, b, b, b, b, b), INV, K_MIN),  # k + null buffer -> k
    ("mlvdb_search_batch_like", (b, b, None, q, NQ, 1025, 0, None, b, b, b, b, b), UNS, "like: k above MLVDB_LIKE_MAX_FETCH"),
    ("mlvdb_search_batch_like", (b, b, None, q, NQ, K, 0, None, b, b, b, b, b), INV, NULLBUF),
    ("mlvdb_search_batch_like", (b, b, p(OFF_START1), q, 1, K, 0, None, b, b, b, b, b), INV, "like: example_offsets must start at 0"),
    ("mlvdb_search_batch_maxsim", (q, b, -1, K, A_F64, None, b, b, b, b, b, b), INV, "maxsim needs an int64 column"),  # + nq
    ("mlvdb_search_batch_maxsim", (q, b, -1, 0, A_INT, None, b, b, b, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_maxsim", (None, b, NQ, 0, A_INT, None, b, b, b, b, b, b), INV, K_MIN),  # k + null buffer -> k
    ("mlvdb_search_batch_maxsim", (None, b, NQ, 65, A_INT, None, b, b, b, b, b, b), UNS, "maxsim: k above MLVDB_MAX_TOPK"),
    ("mlvdb_search_batch_maxsim", (None, b, NQ, K, A_INT, None, b, b, b, b, b, b), INV, NULLBUF),
    ("mlvdb_search_batch_maxsim", (q, p(OFF_START1), 1, K, A_INT, None, b, b, b, b, b, b), INV, "maxsim: token_offsets must start at 0"),
    # ---- facets, statistics, ordered rows
    ("mlvdb_facet_values", (A_NONE, None, 0, b, b, R, R, R), INV, NOT_DEFINED),
    ("mlvdb_facet_values", (A_F64, None, 0, b, b, R, R, R), INV, "value facets need an int64 column"),  # column + max_values
    ("mlvdb_facet_values", (A_INT, None, 0, None, b, R, R, R), INV, MAX_VALUES),  # max_values + null buffer -> max_values
    ("mlvdb_facet_values", (A_INT, C.byref(NO_OPS), 4, None, b, R, R, R), INV, NULLBUF),  # null buffer + program -> null buffer
    ("mlvdb_facet_values", (A_INT, C.byref(NO_OPS), 4, b, b, R, R, R), INV, BAD_PROGRAM),
    ("mlvdb_facet_bins", (A_LIST, None, b, 0, b, R, R), INV, LIST_COL),  # column + n_edges -> column
    ("mlvdb_facet_bins", (A_GEO, None, b, 0, b, R, R), INV, GEO_COL),
    ("mlvdb_facet_bins", (A_INT, None, None, 0, b, R, R), INV, "n_edges must be in 1..MLVDB_FACET_MAX_EDGES"),  # + null buffer
    ("mlvdb_facet_bins", (A_INT, None, None, 1, b, R, R), INV, NULLBUF),
    ("mlvdb_attr_stats", (A_LIST, A_F64, None, 0, b, b, b, b, b, b, b, R, R, R), INV, LIST_COL),  # column + by -> column
    ("mlvdb_attr_stats", (A_INT, A_NONE, None, 0, b, b, b, b, b, b, b, R, R, R), INV, NOT_DEFINED),
    ("mlvdb_attr_stats", (A_INT, A_GEO, None, 0, b, b, b, b, b, b, b, R, R, R), INV, GEO_COL),
    ("mlvdb_attr_stats", (A_INT, A_F64, None, 0, b, b, b, b, b, b, b, R, R, R), INV, "attr_stats: by needs an int64 column"),
    ("mlvdb_attr_stats", (A_INT, -1, None, 0, None, b, b, b, b, b, b, R, R, R), INV,
     "max_groups must be in 1..MLVDB_FACET_MAX_VALUES"),  # max_groups + null buffer -> max_groups
    ("mlvdb_attr_stats", (A_INT, -1, None, 1, None, b, b, b, b, b, b, R, R, R), INV, NULLBUF),
    ("mlvdb_where_ordered", (A_LIST, 0, None, 0, 0, b, b, R, R, R), INV, LIST_COL),  # column + window -> column
    ("mlvdb_where_ordered", (A_GEO, 0, None, 0, 0, b, b, R, R, R), INV, GEO_COL),
    ("mlvdb_where_ordered", (A_INT, 0, None, 0, 0, None, b, R, R, R), INV, WINDOW),  # window + null buffer -> window
    ("mlvdb_where_ordered", (A_INT, 0, C.byref(NO_OPS), 0, 1, None, b, R, R, R), INV, NULLBUF),  # null buffer + program
    ("mlvdb_geo_nearest", (A_INT, 0, None, 0, 0, b, b, b, R, R, R), INV, "geo_nearest needs a geo column"),
    ("mlvdb_geo_nearest", (A_GEO, int(BAD_POINT[0]), None, 0, 0, b, b, b, R, R, R), INV,
     "geo_nearest: center is not a point (lat_e7, lon_e7 out of range)"),  # center + window -> center
    ("mlvdb_geo_nearest", (A_GEO, 0, None, 4096, 1, b, b, b, R, R, R), INV, WINDOW),
    # ---- writes by label and by program
    ("mlvdb_attr_set_at", (A_LIST, None, 1, b, R), INV, LIST_COL),  # column + labels -> column
    ("mlvdb_attr_set_at", (A_INT, None, 1, b, R), INV, "bad labels / values / n"),
    ("mlvdb_attr_set_at", (A_INT, p(L0), 1, None, R), INV, "bad labels / values / n"),
    ("mlvdb_attr_set_at", (A_INT, p(L0), 1, b, None), INV, "bad labels / values / n"),
    ("mlvdb_attr_set_at", (A_GEO, p(L6), 1, p(BAD_POINT), R), INV, LABEL_RANGE),  # label + value -> label
    ("mlvdb_attr_set_at", (A_INT, p(L00), 2, b, R), INV, LABEL_TWICE),
    ("mlvdb_attr_set_at", (A_GEO, p(L0), 1, p(BAD_POINT), R), INV, "a geo value outside lat_e7 in [-9e8, 9e8], lon_e7 in [-18e8, 18e8]"),
    ("mlvdb_attr_update_where", (None, None, 0, None, None), INV, "null counter"),  # counters + assignments + program
    ("mlvdb_attr_update_where", (None, None, 0, R, R), INV, "a call holds 1..MLVDB_MAX_ATTRS assignments"),  # + program
    ("mlvdb_attr_update_where", (None, p(ONE_SET), 1, R, R), INV, WHERE_NULL),
    ("mlvdb_tombstone_where", (None, None, 1, R), INV, "bad output buffers"),  # buffers + program -> buffers
    ("mlvdb_tombstone_where", (None, b, 1, R), INV, WHERE_NULL),
    # ---- list columns
    ("mlvdb_attr_list_set", (A_INT, 5, 2, None, b, None), INV, "not a list column"),  # column + range -> column
    ("mlvdb_attr_list_set", (A_LIST, 5, 2, None, b, None), INV, RANGE),  # range + offsets -> range
    ("mlvdb_attr_list_set", (A_LIST, 0, 1, None, b, None), INV, "bad list offsets"),
    ("mlvdb_attr_list_set_at", (A_INT, None, 1, None, b, None, R), INV, "not a list column"),  # column + labels -> column
    ("mlvdb_attr_list_set_at", (A_LIST, None, 1, None, b, None, R), INV, "bad labels / n"),  # labels + offsets -> labels
    ("mlvdb_attr_list_set_at", (A_LIST, p(L0), 1, None, b, None, None), INV, "bad labels / n"),
    ("mlvdb_attr_list_set_at", (A_LIST, p(L6), 1, None, b, None, R), INV, LABEL_RANGE),  # label + offsets -> label
    ("mlvdb_attr_list_set_at", (A_LIST, p(L00), 2, None, b, None, R), INV, LABEL_TWICE),
    ("mlvdb_attr_list_set_at", (A_LIST, p(L0), 1, None, b, None, R), INV, "bad list offsets"),
    ("mlvdb_attr_list_get", (A_LIST, 5, 2, None, b, None, 1, None), INV, RANGE),  # range + buffers -> range
    ("mlvdb_attr_list_get", (A_LIST, 0, 1, None, b, None, 1, None), INV, "bad output buffers"),
    ("mlvdb_attr_list_update_where", (None, A_INT, None, 1, 0, None), INV, "null counter"),  # counter + column -> counter
    ("mlvdb_attr_list_update_where", (None, A_INT, None, 1, 0, R), INV, "not a list column"),  # column + values -> column
    ("mlvdb_attr_list_update_where", (None, A_LIST, None, 1, 0, R), INV, "values is null"),  # values + program -> values
    ("mlvdb_attr_list_update_where", (None, A_LIST, None, 1, 1, R), INV, WHERE_NULL),
    ("mlvdb_attr_list_stats", (A_INT, None, None), INV, "not a list, sparse or bits column"),  # column + counters -> column
    ("mlvdb_attr_list_stats", (A_LIST, None, None), INV, "null counter"),
    ("mlvdb_facet_list_values", (A_INT, None, 0, b, b, R, R, R), INV, "not a list column"),  # column + max_values -> column
    ("mlvdb_facet_list_values", (A_LIST, None, 0, None, b, R, R, R), INV, MAX_VALUES),  # max_values + null buffer
    ("mlvdb_facet_list_values", (A_LIST, C.byref(NO_OPS), 1, None, b, R, R, R), INV, NULLBUF),  # null buffer + program
    # ---- sparse columns
    ("mlvdb_sparse_set", (A_LIST, 5, 2, None, b, b, None), INV, "not a sparse column"),  # column + range -> column
    ("mlvdb_sparse_set", (A_SPARSE, 5, 2, None, b, b, None), INV, RANGE),  # range + offsets -> range
    ("mlvdb_sparse_set", (A_SPARSE, 0, 1, None, b, b, None), INV, "bad sparse offsets"),
    ("mlvdb_sparse_set_at", (A_SPARSE, None, 1, None, b, b, None, R), INV, "bad labels / n"),  # labels + offsets -> labels
    ("mlvdb_sparse_set_at", (A_SPARSE, p(L6), 1, None, b, b, None, R), INV, LABEL_RANGE),  # label + offsets -> label
    ("mlvdb_sparse_set_at", (A_SPARSE, p(L00), 2, None, b, b, None, R), INV, LABEL_TWICE),
    ("mlvdb_sparse_set_at", (A_SPARSE, p(L0), 1, None, b, b, None, R), INV, "bad sparse offsets"),
    ("mlvdb_sparse_get", (A_SPARSE, 5, 2, None, b, b, None, 1, None), INV, RANGE),  # range + buffers -> range
    ("mlvdb_sparse_get", (A_SPARSE, 0, 1, None, b, b, None, 1, None), INV, "bad output buffers"),
    ("mlvdb_search_batch_sparse", (A_LIST, b, b, b, -1, K, None, b, b, b, b), INV, "not a sparse column"),  # column + nq
    ("mlvdb_search_batch_sparse", (A_SPARSE, b, b, b, -1, 0, None, b, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_sparse", (A_SPARSE, None, b, b, 1, 0, None, b, b, b, b), INV, K_MIN),  # k + null buffer -> k
    ("mlvdb_search_batch_sparse", (A_SPARSE, None, b, b, 1, 65, None, b, b, b, b), UNS, "sparse search: k above MLVDB_MAX_TOPK"),
    ("mlvdb_search_batch_sparse", (A_SPARSE, None, b, b, 1, K, None, b, b, b, b), INV, NULLBUF),
    ("mlvdb_search_batch_sparse", (A_SPARSE, p(OFF_START1), b, b, 1, K, None, b, b, b, b), INV,
     "sparse search: q_offsets must start at 0"),
    ("mlvdb_search_batch_sparse", (A_SPARSE, p(OFF_DOWN), b, b, 1, K, C.byref(NO_OPS), b, b, b, b), INV, DECREASE),  # + program
    ("mlvdb_search_batch_sparse", (A_SPARSE, p(OFF_LONG), b, b, 1, K, None, b, b, b, b), INV,
     "a sparse vector with too many entries"),
    ("mlvdb_search_batch_sparse", (A_SPARSE, p(OFF01), None, b, 1, K, None, b, b, b, b), INV, "terms / weights is null"),
    ("mlvdb_search_batch_sparse", (A_SPARSE, p(OFF01), b, b, 1, K, C.byref(NO_OPS), b, b, b, b), INV, BAD_PROGRAM),
    # ---- bits columns
    ("mlvdb_bits_set", (A_LIST, 5, 2, 0, None, None), INV, "not a bits column"),  # column + words -> column
    ("mlvdb_bits_set", (A_BITS, 5, 2, 0, None, None), INV, "words must be in 1..MLVDB_BITS_MAX_WORDS"),  # words + range -> words
    ("mlvdb_bits_set", (A_BITS, 5, 2, 1, None, None), INV, RANGE),  # range + codes -> range
    ("mlvdb_bits_set", (A_BITS, 0, 1, 1, None, None), INV, "codes is null"),
    ("mlvdb_bits_set_at", (A_BITS, None, 1, 256, None, None, R), INV, "words must be in 1..MLVDB_BITS_MAX_WORDS"),  # + labels
    ("mlvdb_bits_set_at", (A_BITS, None, 1, 1, None, None, R), INV, "bad labels / n"),  # labels + codes -> labels
    ("mlvdb_bits_set_at", (A_BITS, p(L6), 1, 1, None, None, R), INV, "codes is null"),  # codes + label -> codes
    ("mlvdb_bits_set_at", (A_BITS, p(L6), 1, 1, b, None, R), INV, LABEL_RANGE),
    ("mlvdb_bits_set_at", (A_BITS, p(L00), 2, 1, b, None, R), INV, LABEL_TWICE),
    ("mlvdb_bits_get", (A_BITS, 5, 2, None, b, 1, None), INV, RANGE),  # range + buffers -> range
    ("mlvdb_bits_get", (A_BITS, 0, 1, None, b, 1, R), INV, "bad output buffers"),
    ("mlvdb_search_batch_bits", (A_LIST, b, -1, 0, 9, K, None, b, b, b, b), INV, "not a bits column"),  # column + words
    ("mlvdb_search_batch_bits", (A_BITS, b, -1, 0, 9, K, None, b, b, b, b), INV, "words must be in 1..MLVDB_BITS_MAX_WORDS"),
    ("mlvdb_search_batch_bits", (A_BITS, b, -1, 1, 9, K, None, b, b, b, b), INV, "unknown bits metric"),  # metric + nq -> metric
    ("mlvdb_search_batch_bits", (A_BITS, b, -1, 1, 0, 0, None, b, b, b, b), INV, NQ_BAD),  # nq + k -> nq
    ("mlvdb_search_batch_bits", (A_BITS, None, 1, 1, 1, 0, None, b, b, b, b), INV, K_MIN),  # k + null buffer -> k
    ("mlvdb_search_batch_bits", (A_BITS, None, 1, 1, 1, 65, None, b, b, b, b), UNS, "bits search: k above MLVDB_MAX_TOPK"),
    ("mlvdb_search_batch_bits", (A_BITS, None, 1, 1, 1, K, C.byref(NO_OPS), b, b, b, b), INV, NULLBUF),  # null buffer + program
    ("mlvdb_search_batch_bits", (A_BITS, b, 1, 1, 1, K, C.byref(NO_OPS), b, b, b, b), INV, BAD_PROGRAM),
    # ---- hybrid
    ("mlvdb_search_batch_hybrid", (q, A_LIST, b, b, b, -1, K, 1, 1, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), INV,
     "not a sparse column"),  # column + nq -> column
    ("mlvdb_search_batch_hybrid", (q, A_SPARSE, b, b, b, -1, 0, 1, 1, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), INV, NQ_BAD),
    ("mlvdb_search_batch_hybrid", (q, A_SPARSE, b, b, b, 1, 0, 0, 1, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), INV, K_MIN),
    ("mlvdb_search_batch_hybrid", (q, A_SPARSE, b, b, b, 1, 65, 0, 1, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), UNS,
     "hybrid: k above MLVDB_MAX_TOPK"),  # k + fetch_dense -> k
    ("mlvdb_search_batch_hybrid", (q, A_SPARSE, b, b, b, 1, K, 0, 65, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), INV,
     "hybrid: fetch_dense / fetch_sparse must be >= 1"),
    ("mlvdb_search_batch_hybrid", (q, A_SPARSE, b, b, b, 1, K, 1, 65, 9, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), UNS,
     "hybrid: fetch_sparse above MLVDB_MAX_TOPK"),  # fetch_sparse + method -> fetch_sparse
    ("mlvdb_search_batch_hybrid", (q, A_SPARSE, b, b, b, 1, K, 1, 1, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), INV,
     "hybrid: k above fetch_dense + fetch_sparse"),
    ("mlvdb_search_batch_hybrid", (None, A_SPARSE, b, b, b, 1, K, K, K, 0, 1.0, 1.0, -1.0, None, b, b, b, b, b, b, b), INV,
     "hybrid: the RRF constant must be finite and >= 0"),  # constant + null buffer -> constant
    ("mlvdb_search_batch_hybrid", (None, A_SPARSE, b, b, b, 1, K, K, K, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), INV, NULLBUF),
    ("mlvdb_search_batch_hybrid", (q, A_SPARSE, p(OFF_START1), b, b, 1, K, K, K, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b), INV,
     "hybrid: q_offsets must start at 0"),
    ("mlvdb_search_batch_hybrid", (p(NAN_Q), A_SPARSE, p(OFF_DOWN), b, b, 1, K, K, K, 0, 1.0, 1.0, 60.0, None, b, b, b, b, b, b, b),
     INV, DECREASE),  # sparse queries + dense queries -> sparse queries
    ("mlvdb_search_batch_hybrid", (p(NAN_Q), A_SPARSE, p(OFF01), b, b, 1, K, K, K, 0, 1.0, 1.0, 60.0, C.byref(NO_OPS),
                                   b, b, b, b, b, b, b), INV, "hybrid: a NaN in the dense queries"),  # + program
    ("mlvdb_search_batch_hybrid", (q, A_SPARSE, p(OFF01), b, b, 1, K, K, K, 0, 1.0, 1.0, 60.0, C.byref(NO_OPS),
                                   b, b, b, b, b, b, b), INV, BAD_PROGRAM),
]


def test_every_handle_entry_has_a_row():
    bound = {**_native.SIGNATURES, **_native.WHERE_SIGNATURES, **_native.WHERE_EACH_SIGNATURES,
             **_native.WHERE_EACH_RANGE_SIGNATURES, **_native.DISTINCT_SIGNATURES, **_native.GROUPED_SIGNATURES,
             **_native.FACET_SIGNATURES, **_native.ORDER_SIGNATURES, **_native.MMR_SIGNATURES, **_native.LIKE_SIGNATURES,
             **_native.MAXSIM_SIGNATURES, **_native.MUTATE_SIGNATURES, **_native.LIST_SIGNATURES, **_native.SPARSE_SIGNATURES,
             **_native.BITS_SIGNATURES, **_native.HYBRID_SIGNATURES, **_native.GEO_SIGNATURES, **_native.STATS_SIGNATURES}
    entries = {n for n, (_, argtypes) in bound.items()
               if argtypes[:1] == [C.c_void_p] and n not in ("mlvdb_index_destroy", "mlvdb_last_error")}
    assert entries == {name for name, *_ in REFUSALS}
    for name, args, *_ in REFUSALS:
        assert len(args) + 1 == len(bound[name][1]), name


@pytest.mark.parametrize("row", range(len(REFUSALS)), ids=lambda i: f"{i}-{REFUSALS[i][0][6:]}")
def test_refusal(hs, row):
    name, args, status, text = REFUSALS[row]
    total, deleted = C.c_int64(-1), C.c_int64(-1)
    got = getattr(hs.lib, name)(hs.filled, *args)
    assert got == status, (name, got, hs.lib.mlvdb_last_error(hs.filled))
    if text is not None:
        assert hs.lib.mlvdb_last_error(hs.filled).decode() == text, name
    # a refused call changed nothing
    assert hs.lib.mlvdb_index_counts(hs.filled, C.byref(total), C.byref(deleted)) == OK
    assert (total.value, deleted.value) == (ROWS, 0), name


# ---------------------------------------------------------------- empty answers
def outs(*specs):
    """Output arrays of (dtype, length), filled with a value no padding uses."""
    return [np.full(n, 77, dtype) for dtype, n in specs]


def check(arrays, values, name):
    for i, (a, v) in enumerate(zip(arrays, values)):
        want = np.full(a.shape, v, a.dtype) if np.isscalar(v) else np.asarray(v, a.dtype)
        assert np.array_equal(a, want), (name, i, a)


NK = NQ * K
i64, f32, f64, i32 = np.int64, np.float32, np.float64, np.int32
QS = np.arange(NQ * DIM, dtype=np.float32)
Q_OFF = np.array([0, 1, 2], np.int64)  # one sparse term / one token per query
Q_TERMS, Q_WEIGHTS = np.array([1, 2], np.int32), np.array([1.0, 2.0], np.float32)
CODES = np.array([5, 9], np.uint64)
NO_EXAMPLES = np.zeros(NQ + 1, np.int64)


def empty_answers(lib, h):
    """(name, status, output arrays, expected fill of each) for every search family, nq = 2 and k = 3."""
    w = C.byref(TRUE)
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK))
    yield "search_batch_ex", lib.mlvdb_search_batch_ex(h, p(QS), NQ, K, None, p(o[0]), p(o[1]), p(o[2]), p(o[3])), o, (-1, INF, 0, INF)
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK))
    yield "search_batch_where", lib.mlvdb_search_batch_where(h, p(QS), NQ, K, w, p(o[0]), p(o[1]), p(o[2]), p(o[3])), o, \
        (-1, INF, 0, INF)
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK), (i32, 1))
    poq = np.array([0, -1], np.int32)
    yield "search_batch_where_each", lib.mlvdb_search_batch_where_each(h, p(QS), NQ, K, PROGS, 1, p(poq), p(o[0]), p(o[1]), p(o[2]),
                                                                      p(o[3]), p(o[4])), o, (-1, INF, 0, INF, _native.ROUTE_NONE)
    o = outs((i64, NQ + 1), (i64, NQ))
    yield "range_batch_packed", lib.mlvdb_range_batch_packed(h, p(QS), NQ, 1.0, 4, 8, b, b, p(o[0]), p(o[1])), o, (0, 0)
    o = outs((i64, NQ + 1), (i64, NQ))
    yield "range_batch_packed_where", lib.mlvdb_range_batch_packed_where(h, p(QS), NQ, 1.0, 4, 8, w, b, b, p(o[0]), p(o[1])), o, (0, 0)
    o = outs((i64, NQ + 1), (i64, NQ), (i32, 1))
    yield "range_batch_packed_where_each", lib.mlvdb_range_batch_packed_where_each(
        h, p(QS), NQ, 1.0, 4, 8, PROGS, 1, p(poq), b, b, p(o[0]), p(o[1]), p(o[2])), o, (0, 0, _native.ROUTE_NONE)
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK), (i64, NK))
    yield "distinct", lib.mlvdb_search_batch_distinct(h, p(QS), NQ, K, A_INT, 0, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4])), o, \
        (-1, INF, 0, INF, I64_MIN)
    o = outs((i64, NK * 2), (f32, NK * 2), (i32, NQ), (i32, NK), (f64, NK * 2), (i64, NK))
    yield "grouped", lib.mlvdb_search_batch_grouped(h, p(QS), NQ, K, 2, A_INT, 0, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]),
                                                    p(o[5])), o, (-1, INF, 0, 0, INF, I64_MIN)
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK), (i32, NK), (f64, NK))
    yield "mmr", lib.mlvdb_search_batch_mmr(h, p(QS), NQ, K, K, 0.5, w, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(o[5])), o, \
        (-1, INF, 0, INF, -1, INF)
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK), (f32, NQ * DIM))
    yield "like", lib.mlvdb_search_batch_like(h, None, None, p(NO_EXAMPLES), p(QS), NQ, K, 0, None, p(o[0]), p(o[1]), p(o[2]),
                                              p(o[3]), p(o[4])), o, (-1, INF, 0, INF, QS)  # every query is its base row
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK), (i64, NK), (f64, NK))
    yield "maxsim", lib.mlvdb_search_batch_maxsim(h, p(QS), p(Q_OFF), NQ, K, A_INT, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]),
                                                  p(o[5])), o, (I64_MIN, INF, 0, INF, -1, INF)
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK))
    yield "sparse", lib.mlvdb_search_batch_sparse(h, A_SPARSE, p(Q_OFF), p(Q_TERMS), p(Q_WEIGHTS), NQ, K, w, p(o[0]), p(o[1]), p(o[2]),
                                                  p(o[3])), o, (-1, -INF, 0, -INF)  # scores: larger is better
    o = outs((i64, NK), (f32, NK), (i32, NQ), (f64, NK))
    yield "bits", lib.mlvdb_search_batch_bits(h, A_BITS, p(CODES), NQ, 1, _native.BITS_HAMMING, K, w, p(o[0]), p(o[1]), p(o[2]),
                                              p(o[3])), o, (-1, INF, 0, INF)
    o = outs((i64, NK), (f64, NK), (i32, NQ), (f64, NK), (f64, NK), (i32, NK), (i32, NK))
    yield "hybrid", lib.mlvdb_search_batch_hybrid(h, p(QS), A_SPARSE, p(Q_OFF), p(Q_TERMS), p(Q_WEIGHTS), NQ, K, K, K,
                                                  _native.FUSE_CODES["linear"], 1.0, 1.0, 60.0, None, p(o[0]), p(o[1]), p(o[2]),
                                                  p(o[3]), p(o[4]), p(o[5]), p(o[6])), o, (-1, -INF, 0, INF, -INF, -1, -1)


@pytest.mark.parametrize("which", ["empty", "dead"])
def test_nothing_to_find_pads_every_output(hs, which):
    """No row at all, and six rows all tombstoned: every family answers OK with its padding in every array, the optional
    ones included."""
    h = getattr(hs, which)
    seen = []
    for name, status, arrays, values in empty_answers(hs.lib, h):
        assert status == OK, (name, status, hs.lib.mlvdb_last_error(h))
        check(arrays, values, name)
        seen.append(name)
    assert len(seen) == 14
