"""The third wave of call histories: binary vectors, geo columns, attribute statistics and hybrid search on ONE
handle, interleaved with every mutation and query of the wide wave.  ``RecentHistoryModel`` is ``WideHistoryModel`` composed
with the four families' own oracle engines, ``_RecentGenerator`` extends the wide generator by four columns (8 geo, 9 bits,
10 late geo, 11 late bits), two mutations, five queries and six program kinds, and the ``recent`` / ``recent_large``
schedules carry the coverage conditions of tests/test_history_host.py.  ``history_helpers.call`` / ``compare`` / ``_history``
dispatch here for the new op kinds and scales; the op lists of every earlier key are untouched.  Nothing here needs a GPU.

How an answer is compared (no tolerance of this module's own):
  bits     labels, counts, fp32 and fp64 distances, ``bits_get`` and ``list_stats`` in every bit.
  stats    every output byte for byte (min / max only where count > 0; after an overflow: matched, by_absent, n_groups > max).
  geo      boxes, labels, points and counts exactly; radius leaves and the ranking exactly, because the generator checks
           the two guards of tests/geo_helpers.py (G = 1e-10) when it draws the op and redraws (counted) one that trips them;
           distances under 16 x ``geo_helpers.fp64_deviation`` measured over every point and centre of the history.
  hybrid   the dense list obeys the history's near-tie rule at k = fetch_dense (else redrawn, counted); the device's own
           dense and sparse lists equal the model's, so union, ranks and counts are compared exactly; dist64 is the bits of
           ``pair_distances`` and within SCORE_ATOL of the model, sparse64 the bits of ``search_batch_sparse`` and of the model
           (exact weights); labels and fused scores are the bits of ``hybrid_helpers.fuse_lists`` fed with the DEVICE's
           components, and for RRF, which reads ranks only, the model's bits too."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import StatsOverflow
from tests import geo_helpers as GH
from tests import history_helpers as H
from tests.bits_helpers import METRICS, BitsOracleEngine, random_codes
from tests.helpers import SCORE_ATOL
from tests.history_helpers import Refused, Unsupported, _leaf, _max_err64, _same
from tests.hybrid_helpers import METHODS, HybridOracleEngine, fuse_lists
from tests.stats_helpers import MAX_VALUES, StatsOracleEngine
from tests.tags_helpers import eval_list_program

RECENT_SCALES = ("recent", "recent_large")
GEO_A, BITS_A, LATE_GEO, LATE_BITS = 8, 9, 10, 11
GEO_COLUMNS, BITS_COLUMNS = (GEO_A, LATE_GEO), (BITS_A, LATE_BITS)
WORDS, WORDS_FEW = 5, 2          # most rows hold a 5-word code, some a 2-word one
MAX_TOPK = 64                    # MLVDB_MAX_TOPK
MAX_FETCH_DENSE = 1024           # MLVDB_HYBRID_MAX_FETCH_DENSE
BITS_MAX_WORDS = W.BITS_MAX_WORDS
STATS_COLUMNS, BY_COLUMNS = (0, 1, 2), (None, 0, 2)
BITS_MUTATIONS = ("bits_set", "bits_set_at")
RECENT_MUTATIONS = H.WIDE_MUTATIONS + BITS_MUTATIONS
RECENT_NEW_QUERIES = ("search_bits", "bits_get", "search_hybrid", "attr_stats", "geo_nearest")
RECENT_QUERIES = H.WIDE_QUERIES + RECENT_NEW_QUERIES
RECENT_PAIRS = [(m, q) for m in RECENT_MUTATIONS for q in RECENT_QUERIES if m in BITS_MUTATIONS or q in RECENT_NEW_QUERIES]
RECENT_PAIR_SLICES = 12  # recent history `seed` carries RECENT_PAIRS[seed % 12::12]
RECENT_REFUSALS = ("geo_add", "geo_lat_set_attr", "geo_lat_set_attr_at", "geo_lat_update_where", "bits_words0", "bits_words256",
                   "bits_at_repeat", "bits_k65", "hybrid_k_sum", "hybrid_fd1025", "hybrid_not_sparse", "stats_geo", "stats_bits",
                   "stats_groups0", "nearest_window", "facet_geo", "distinct_geo", "ordered_geo", "sparse_on_bits",
                   "list_get_on_bits")
UNSUPPORTED_REFUSALS = ("bits_k65", "hybrid_fd1025")  # MLVDB_ERR_UNSUPPORTED; every other one MLVDB_ERR_INVALID_ARG
RECENT_PROGRAMS = ("radius", "box", "box_anti", "not_radius", "geo_and_scalar", "bits_exists")
PROGRAM_TAKING = ("search_where", "search_each", "range_where", "range_each", "search_distinct", "facet_values", "facet_bins",
                  "where_count", "where_labels", "count_each", "update_where", "tombstone_where", "update_where_list",
                  "where_ordered", "search_mmr", "search_grouped", "search_like", "search_maxsim", "facet_list_values",
                  "search_batch_sparse", "search_bits", "search_hybrid", "attr_stats", "geo_nearest")
ORDER_MAX_ROWS = H.ORDER_MAX_ROWS
WINDOW_FULL, WINDOW_ONE = (50, ORDER_MAX_ROWS - 50), (1, 0)  # (limit, offset): offset + limit = 4096, and limit = 1
CENTRES = ((48.2082, 16.3738), (35.6762, 139.6503), (-1.2921, 36.8219), (64.1466, -21.9426))  # the cluster's centre, by seed
FAR = (-33.8688, 151.2093)
RADII = (0.0, 5.0e3, 3.0e4, 2.5e6, 2.1e7)  # metres; the last one is above pi R: every row that holds a point
BAD_LAT = int(GH.pack(W.GEO_LAT_MAX_E7 + 1, 0))


# ---------------------------------------------------------------- the model
def geo_valid(values) -> bool:
    """Every non-absent value holds a latitude and a longitude inside the ranges of mlvdb_geo.h."""
    v = np.asarray(values, dtype=np.int64).ravel()
    lat, lon = GH.unpack(v[v != GH.ABSENT])
    return bool((np.abs(lat) <= W.GEO_LAT_MAX_E7).all() and (np.abs(lon) <= W.GEO_LON_MAX_E7).all())


class RecentHistoryModel(H.WideHistoryModel, BitsOracleEngine, HybridOracleEngine, StatsOracleEngine, GH.oracle_engine_class()):
    """``WideHistoryModel`` + bits columns, hybrid search, attribute statistics and geo columns, composed from their oracle
    engines: one ``match`` that knows scalar, list and geo leaves and EXISTS on a bits column, the bits pool's capacity
    mirrored like a list's, and the refusals the C ABI makes on the host, all raised before any state changes."""

    # -- programs
    def match(self, program):
        n = self._rows.shape[0]
        stack = []
        for i, (op, attr, a, b) in enumerate(program.ops.tolist()):
            if op in (W.AND, W.OR):
                y, x = stack.pop(), stack.pop()
                stack.append(x & y if op == W.AND else x | y)
            elif op == W.NOT:
                stack.append(~stack.pop())
            elif op == W.TRUE:
                stack.append(np.ones(n, bool))
            else:
                col, kind = self._col(attr), self._kinds[attr]
                if (op in (W.GEO_BOX, W.GEO_RADIUS)) != (kind == "geo") and op != W.EXISTS:
                    raise Refused("a geo op needs a geo column, and a geo column takes GEO_BOX, GEO_RADIUS and EXISTS")
                if kind == "bits" and op != W.EXISTS:
                    raise Refused("a bits column takes EXISTS only")
                if op == W.GEO_BOX:
                    stack.append(GH.box_mask(col, a, b))
                elif op == W.GEO_RADIUS:  # hav against the op's threshold, as the device compares it
                    have = col != GH.ABSENT
                    bit = np.zeros(n, bool)
                    bit[have] = GH.hav(col[have], a) <= GH.LD(np.array([b], np.int64).view(np.float64)[0])
                    stack.append(bit)
                else:
                    stack.append(eval_list_program(W.Program(program.ops[i:i + 1], program.set), self._cols, self._lists, n))
        assert len(stack) == 1
        return stack[0] & ~self._deleted

    # -- which column an entry takes
    def _is(self, attr, kind):
        return self._kinds.get(attr) == kind

    def _value_col(self, attr, what):
        self._col(attr)
        if attr in self._lists or self._is(attr, "geo"):
            raise Refused(f"{what} needs an int64 or float64 value column")

    def _list_col(self, attr, sparse, what):
        if self._is(attr, "bits"):
            raise Refused(f"{what}: a bits column")
        super()._list_col(attr, sparse, what)

    def _group_col(self, attr, what):
        self._value_col(attr, what)
        super()._group_col(attr, what)

    def _geo_write(self, attr, values, what):
        if self._is(attr, "geo") and not geo_valid(values):
            raise Refused(f"{what}: lat_e7 / lon_e7 out of range")

    def set_attr(self, attr, first, values):
        self._geo_write(attr, values, "attr_set")
        return super().set_attr(attr, first, values)

    def set_attr_at(self, attr, labels, values):
        self._geo_write(attr, values, "attr_set_at")
        return super().set_attr_at(attr, labels, values)

    def update_where(self, program, assigns):
        for attr, op, a in assigns:
            if self._is(attr, "geo") and op == _native.SET_ADD:
                raise Refused("attr_update_where: ADD on a geo column")
            self._geo_write(attr, [a], "attr_update_where")
        return super().update_where(program, assigns)

    def facet_values(self, attr, max_values, where=None):
        self._value_col(attr, "facet_values")
        return super().facet_values(attr, max_values, where)

    def facet_bins(self, attr, edges, where=None):
        self._value_col(attr, "facet_bins")
        return super().facet_bins(attr, edges, where)

    def search_distinct(self, queries, k, attr, max_groups=0, where=None, want64=False):
        self._value_col(attr, "search_distinct")
        return super().search_distinct(queries, k, attr, max_groups, where, want64)

    def where_ordered(self, attr, limit, where=None, descending=False, offset=0):
        self._value_col(attr, "where_ordered")
        return super().where_ordered(attr, limit, where, descending, offset)

    # -- binary vectors
    def _bits_col(self, attr, what, words=None):
        if not self._is(attr, "bits"):
            raise Refused(f"{what}: attribute {attr} is no bits column")
        if words is not None and not 1 <= words <= BITS_MAX_WORDS:
            raise Refused(f"{what}: words must be in 1..MLVDB_BITS_MAX_WORDS")

    def bits_set(self, attr, first, col):
        self._bits_col(attr, "bits_set", np.asarray(col.words).shape[1])
        if first < 0 or first + len(col) > self._rows.shape[0]:
            raise Refused("bits_set: rows outside [0, total)")
        super().bits_set(attr, first, col)
        self._grown(attr)

    def bits_set_at(self, attr, labels, col):
        self._bits_col(attr, "bits_set_at", np.asarray(col.words).shape[1])
        self._labels_ok(labels, "bits_set_at")
        n = super().bits_set_at(attr, labels, col)
        self._grown(attr)
        return n

    def bits_get(self, attr, first, n):
        self._bits_col(attr, "bits_get")
        return super().bits_get(attr, first, n)

    def search_bits(self, attr, queries, k, metric="hamming", where=None):
        self._bits_col(attr, "search_bits", np.asarray(queries).shape[1])
        if k < 1 or metric not in METRICS:
            raise Refused("search_bits: k >= 1 and a known metric")
        if k > MAX_TOPK:
            raise Unsupported("search_bits: k above MLVDB_MAX_TOPK")
        if where is not None:
            self.match(where)
        return super().search_bits(attr, queries, k, metric, where)

    # -- hybrid search: the entry's seven outputs, and behind them the same seven at k = fetch_dense + fetch_sparse (the whole
    # completed union with every member's ranks, which the comparison reads)
    def search_hybrid(self, queries, attr, sparse_queries, k, fetch_dense, fetch_sparse, method="rrf", weights=(1.0, 1.0),
                      rrf_k=60.0, where=None, components=True):
        if attr not in self._sparse:
            raise Refused("search_hybrid: no sparse column")
        if k < 1 or fetch_dense < 1 or fetch_sparse < 1:
            raise Refused("search_hybrid: k, fetch_dense and fetch_sparse must be >= 1")
        if k > MAX_TOPK or fetch_dense > MAX_FETCH_DENSE or fetch_sparse > MAX_TOPK:
            raise Unsupported("search_hybrid: k or a fetch size above its limit")
        if k > fetch_dense + fetch_sparse or method not in METHODS:
            raise Refused("search_hybrid: k above fetch_dense + fetch_sparse, or an unknown method")
        if not all(np.isfinite(x) and x >= 0 for x in (*weights, rrf_k)):
            raise Refused("search_hybrid: weights and the RRF constant must be finite and >= 0")
        if where is not None:
            self.match(where)
        full = super().search_hybrid(queries, attr, sparse_queries, fetch_dense + fetch_sparse, fetch_dense, fetch_sparse,
                                     method, weights, rrf_k, where, components=True)
        out = tuple(np.ascontiguousarray(x[:, :k]) if x.ndim == 2 else np.minimum(x, k).astype(x.dtype) for x in full)
        return out + (full,)

    # -- attribute statistics
    def attr_stats(self, attr, by=None, max_groups=1, where=None):
        self._value_col(attr, "attr_stats")
        if by is not None and (by in self._lists or self._is(by, "geo") or self._col(by).dtype != np.int64):
            raise Refused("attr_stats: by needs an int64 column")
        if not 1 <= max_groups <= MAX_VALUES:
            raise Refused("attr_stats: max_groups must be in 1..MLVDB_FACET_MAX_VALUES")
        if where is not None:
            self.match(where)
        return super().attr_stats(attr, by, max_groups, where)

    # -- nearest by distance: the distances stay in long double (the comparison's reference)
    def geo_nearest(self, attr, center, limit, where=None, offset=0):
        if not self._is(attr, "geo") or not geo_valid([center]) or int(center) == GH.ABSENT:
            raise Refused("geo_nearest: a geo column and a valid centre")
        if offset < 0 or limit < 1 or offset + limit > ORDER_MAX_ROWS:
            raise Refused("geo_nearest: 0 <= offset, 1 <= limit, offset + limit <= MLVDB_ORDER_MAX_ROWS")
        mask = self._mask(where)
        top, d, matched, absent = GH.nearest_oracle(self._cols[attr], mask, center)
        top, d = top[offset:offset + limit], d[offset:offset + limit]
        return top.astype(np.int64), self._cols[attr][top], d, matched, absent


# ---------------------------------------------------------------- the values of the four columns
def landmarks(centre_deg):
    """Packed points many rows share: the centre's own coordinates (a radius of 0 matches them, and they tie at distance 0),
    the two poles, and one point on each side of the antimeridian (at different latitudes: no two of them are equally far
    from a pole)."""
    lat, lon = centre_deg
    return GH.quantise([lat, lat, 90.0, -90.0, lat + 1.0, lat - 0.7], [lon, lon, 0.0, 0.0, 179.999, -179.9985])


def geo_values(rng, n, centre_deg):
    """n values of a geo column: 70 % clustered round ``centre_deg`` (sigma 0.2 degrees), 15 % ``landmarks``, the rest uniform
    on the sphere; about 10 % absent."""
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, n)))
    lon = rng.uniform(-180, 180, n)
    r = rng.random(n)
    near = r < 0.7
    lat = np.where(near, np.clip(centre_deg[0] + 0.2 * rng.standard_normal(n), -90, 90), lat)
    lon = np.where(near, (centre_deg[1] + 0.2 * rng.standard_normal(n) + 180) % 360 - 180, lon)
    col = GH.quantise(lat, lon)
    marks = landmarks(centre_deg)
    pick = (r >= 0.7) & (r < 0.85)
    col[pick] = marks[rng.integers(0, marks.size, int(pick.sum()))]
    col[rng.random(n) < 0.10] = GH.ABSENT
    return col


def _alphabet(words):
    return random_codes(np.random.default_rng(7000 + words), 0, words)[1]  # the same per width in every call: distances tie


def bits_codes(rng, n, words):
    """uint64 [n, words] drawn as ``bits_helpers.random_codes`` draws them, from one alphabet per width."""
    base = _alphabet(words)
    codes = rng.integers(0, 2 ** 64, size=(n, words), dtype=np.uint64)
    pick = rng.random(n) < 0.5
    codes[pick] = base[rng.integers(0, base.shape[0], int(pick.sum()))]
    return codes


def bits_column(rng, n, words, p_absent):
    codes = bits_codes(rng, n, words) if 1 <= words <= BITS_MAX_WORDS else np.zeros((n, words), np.uint64)
    return W.BitsColumn(codes, (rng.random(n) >= p_absent).astype(np.uint8))


# ---------------------------------------------------------------- ops: arrays, calls
def is_geo_write(op):
    return op["op"] in ("set_attr", "set_attr_at") and op["attr"] in GEO_COLUMNS


def materialise(model, op):
    """``history_helpers.materialise`` + the arrays of the new kinds and of the geo values the old writers carry."""
    a = H.materialise(model, op)
    kind = op["op"]
    total = model._rows.shape[0]
    rng = np.random.default_rng(op["seed"]) if "seed" in op else None
    if is_geo_write(op) and "values" not in op:
        n = op["n"] if kind == "set_attr" else a["labels"].size
        a["values"] = geo_values(np.random.default_rng([op["seed"], 1]), n, op["centre"])
    elif kind == "bits_set":
        a["col"] = bits_column(rng, op["n"], op["words"], op["p_absent"])
    elif kind == "bits_set_at":
        a["labels"] = H._labels_of(op, rng, total)
        a["col"] = bits_column(rng, a["labels"].size, op["words"], op["p_absent"])
    elif kind == "search_bits":
        a["bq"] = bits_codes(rng, op["nbq"], op["words"])
    elif kind == "search_hybrid":
        a["sq"] = H._sparse_queries(np.random.default_rng(op["sq_seed"]), op["nq"])
    elif kind == "refuse_recent":
        which = op["which"]
        if which in ("bits_words0", "bits_words256"):
            a["col"] = bits_column(rng, 2, 0 if which == "bits_words0" else BITS_MAX_WORDS + 1, 0.0)
        elif which == "bits_at_repeat":
            a["col"] = bits_column(rng, 2, WORDS, 0.0)
        elif which == "bits_k65":
            a["bq"] = bits_codes(rng, 2, WORDS)
        elif which.startswith("hybrid") or which in ("sparse_on_bits",):
            a["sq"] = H._sparse_queries(rng, 3)
    return a


def _stats(e, op, a):
    try:
        return e.attr_stats(op["attr"], op["by"], op["max_groups"], a.get("program"))
    except StatsOverflow as err:  # MLVDB_ERR_OVERFLOW: matched and by_absent are still exact, n_groups is some number above
        return ("overflow", err.n_groups > err.max_groups, err.matched, err.by_absent)


def _refusal(e, op, a):
    """The call of a RECENT_REFUSALS op -> ("refused", status) when it ends in a ``RuntimeError``, else ("accepted",)."""
    which = op["which"]
    lat = np.array([BAD_LAT], np.int64)
    true = H.program_of({"ops": [_leaf(W.TRUE, 0)], "set": []})
    try:
        if which == "geo_add":
            e.update_where(true, [(GEO_A, _native.SET_ADD, 1)])
        elif which == "geo_lat_set_attr":
            e.set_attr(GEO_A, 0, lat)
        elif which == "geo_lat_set_attr_at":
            e.set_attr_at(GEO_A, np.array([0], np.int64), lat)
        elif which == "geo_lat_update_where":
            e.update_where(true, [(GEO_A, _native.SET_ASSIGN, BAD_LAT)])
        elif which in ("bits_words0", "bits_words256"):
            e.bits_set(BITS_A, 0, a["col"])
        elif which == "bits_at_repeat":
            e.bits_set_at(BITS_A, np.array([0, 0], np.int64), a["col"])
        elif which == "bits_k65":
            e.search_bits(BITS_A, a["bq"], MAX_TOPK + 1)
        elif which == "hybrid_k_sum":
            e.search_hybrid(a["qs"], H.SPARSE_A, a["sq"], 5, 2, 2, components=True)
        elif which == "hybrid_fd1025":
            e.search_hybrid(a["qs"], H.SPARSE_A, a["sq"], 5, MAX_FETCH_DENSE + 1, 10, components=True)
        elif which == "hybrid_not_sparse":
            e.search_hybrid(a["qs"], H.LIST_A, a["sq"], 5, 10, 10, components=True)
        elif which == "stats_geo":
            e.attr_stats(GEO_A, None, 1)
        elif which == "stats_bits":
            e.attr_stats(BITS_A, None, 1)
        elif which == "stats_groups0":
            e.attr_stats(2, 0, 0)
        elif which == "nearest_window":
            e.geo_nearest(GEO_A, op["centre"], ORDER_MAX_ROWS, None, 1)
        elif which == "facet_geo":
            e.facet_values(GEO_A, 4096)
        elif which == "distinct_geo":
            e.search_distinct(a["qs"], 5, GEO_A)
        elif which == "ordered_geo":
            e.where_ordered(GEO_A, 5)
        elif which == "sparse_on_bits":
            e.search_batch_sparse(BITS_A, a["sq"], 5)
        elif which == "list_get_on_bits":
            e.get_attr_list(BITS_A, 0, 1)
        else:
            raise ValueError(which)
    except RuntimeError as err:
        return ("refused", H._status_of(err))
    return ("accepted",)


CALLS = {
    "bits_set": lambda e, op, a: e.bits_set(op["attr"], op["first"], a["col"]),
    "bits_set_at": lambda e, op, a: e.bits_set_at(op["attr"], a["labels"], a["col"]),
    "search_bits": lambda e, op, a: e.search_bits(op["attr"], a["bq"], op["k"], op["metric"], a.get("program")),
    "bits_get": lambda e, op, a: e.bits_get(op["attr"], op["first"], op["n"]),
    "search_hybrid": lambda e, op, a: e.search_hybrid(a["qs"], op["attr"], a["sq"], op["k"], op["fd"], op["fs"], method=op["method"],
                                                      weights=tuple(op["weights"]), rrf_k=op["c"], where=a.get("program"),
                                                      components=True),
    "attr_stats": _stats,
    "geo_nearest": lambda e, op, a: e.geo_nearest(op["attr"], op["centre"], op["limit"], a.get("program"), op["offset"]),
    "refuse_recent": _refusal,
}


# ---------------------------------------------------------------- comparison of one answer
NAMES = ("labels", "fused", "counts", "dist64", "sparse64", "rank_dense", "rank_sparse")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _compare_hybrid(e, op, a, got, want, tag, stats):
    lab, fused, cnt, d64, s64, rd, rs = got[:7]
    full = want[7]  # the model's completed union, all of it: labels, fused, count, dist64, sparse64, ranks
    qs, sq, program = a["qs"], a["sq"], a.get("program")
    k, fd, fs, method = op["k"], op["fd"], op["fs"], op["method"]
    _same(cnt, want[2], tag, "counts")
    for name, g, w in zip(NAMES, got[:7], want[:7]):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{tag}: {name}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
    if op.get("lean"):
        # The call whose leftovers the NEXT op must not see (a mask, a shadow, a workspace): nothing else is asked of the
        # engine here.  Such an op is always RRF, which reads ranks alone, so the model's bits are the whole answer.
        assert method == "rrf"
        for i in (0, 1, 4, 5, 6):
            _same(got[i], want[i], tag, f"{NAMES[i]} against the model")
        _max_err64(d64, want[3], tag, stats)
        return
    # the device's own two lists are the model's: the union and every member's ranks are then the model's, exactly
    dl, _, dc, dd64 = e.search64(qs, fd, where=program)
    sl, _, sc, ss64 = e.search_batch_sparse(op["attr"], sq, fs, program)
    pd_s = e.pair_distances(qs, sl)[0]       # the distances of the members the dense list may not hold
    pd_hit = e.pair_distances(qs, lab)[0]    # (padding: label -1 -> +inf, as dist64 pads)
    assert np.array_equal(_bits(d64), _bits(pd_hit)), f"{tag}: dist64 is not the bits of pair_distances"
    score = {}
    for q in range(lab.shape[0]):
        n = int(full[2][q])
        ul, ud, us, urd, urs = (full[i][q, :n] for i in (0, 3, 4, 5, 6))
        by_rank = lambda r: ul[r >= 0][np.argsort(r[r >= 0])]  # noqa: E731
        assert np.array_equal(dl[q, :dc[q]], by_rank(urd)) and (dl[q, dc[q]:] == -1).all(), f"{tag}: query {q}: the dense list differs"
        assert np.array_equal(sl[q, :sc[q]], by_rank(urs)) and (sl[q, sc[q]:] == -1).all(), f"{tag}: query {q}: the sparse list differs"
        hits = lab[q, :cnt[q]]
        assert n >= cnt[q] and np.isin(hits, ul).all(), f"{tag}: query {q}: a hit outside the model's union"
        order = np.argsort(ul)
        at = order[np.searchsorted(ul[order], hits)]
        assert np.array_equal(rd[q, :cnt[q]], urd[at]) and np.array_equal(rs[q, :cnt[q]], urs[at]), f"{tag}: query {q}: ranks differ"
        assert np.array_equal(_bits(s64[q, :cnt[q]]), _bits(us[at])), f"{tag}: query {q}: sparse64 differs from the model's bits"
        in_s = rs[q, :cnt[q]] >= 0
        assert np.array_equal(_bits(s64[q, :cnt[q]][in_s]), _bits(ss64[q, rs[q, :cnt[q]][in_s]])), \
            f"{tag}: query {q}: sparse64 is not what search_batch_sparse reports"
        if cnt[q]:
            err = float(np.abs(d64[q, :cnt[q]] - ud[at]).max())
            stats["max_err64"] = max(stats["max_err64"], err)
            assert err <= SCORE_ATOL, f"{tag}: query {q}: max |dist64 - oracle| {err}"
        score[q] = dict(zip(ul.tolist(), us.tolist()))
        score[q].update({int(l): float(s) for l, s in zip(sl[q, :sc[q]], ss64[q, :sc[q]])})
    for g, pad in ((lab, -1), (fused, -np.inf), (d64, np.inf), (s64, -np.inf), (rd, -1), (rs, -1)):
        assert all((g[q, cnt[q]:] == pad).all() for q in range(lab.shape[0])), f"{tag}: padding differs"

    def dist_of(q, labels):  # a member only the sparse list holds
        return pd_s[q, [int(np.flatnonzero(sl[q] == l)[0]) for l in labels]]

    def score_of(q, labels):  # a member only the dense list holds: exact weights, the model's bits are the score
        return np.array([score[q][int(l)] for l in labels])

    own = fuse_lists(dl, dd64, dc, sl, ss64, sc, dist_of, score_of, k, method, tuple(op["weights"]), op["c"])
    for name, g, w in zip(NAMES, got[:7], own):
        _same(g, w, tag, f"{name} against the fusion of the device's own components")
    if method == "rrf":  # ranks only: the model's bits as well
        for i in (0, 1, 5, 6):
            _same(got[i], want[i], tag, f"{NAMES[i]} against the model")


def compare(e, op, a, got, want, tag, stats):
    """One branch per new kind, by that family's own committed rule."""
    kind = op["op"]
    if kind == "bits_set":
        assert got is None and want is None, f"{tag}: returned {got!r}"
    elif kind == "bits_set_at":
        assert got == want, f"{tag}: {got} rows written, the model {want}"
    elif kind == "search_bits":
        lab, d32, cnt, d64 = got
        _same(lab, want[0], tag, "labels")
        _same(cnt, want[2], tag, "counts")
        _same(d64, want[3], tag, "dist64")
        _same(d32, want[1], tag, "dist32")
    elif kind == "bits_get":
        _same(got[0], want[0], tag, "widths")
        _same(got[1], want[1], tag, "codes")
    elif kind == "attr_stats":
        assert isinstance(got[0], str) == isinstance(want[0], str), f"{tag}: {got[0]!r}, the model {want[0]!r}"
        if isinstance(want[0], str):
            assert tuple(got) == tuple(want), f"{tag}: {got}, the model {want}"
        else:
            for i, name in ((0, "keys"), (1, "rows"), (2, "count"), (5, "sum_hi"), (6, "sum_lo")):
                _same(got[i], want[i], tag, name)
            has = want[2] > 0  # min / max are unspecified where nothing is present
            for i, name in ((3, "min"), (4, "max")):
                assert got[i].dtype == want[i].dtype and got[i].shape == want[i].shape, f"{tag}: {name}: {got[i].dtype}{got[i].shape}"
                _same(got[i][has], want[i][has], tag, name)
            assert tuple(got[7:]) == tuple(want[7:]), f"{tag}: (matched, by_absent) {got[7:]}, the model {want[7:]}"
    elif kind == "geo_nearest":
        _same(got[0], want[0], tag, "labels")
        _same(got[1], want[1], tag, "points")
        assert tuple(got[3:]) == tuple(want[3:]), f"{tag}: (matched, absent) {got[3:]}, the model {want[3:]}"
        d, wd = np.asarray(got[2]), np.asarray(want[2], dtype=GH.LD)
        assert d.shape == wd.shape and np.array_equal(d == 0, wd == 0), f"{tag}: zero distances differ"
        nz = wd > 0
        if nz.any():
            dev = float(np.max(np.abs(d[nz].astype(GH.LD) - wd[nz]) / wd[nz]))
            stats["geo_dev"] = max(stats.get("geo_dev", 0.0), dev)
            print(f"{tag}: distance deviation {dev:.3e}, bar {a['tol']:.3e}")
            assert dev <= a["tol"], f"{tag}: distance deviates by {dev:.3e} relative, bar {a['tol']:.3e}"
    elif kind == "search_hybrid":
        _compare_hybrid(e, op, a, got, want, tag, stats)
    elif kind == "refuse_recent":
        assert tuple(got) == tuple(want), f"{tag}: {got}, the model {want}"
    else:
        raise ValueError(kind)


# ---------------------------------------------------------------- generation
def has_recent_leaf(program):
    """A geo op, or EXISTS on a bits column, in a program's JSON form."""
    return any(o[0] in (W.GEO_BOX, W.GEO_RADIUS) or (o[0] == W.EXISTS and o[1] in BITS_COLUMNS) for o in program["ops"])


def programs_of(op):
    return ([op["program"]] if op.get("program") else []) + op.get("programs", [])


class _RecentGenerator(H._WideGenerator):
    """The generator over RECENT_MUTATIONS / RECENT_QUERIES: the wide columns 0 to 5 and 8 geo, 9 bits, 10 late geo, 11 late
    bits; the wide program pool and RECENT_PROGRAMS in every program-taking op; schedules of its own."""

    PROGRAMS = H._WideGenerator.PROGRAMS + RECENT_PROGRAMS + ("late_geo",)

    def __init__(self, seed, space, d, scale):
        assert scale in RECENT_SCALES
        super().__init__(seed, space, d, "wide_large" if scale == "recent_large" else "wide")  # (read for the size of appends alone)
        self.rng = np.random.default_rng([seed, d, H.SPACES.index(space), 16 + RECENT_SCALES.index(scale)])
        self.model = RecentHistoryModel(d, space)
        self.centre = CENTRES[seed % len(CENTRES)]
        marks = landmarks(self.centre)
        self.centres = [int(x) for x in (marks[0], marks[4], GH.quantise([FAR[0]], [FAR[1]])[0],
                                         GH.quantise([self.centre[0] + 0.05], [self.centre[1] - 0.03])[0])]
        self.defined10 = False
        self.points, self.asked = [], set()  # every geo value written and every centre asked: the pool the distance bar is measured over
        self.geo_tol = 0.0
        self.only_recent = False

    # -- plumbing
    def emit(self, op):
        for p in programs_of(op):  # the radius guard holds for the state the program is evaluated on
            assert self._radius_ok(p), f"radius guard tripped at emission: {op}"
        args = materialise(self.model, op)
        exp = {"args": args}
        kind = op["op"]
        if kind == "bits_set_at":  # what the host conditions read: the widths the rows held, and how many of them are dead
            rows = self.model._lists[op["attr"]]
            exp["widths_before"] = [0 if rows[l] is None else len(rows[l]) for l in args["labels"].tolist()]
            exp["dead"] = int(self.model._deleted[args["labels"]].sum())
        if is_geo_write(op):
            self.points.append(args["values"].copy())
        if kind == "update_where":
            self.points.append(np.array([a for attr, _, a in op["assigns"] if attr in GEO_COLUMNS], np.int64))
        if kind == "geo_nearest":
            self.asked.add(op["centre"])
        exp["want"] = H.call(self.model, op, args)
        if kind in RECENT_MUTATIONS:
            exp["counts"] = self.model.counts()
        exp["pools"] = self.model.pools()
        self.ops.append(op)
        self.expected.append(exp)
        return exp["want"]

    def finish(self):
        """The bar of every returned distance: 16 x the fp64 deviation over the history's own points and centres."""
        points = np.unique(np.concatenate(self.points + [np.zeros(0, np.int64)]))
        self.geo_tol = 16 * GH.fp64_deviation(points, sorted(self.asked)) if self.asked else 0.0
        for op, exp in zip(self.ops, self.expected):
            if op["op"] == "geo_nearest":
                exp["args"]["tol"] = self.geo_tol

    # -- columns
    def attrs(self):  # the scalar value columns
        return [a for a in super().attrs() if a not in GEO_COLUMNS]

    def geo_attrs(self):
        return [a for a in GEO_COLUMNS if a in self.model._cols]

    def bits_attrs(self):
        return [a for a in BITS_COLUMNS if a in self.model._cols]

    def pooled(self, sparse=None):
        return [a for a in super().pooled(sparse) if a not in BITS_COLUMNS]

    def set_geo(self, attr, first):
        first = min(first, self.total)
        self.emit({"op": "set_attr", "attr": int(attr), "first": int(first), "n": int(self.total - first), "seed": self._seed(),
                   "centre": list(self.centre)})

    def set_geo_at(self, attr, **extra):
        return self.emit({"op": "set_attr_at", "attr": int(attr), "n": int(self.rng.integers(1, 40)), "seed": self._seed(),
                          "centre": list(self.centre), **extra})

    def bits_set(self, attr, first, words=WORDS, p_absent=0.1):
        first = min(first, self.total)
        self.emit({"op": "bits_set", "attr": int(attr), "first": int(first), "n": int(self.total - first), "words": int(words),
                   "p_absent": p_absent, "seed": self._seed()})

    def bits_set_at(self, attr, n=None, lo=0, words=WORDS, p_absent=0.1, **extra):
        n = int(self.rng.integers(1, 60)) if n is None else int(n)
        return self.emit({"op": "bits_set_at", "attr": int(attr), "n": n, "lo": int(lo), "words": int(words), "p_absent": p_absent,
                          "seed": self._seed(), **extra})

    def set_bits(self, attr, first):
        """Most rows of the span a 5-word code (about 10 % none), then about a seventh of them a 2-word one."""
        first = min(first, self.total)
        self.bits_set(attr, first)
        if self.total > first:
            self.bits_set_at(attr, n=max(1, (self.total - first) // 7), lo=first, words=WORDS_FEW)

    def set_attrs(self):
        super().set_attrs()
        first = max(0, self.last_first - int(self.rng.integers(0, 60)))
        for attr in self.geo_attrs():
            self.set_geo(attr, first)
        for attr in self.bits_attrs():
            self.set_bits(attr, first)

    def append(self, mode=None, n=None):
        if self.scale == "wide" and self.total > 1400:  # stay under MAX_ROWS_WIDE: drop most rows first
            self.emit({"op": "tombstone", "mode": "frac", "seed": self._seed(), "frac": 0.7})
            self.compact()
        super().append(mode, n)

    # -- programs: the wide kinds and the six new ones; a radius leaf is kept only if the radius guard holds
    def _radius_ok(self, program):
        for attr, centre, radius in program.get("radii", []):
            try:
                GH.radius_mask(self.model._cols[attr], centre, radius)
            except AssertionError:
                return False
        return True

    def _radius(self, attr, centre=None, radius=None):
        centre = self.centres[self.rng.integers(len(self.centres))] if centre is None else centre
        radius = float(RADII[self.rng.integers(len(RADII))] if radius is None else radius)
        return _leaf(W.GEO_RADIUS, attr, centre, W.float_bits(W.geo_radius_threshold(radius))), [int(attr), int(centre), radius]

    def _program(self, which):
        rng = self.rng
        lat, lon = self.centre
        if which == "late_geo":
            which, attr = "radius", (LATE_GEO if self.defined10 else GEO_A)
        else:
            attr = GEO_A
        if which == "bits_exists":
            return {"ops": [_leaf(W.EXISTS, BITS_A)], "set": []}
        if which == "box":
            h = float(rng.choice([0.1, 0.3, 2.0]))
            sw, ne = GH.quantise([lat - h, lat + h], [lon - h, lon + h / 2])
            return {"ops": [_leaf(W.GEO_BOX, attr, sw, ne)], "set": []}
        if which == "box_anti":  # lon_sw > lon_ne: across the antimeridian
            sw, ne = GH.quantise([lat - 5.0, lat + 5.0], [179.5, -179.5])
            return {"ops": [_leaf(W.GEO_BOX, attr, sw, ne)], "set": []}
        leaf, radii = self._radius(attr, radius=3.0e4 if which == "geo_and_scalar" else None)
        if which == "radius":
            ops = [leaf]
        elif which == "not_radius":
            ops = [leaf, _leaf(W.NOT, 0)]
        elif which == "geo_and_scalar":
            ops = [leaf, _leaf(W.LT, 2, 8), _leaf(W.AND, 0)]
        else:
            raise ValueError(which)
        return {"ops": ops, "set": [], "radii": [radii]}

    def program(self, which=None):
        pool = RECENT_PROGRAMS if self.only_recent else self.PROGRAMS
        which = which or pool[self.rng.integers(len(pool))]
        if which not in RECENT_PROGRAMS + ("late_geo",):
            return super().program(which)
        while True:
            self.drawn += 1
            p = self._program(which)
            if self._radius_ok(p):
                return p
            self.redraws += 1

    def each(self, nq, which=None):
        if which is None and (self.only_recent or self.rng.random() < 0.5):
            which = ("nothing", "radius", "half", "geo_and_scalar")
        return super().each(nq, which)

    # -- mutations
    def update_where(self, assigns=None, program=None):
        if assigns is None and self.rng.random() < 0.3:
            assigns = [[GEO_A, _native.SET_ASSIGN, (self.centres[self.rng.integers(len(self.centres))], int(GH.ABSENT))[self.rng.integers(2)]]]
        return super().update_where(assigns, program)

    def tombstone_where(self, which=None):
        kinds = ("radius", "box") if self.only_recent else ("few", "has_all", "groups", "tag_and_scalar", "len", "radius", "box")
        which = which or kinds[self.rng.integers(len(kinds))]
        return super().tombstone_where(which)

    def mutate(self, kind):
        rng = self.rng
        if kind == "bits_set":
            return self.bits_set(BITS_A, int(rng.integers(0, max(self.total, 1))), words=(WORDS, WORDS, WORDS_FEW)[rng.integers(3)])
        if kind == "bits_set_at":
            return self.bits_set_at(BITS_A, words=(WORDS, WORDS_FEW)[rng.integers(2)])
        if kind == "set_attr" and rng.random() < 0.3:
            return self.set_geo(GEO_A, int(rng.integers(0, self.total + 1)))
        if kind == "set_attr_at" and rng.random() < 0.3:
            return self.set_geo_at(GEO_A)
        return super().mutate(kind)

    # -- queries
    def _hybrid_ok(self, op):
        return self._knn_ok({**op, "k": op["fd"]})

    def _nearest_ok(self, op):
        m = self.model
        mask = ~m._deleted if op.get("program") is None else m.match(H.program_of(op["program"]))
        try:
            GH.nearest_oracle(m._cols[op["attr"]], mask, op["centre"])
        except AssertionError:
            return False
        return True

    def query(self, kind, **kw):
        rng, total = self.rng, self.total
        if kind not in RECENT_NEW_QUERIES:
            return super().query(kind, **kw)
        program = kw.pop("program", "random")
        if program == "random":
            program = self.program() if rng.random() < 0.5 else None
        if kind == "search_bits":
            return self.emit({"op": kind, "attr": kw.pop("attr", BITS_A), "nbq": int(kw.pop("nq", (1, 3, 9)[rng.integers(3)])),
                              "words": int(kw.pop("words", (WORDS, WORDS, WORDS_FEW, 3)[rng.integers(4)])),
                              "metric": METRICS[rng.integers(2)], "k": int(kw.pop("k", (1, 10, 64)[rng.integers(3)])),
                              "seed": self._seed(), "program": program})
        if kind == "bits_get":
            first = int(kw.pop("first", rng.integers(0, total + 1)))
            return self.emit({"op": kind, "attr": kw.pop("attr", BITS_A), "first": first,
                              "n": int(min(total - first, kw.pop("n", rng.integers(0, 300))))})
        if kind == "search_hybrid":
            nq = int(kw.pop("nq", (1, 3, 12)[rng.integers(3)]))
            shapes = ((1, 1, 1), (10, 40, 20), (64, 64, 64), (5, 3, 64), (10, 65, 5), (64, 1024, 64))
            k, fd, fs = kw.pop("shape", None) or shapes[rng.integers(len(shapes))]
            lean = bool(kw.pop("lean", False))  # (compared against the model alone: see _compare_hybrid)
            method = "rrf" if lean else METHODS[rng.integers(3)]
            weights = ((1.0, 1.0), (0.75, 1.3), (2.0, 0.0), (0.0, 1.5))[rng.integers(4)]
            c = float((60.0, 7.5, 0.0)[rng.integers(3)])
            return self._draw(lambda: {"op": kind, "attr": H.SPARSE_A, "nq": nq, "k": k, "fd": fd, "fs": fs, "method": method,
                                       "weights": list(weights), "c": c, "seed": self._seed(), "sq_seed": self._seed(),
                                       "program": program, **({"lean": True} if lean else {})}, self._hybrid_ok)
        if kind == "attr_stats":
            attr = kw.pop("attr", STATS_COLUMNS[rng.integers(3)])
            by = kw.pop("by", BY_COLUMNS[rng.integers(3)])
            return self.emit({"op": kind, "attr": attr, "by": by, "max_groups": int(kw.pop("max_groups", 1 if by is None else 4096)),
                              "program": program})
        if kind == "geo_nearest":
            attr = kw.pop("attr", GEO_A)
            window = kw.pop("window", None)
            while True:
                self.drawn += 1
                limit, offset = window or ((1, 0), (20, 0), (5, 7), (ORDER_MAX_ROWS, 0), WINDOW_FULL)[rng.integers(5)]
                op = {"op": kind, "attr": attr, "centre": self.centres[rng.integers(len(self.centres))], "limit": limit,
                      "offset": offset, "program": program}
                if self._nearest_ok(op):
                    return self.emit(op)
                self.redraws += 1
        raise ValueError(kind)

    def refuse(self, which, **extra):
        if which not in RECENT_REFUSALS:
            return super().refuse(which, **extra)
        op = {"op": "refuse_recent", "which": which, "seed": self._seed()}
        if which.startswith("hybrid") or which == "distinct_geo":
            op["nq"] = 3
        if which == "nearest_window":
            op["centre"] = self.centres[0]
        return self.emit(op)

    def tagged(self, kind):
        """One op of a program-taking kind whose program holds a geo leaf or EXISTS on the bits column."""
        self.only_recent = True
        try:
            for _ in range(16):
                self.ensure_rows()
                if kind in RECENT_MUTATIONS:
                    self.mutate(kind)
                elif kind in self.TAKES_PROGRAM:
                    self.query(kind, program=self.program())
                else:
                    self.query(kind)
                if any(has_recent_leaf(p) for p in programs_of(self.ops[-1])):
                    return
        finally:
            self.only_recent = False
        raise AssertionError(f"no program with a new leaf drawn for {kind}")

    # -- the schedules
    TAKES_PROGRAM = ("search_where", "search_distinct", "where_count", "where_labels", "where_ordered", "search_mmr",
                     "search_grouped", "search_like", "search_maxsim", "facet_list_values", "search_batch_sparse", "search_bits",
                     "search_hybrid", "attr_stats", "geo_nearest")  # the kinds whose ``query`` takes the program as given

    def _ask_new(self):
        """The five new queries, without a program."""
        self.query("search_bits", words=WORDS, program=None)
        self.query("bits_get", first=0, n=200)
        self.query("search_hybrid", program=None)
        self.query("attr_stats", program=None)
        self.query("geo_nearest", program=None)

    def _define(self):
        for attr, kind in ((0, "int64"), (1, "float64"), (2, "int64"), (H.LIST_A, "int64_list"), (H.SPARSE_A, "sparse"),
                           (GEO_A, "geo"), (BITS_A, "bits")):
            self.emit({"op": "define_attr", "attr": attr, "kind": kind})

    def recent(self):
        rng, seed = self.rng, self.seed
        self._define()
        self.append("hundreds")
        self.set_attrs()
        items = [lambda m=m, q=q: (self.ensure_rows(), self.mutate(m), self.query(q))
                 for m, q in RECENT_PAIRS[seed % RECENT_PAIR_SLICES::RECENT_PAIR_SLICES]]

        def garbage(tombstones):  # the bits pool: a compaction with garbage in it
            self.ensure_rows()
            if not tombstones and self.model.counts()[1]:
                self.compact()
            for _ in range(2):  # half the rows overwritten twice: their old codes stay behind in the pool
                self.bits_set_at(BITS_A, n=max(1, self.live.size // 2))
            if tombstones:
                self.tombstone("frac")
            self.compact()
            self.query("search_bits", words=WORDS, program=None)
            self.query("list_stats", attr=BITS_A)

        def doubling():  # the bits pool regrows twice while it holds live codes
            self.ensure_rows(300)
            self.compact()
            lo = self.total // 2  # rows [0, lo) keep what they held before the first regrowth
            cap, grown = self.model._pool_cap[BITS_A], 0
            for _ in range(16):
                used = self.model._pool_used[BITS_A]
                self.bits_set_at(BITS_A, n=self.total - lo, lo=lo)
                if self.model._pool_cap[BITS_A] != cap and used > 0:
                    cap, grown = self.model._pool_cap[BITS_A], grown + 1
                if grown >= 2:
                    break
            assert grown >= 2
            self.query("bits_get", first=0, n=lo)
            self.query("search_bits", words=WORDS, program=None)

        def width(p_absent):  # rows of 5 words rewritten with 2 words, or made absent; both widths are searched at once
            self.ensure_rows()
            rows = self.model._lists[BITS_A]
            five = [int(i) for i in self.live if rows[i] is not None and len(rows[i]) == WORDS]
            if len(five) < 40:
                self.set_bits(BITS_A, 0)
                rows = self.model._lists[BITS_A]
                five = [int(i) for i in self.live if rows[i] is not None and len(rows[i]) == WORDS]
            labels = [int(x) for x in rng.choice(five, min(40, len(five)), replace=False)]
            self.bits_set_at(BITS_A, words=WORDS_FEW, p_absent=p_absent, labels=labels, n=len(labels))
            self.query("search_bits", words=WORDS, program=None)
            self.query("search_bits", words=WORDS_FEW, program=None)

        def regrowth():  # two regrowths of the rows with values present, then every new reader
            self.ensure_rows()
            for _ in range(2):
                self.append("cross")
                self.set_attrs()
            self.query("bits_get", first=0, n=200)
            self.query("search_bits", words=WORDS)
            self.query("geo_nearest")
            self.query("where_count", program=self.program("radius"))
            self.query("attr_stats", by=(0, 2)[rng.integers(2)])
            self.query("search_hybrid")

        def empty(how):  # emptied, the five new queries, rows again, the five, their values, the five again
            self.ensure_rows()
            if how == "compact":
                self.tombstone_where("true")
                self.compact()
            else:
                self.reset(how == "reset_other")
            self._ask_new()
            self.append("hundreds")
            self._ask_new()  # rows without a value yet: what the emptying left behind would show here
            self.set_attrs()
            self._ask_new()

        def hybrid_across(big, x):  # hybrid on the filter route, mutations, hybrid again
            self.ensure_rows()
            self.strategy("filter")
            shape = ((10, 65, 5), (64, 1024, 64))[rng.integers(2)] if big else ((10, 40, 20), (64, 64, 64))[rng.integers(2)]
            self.query("search_hybrid", shape=shape, lean=True)
            if x == "regrowth":
                self.append("cross")
            elif x == "compact":
                self.tombstone("few")
                self.compact()
            else:
                {"tombstone_where": self.tombstone_where, "tombstone": self.tombstone, "append": self.append}[x]()
            self.query("search_hybrid", shape=shape)
            self.strategy("auto")

        def l2_hybrid():  # two hybrid calls of different nq, tombstone_where, a plain search: the offsets plane
            if self.model.space != "l2":
                self.reset_to("l2")
            self.ensure_rows()
            self.strategy("filter")
            self.query("search_hybrid", nq=12, shape=(10, 40, 20), lean=True)
            self.query("search_hybrid", nq=3, shape=(10, 40, 20), lean=True)
            self.tombstone_where("few")
            self.query("search", nq=12, k=10)
            self.strategy("auto")

        def masked(kind):  # the mask is handed back: a plain search, and the same call without a program
            self.ensure_rows()
            for after in ("search64", kind):
                self.query(kind, program=self.program(("half", "radius", "geo_and_scalar", "box")[rng.integers(4)]),
                           **({"lean": True} if kind == "search_hybrid" else {}))
                self.query(after) if after == "search64" else self.query(kind, program=None)

        def workspace():  # where_ordered and geo_nearest share one workspace: windows of 4096 and of 1, both ways round
            self.ensure_rows()

            def ordered(attr, window):
                self.emit({"op": "where_ordered", "attr": attr, "limit": window[0], "offset": window[1],
                           "descending": bool(rng.random() < 0.5), "program": None})

            ordered(2, WINDOW_FULL)
            self.query("geo_nearest", window=WINDOW_ONE, program=None)
            ordered(1, WINDOW_FULL)
            self.query("geo_nearest", window=WINDOW_FULL, program=None)
            ordered(0, WINDOW_ONE)

        def tables():  # the statistics table is grow-only and sized by max_groups
            self.ensure_rows()
            by = (0, 2)[rng.integers(2)]
            groups = int(self.model.attr_stats(1, by, MAX_VALUES)[0].size)
            assert groups >= 2
            self.query("attr_stats", attr=1, by=by, max_groups=MAX_VALUES, program=None)
            self.query("attr_stats", attr=0, by=by, max_groups=groups, program=None)
            assert self.query("attr_stats", attr=1, by=by, max_groups=groups - 1, program=None)[0] == "overflow"
            self.query("attr_stats", attr=2, by=by, max_groups=groups, program=None)
            self.query("facet_values", attr=by)
            self.query("attr_stats", attr=1, by=by, program=None)
            self.query("facet_values", attr=by)

        def writers(which):  # a writer, then at once the reader of what it wrote
            self.ensure_rows()
            if which in ("geo_assign>geo_nearest", "geo_assign>radius"):
                target = self.centres[3]
                self.update_where([[GEO_A, _native.SET_ASSIGN, target]], self.program("half"))
                if which.endswith("nearest"):
                    self.query("geo_nearest", program=None)
                else:
                    self.query("where_count", program=self._program_at(target, 0.0))
            elif which == "by>attr_stats":
                by = (0, 2)[rng.integers(2)]
                self.set_attr_at(by)
                self.query("attr_stats", by=by)
            elif which == "float_add>attr_stats":
                self.update_where([[1, _native.SET_ADD, W.float_bits(0.5)]], self.program("half"))
                self.query("attr_stats", attr=1)
            elif which == "sparse_at>search_hybrid":
                self.set_pooled_at(H.SPARSE_A)
                self.query("search_hybrid")
            elif which == "bits_at_dead>search_bits":
                if not self.model.counts()[1]:
                    self.tombstone("few")
                dead = np.flatnonzero(self.model._deleted)[:3].tolist()
                labels = dead + [int(x) for x in self.live[:20]]
                self.bits_set_at(BITS_A, labels=labels, n=len(labels))
                self.query("search_bits", words=WORDS)
            else:
                self.tombstone_where("radius")
                self.query(which.split(">")[1], **({"words": WORDS} if which.endswith("search_bits") else {}))

        def late_columns():  # columns 10 and 11, defined when rows exist: all absent, then written
            self.ensure_rows()
            self.emit({"op": "define_attr", "attr": LATE_GEO, "kind": "geo"})
            self.emit({"op": "define_attr", "attr": LATE_BITS, "kind": "bits"})
            self.defined10 = True
            for phase in range(2):
                self.query("geo_nearest", attr=LATE_GEO, program=None)
                self.query("where_count", program=self.program("late_geo"))
                self.query("search_bits", attr=LATE_BITS, words=WORDS, program=None)
                self.query("bits_get", attr=LATE_BITS, first=0, n=200)
                if phase == 0:
                    self.set_geo(LATE_GEO, 0)
                    self.set_bits(LATE_BITS, 0)

        def refusals():  # every refusal is followed at once by a query
            self.ensure_rows()
            for i, which in enumerate(RECENT_REFUSALS):
                if i % 2 == seed % 2:
                    self.refuse(which)
                    self.query(("search64", "search_bits", "geo_nearest", "attr_stats", "search_hybrid", "bits_get")[rng.integers(6)])

        across = [(False, x) for x in ("tombstone_where", "tombstone", "append", "compact")] + [(True, "compact"), (True, "regrowth")]
        pairs = ("geo_assign>geo_nearest", "geo_assign>radius", "by>attr_stats", "float_add>attr_stats", "sparse_at>search_hybrid",
                 "bits_at_dead>search_bits", "tombstone_radius>attr_stats", "tombstone_radius>geo_nearest", "tombstone_radius>search_bits")
        items += [lambda: garbage(seed % 2 == 0), doubling, lambda: width(0.0 if seed % 2 == 0 else 1.0), regrowth,
                  lambda: empty(("reset", "reset_other", "compact")[seed % 3]), late_columns, refusals, workspace, tables,
                  lambda: masked(("search_hybrid", "search_bits")[seed % 2])]
        items += [lambda c=across[(3 * seed + i) % 6]: hybrid_across(*c) for i in range(3)]
        items += [lambda w=w: writers(w) for w in pairs[seed % 2::2]]
        items += [lambda kind=kind: self.tagged(kind) for kind in PROGRAM_TAKING[seed % 12::12]]
        if self.model.space == "l2":
            items.append(l2_hybrid)
        items += [lambda: (self.ensure_rows(), self.query(RECENT_QUERIES[rng.integers(len(RECENT_QUERIES))])) for _ in range(4)]
        for i in rng.permutation(len(items)):
            items[i]()
        self.finish()

    def _program_at(self, centre, radius):
        leaf, radii = self._radius(GEO_A, centre, radius)
        return {"ops": [leaf], "set": [], "radii": [radii]}

    def recent_large(self):
        """The pattern of ``wide_large()`` over the four families: appends of 12,000 rows until past 32,768 (`auto` moves hybrid's
        dense leg to the filter route at nq = 12 and 40 with fetch_dense <= 64), fetch_dense = 65 and 1024 on each side, a
        ``tombstone_where`` of about a third of the rows through a geo box, a compaction back below, growth again."""
        self._define()
        lat, lon = self.centre
        small, paged, deep = (10, 40, 20), (10, 65, 5), (64, 1024, 64)
        self.append(n=12000)
        self.set_attrs()
        self.query("search_hybrid", nq=12, shape=small, program=None)  # below the threshold: the exact scan inside
        self.query("search_hybrid", nq=3, shape=paged, program=None)
        self.query("search_hybrid", nq=3, shape=deep, program=self.program("half"))
        for _ in range(2):
            self.append(n=12000)
            self.set_attrs()
        self.query("search_hybrid", nq=12, shape=small, program=None)
        self.query("search_hybrid", nq=40, shape=(64, 64, 64), program=self.program("geo_and_scalar"))
        self.query("search_hybrid", nq=3, shape=paged, program=None)
        self.query("search_hybrid", nq=3, shape=deep, program=None)
        self.query("search_bits", words=WORDS, k=10, program=None)
        self.query("bits_get")
        self.query("attr_stats", attr=1, by=0, program=None)
        self.query("geo_nearest", window=WINDOW_FULL, program=None)
        sw, ne = GH.quantise([lat - 2.0, lat + 2.0], [lon - 2.0, lon])
        self.emit({"op": "tombstone_where", "program": {"ops": [_leaf(W.GEO_BOX, GEO_A, sw, ne)], "set": []}})
        self.query("search_hybrid", nq=12, shape=small, program=self.program("box"))
        self.query("geo_nearest", program=None)
        self.compact()
        assert self.total < H.FILTER_MIN_ROWS
        self.query("search_hybrid", nq=12, shape=small, program=None)
        self.query("attr_stats", attr=2, by=None, program=self.program("radius"))
        self.append(n=12000)
        assert self.total > H.FILTER_MIN_ROWS
        self.set_attrs()
        self.query("search_hybrid", nq=12, shape=small, program=None)
        self.query("search_hybrid", nq=40, shape=small, program=self.program("bits_exists"))
        self.query("search_bits", words=WORDS_FEW, k=64, program=self.program("radius"))
        self.query("attr_stats", attr=0, by=2, program=None)
        self.query("geo_nearest", program=self.program("half"))
        self.finish()


# The committed seed set: (seed, space, d, scale).
RECENT = [(500 + 2 * i + j, space, d, "recent") for i, (space, d) in
          enumerate([("l2", 20), ("cosine", 64), ("ip", 128), ("l2", 256), ("cosine", 100), ("ip", 48)]) for j in range(2)]
RECENT_LARGE = [(600 + i, space, 64, "recent_large") for i, space in enumerate(H.SPACES)]


def geo_bar(seed, space, d, scale):
    """The relative bar of the history's returned distances (16 x the fp64 deviation over its own points and centres)."""
    return H._history(seed, space, d, scale).geo_tol
