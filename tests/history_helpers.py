"""Seeded call histories on ONE engine handle, replayed against a NumPy model of the whole engine.

``HistoryModel`` is one oracle engine with every entry point of ``HipScanEngine``; ``make_history`` builds a list of plain,
JSON-serialisable ops from a shuffled schedule (the coverage conditions of tests/test_history_host.py) padded with random
steps, running the model as it goes, and returns the ops with the model's answers; ``run_history`` applies them to an engine
one by one and compares every answer at once.  The ``wide`` and ``wide_large`` scales (``WideHistoryModel``, ``_WideGenerator``)
do the same over the entry families added since -- ordered, diversified, grouped, by-example and late-interaction queries,
updates and filtered deletes, list and sparse columns -- with op tuples, a program pool and schedules of their own, so that the
first histories keep generating the op lists they always did.  The ``recent`` scales (bits, geo, statistics, hybrid) live in
tests/history_recent_helpers.py; ``call``, ``compare`` and ``_history`` dispatch there.  Nothing here needs a GPU."""
from __future__ import annotations

import functools
import json
import re

import numpy as np

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import FacetOverflow
from oracle import exact_scan
from tests import distinct_helpers, order_helpers
from tests.distinct_helpers import ABSENT, DistinctOracleEngine
from tests.facet_helpers import FacetOracleEngine
from tests.grouped_helpers import MAX_GROUP_SIZE, GroupedOracleEngine, check_grouped
from tests.helpers import SCORE_ATOL, assert_knn_matches, assert_range_matches
from tests.like_helpers import LikeOracleEngine, cosine_query_bound, example_sets, like_queries, like_strip, most_examples
from tests.maxsim_helpers import MAX_TOKENS, MaxSimOracleEngine, check_maxsim, maxsim_oracle, offsets_of
from tests.mmr_helpers import D64_BOUND, GAP_MIN, MmrOracleEngine, mmr_select
from tests.sparse_helpers import SparseOracleEngine, random_corpus, random_vector, sparse_csr
from tests.tags_helpers import csr
from tests.where_helpers import FLOAT_POOL, EachOracleEngine, EachRangeOracleEngine

SPACES = ("l2", "cosine", "ip")
SCALES = ("small", "large", "multi")
WIDE_SCALES = ("wide", "wide_large")  # the entry families added since: ops, programs and schedules of their own
TILE_ROWS = 768          # layout.h: kTileRows, the granule of the row capacity
FILTER_MIN_ROWS = 32768  # api.hip: use_filter, the corpus at which `auto` takes the filter route for nq >= 12
MAX_ROWS_SMALL = 6000
MAX_ROWS_WIDE = 2400   # what a wide history stays under: its appends are hundreds of rows, two capacity crossings at most
TIE_REL = 1e-9           # near-ties: the device's and the oracle's fp64 sums differ by far less (d 2^-53 sum|terms| < 1e-10)
WHERE_GATHER_VALUES = (0, 150, 1 << 30)  # never / the default / always (internal.h)
MUTATIONS = ("append", "set_attr", "define_attr", "tombstone", "compact", "reset", "set_strategy", "set_tuning")
QUERIES = ("search", "search64", "search_mask", "search_where", "search_each", "range", "range_where", "range_each",
           "search_distinct", "facet_values", "facet_bins", "where_count", "where_labels", "count_each", "pair_distances",
           "get_rows", "get_rows_at", "get_attr", "counts")
# what MultiDeviceEngine implements
MULTI_QUERIES = ("search", "search64", "search_mask", "range", "pair_distances", "get_rows", "get_rows_at", "counts")
REFUSALS = ("k0", "distinct_float", "facet_max0", "edges_unsorted", "undefined", "facet_overflow", "range_small")
ATTR_READERS = ("search_where", "search_each", "range_where", "range_each", "search_distinct", "facet_values", "facet_bins",
                "where_count", "where_labels", "count_each", "get_attr")
PAIRS = [(m, q) for m in MUTATIONS for q in QUERIES]
PAIR_SLICES = 10  # history `seed` carries PAIRS[seed % 10::10]


def capacity_after(cap: int, total_needed: int) -> int:
    """Row capacity after ``reserve_rows(total_needed)`` (api.hip): unchanged while the rows fit, else max(needed, 1.5 x
    capacity) rounded up to the 768-row granule."""
    if total_needed <= cap:
        return cap
    want = total_needed
    if cap > 0 and want < cap + cap // 2:
        want = cap + cap // 2
    return -(-want // TILE_ROWS) * TILE_ROWS


def capacity_after_compact(cap: int, live: int, deleted: int) -> int:
    """Row capacity after ``mlvdb_index_compact``: nothing tombstoned is the identity, else the live rows' granule."""
    return cap if deleted == 0 else -(-max(live, 1) // TILE_ROWS) * TILE_ROWS


# ---------------------------------------------------------------- the model
class Refused(RuntimeError):
    """A call the C ABI rejects before it launches anything: MLVDB_ERR_INVALID_ARG."""
    status = 1


class Unsupported(Refused):
    """A call beyond a compiled-in limit, rejected before any launch as well: MLVDB_ERR_UNSUPPORTED."""
    status = 6


class HistoryModel(DistinctOracleEngine, FacetOracleEngine, EachOracleEngine, EachRangeOracleEngine):
    """Every entry point of ``HipScanEngine`` in NumPy, composed from the suite's oracle engines, plus ``reset``, a
    ``define_attr`` that may come after rows and be repeated, and the argument refusals of the C ABI as ``Refused``."""

    def __init__(self, dim: int, space: str) -> None:
        super().__init__(dim, space)
        self._kinds = {}

    def define_attr(self, attr, kind):
        if attr in self._kinds:  # (mlvdb_attr_define: the same type again is accepted and changes nothing)
            if self._kinds[attr] != kind:
                raise RuntimeError("attribute already defined with another type")
            return
        super().define_attr(attr, kind)
        self._kinds[attr] = kind

    def reset(self, space=None):
        """Rows and values go, column definitions stay, the space may change."""
        self._rows = np.zeros((0, self.dim), dtype=np.float32)
        self._deleted = np.zeros(0, dtype=bool)
        self._cols = {a: col[:0].copy() for a, col in self._cols.items()}
        if space is not None:
            self.space = space

    def set_strategy(self, strategy):  # routes: the answers do not depend on them
        pass

    def set_tuning(self, **knobs):
        pass

    def _col(self, attr):
        if attr not in self._cols:
            raise Refused("attribute not defined")
        return self._cols[attr]

    def match(self, program):
        for op, attr, _, _ in program.ops.tolist():
            if op not in (W.AND, W.OR, W.NOT, W.TRUE):
                self._col(attr)
        return super().match(program)

    def get_attr(self, attr, first, n, dtype=np.int64):
        return self._col(attr)[first:first + n].astype(dtype)

    def search(self, queries, k, mask=None, where=None):
        if k < 1:
            raise Refused("k must be >= 1")
        return super().search(queries, k, mask, where)

    def search64(self, queries, k, mask=None, where=None):
        if k < 1:
            raise Refused("k must be >= 1")
        return super().search64(queries, k, mask, where)

    def pair_distances(self, queries, labels):
        if self._rows.shape[0] == 0:
            labels = np.asarray(labels)
            if labels.size and labels.max() >= 0:
                raise RuntimeError("label out of range")
            d64 = np.full(labels.shape, np.inf)
            return d64, d64.astype(np.float32)
        return super().pair_distances(queries, labels)

    def search_distinct(self, queries, k, attr, max_groups=0, where=None, want64=False):
        if self._col(attr).dtype != np.int64:
            raise Refused("distinct needs an int64 column")
        if k < 1:
            raise Refused("k must be >= 1")
        return super().search_distinct(queries, k, attr, max_groups, where, want64)

    def facet_values(self, attr, max_values, where=None):
        if self._col(attr).dtype != np.int64:
            raise Refused("value facets need an int64 column")
        if max_values < 1:
            raise Refused("max_values must be in 1..MLVDB_FACET_MAX_VALUES")
        return super().facet_values(attr, max_values, where)

    def facet_bins(self, attr, edges, where=None):
        edges = np.asarray(edges)
        if edges.size < 1 or edges.dtype != self._col(attr).dtype or not (np.diff(edges) > 0).all():
            raise Refused("edges must be strictly ascending and of the column's type")
        return super().facet_bins(attr, edges, where)


# ---------------------------------------------------------------- ops: plain parameters -> arrays, and the one call they make
def program_of(p) -> W.Program:
    """A ``where.Program`` from its JSON form {"ops": [[op, attr, a, b], ...], "set": [...]}."""
    return W.Program(np.array([tuple(o) for o in p["ops"]], dtype=W.OP_DTYPE), np.array(p["set"], dtype=np.int64))


def column_values(attr: int, n: int, rng, total: int) -> np.ndarray:
    """Values of column ``attr``: 0 = int64 "group" (~total / 20 values, 15 % absent), 1 = float64 "score" (the hostile pool and
    Gaussians), 2 = int64 "tenant" (16 values), 3 = the int64 column defined mid-history (8 values, 10 % absent)."""
    if attr == 0:
        v = rng.integers(0, max(1, total // 20), n).astype(np.int64)
        v[rng.random(n) < 0.15] = ABSENT
        return v
    if attr == 1:
        pool = rng.choice(FLOAT_POOL, n)
        pick = rng.random(n) < 0.3
        v = rng.standard_normal(n)
        v[pick] = pool[pick]
        return v
    if attr == 2:
        return rng.integers(0, 16, n).astype(np.int64)
    v = rng.integers(0, 8, n).astype(np.int64)
    v[rng.random(n) < 0.10] = ABSENT
    return v


def _queries(op, d):
    return np.random.default_rng(op["seed"]).standard_normal((op["nq"], d), dtype=np.float32)


def materialise(model: HistoryModel, op: dict) -> dict:
    """The arrays of an op, from its parameters and the model's state before it."""
    kind, d, a = op["op"], model.dim, {}
    total = model._rows.shape[0]
    if kind == "append":
        rows = np.random.default_rng(op["seed"]).standard_normal((op["n"], d), dtype=np.float32)
        for i, src in op["copies"]:
            rows[i] = model._rows[src]  # bit-copies of stored rows: exact ties, ordered by label
        a["rows"] = rows
    elif kind == "set_attr":
        a["values"] = column_values(op["attr"], op["n"], np.random.default_rng(op["seed"]), total)
    elif kind == "tombstone":
        mode = op["mode"]
        if mode == "labels":
            lab = np.array(op["labels"], dtype=np.int64)
        elif mode == "frac":
            lab = np.flatnonzero(np.random.default_rng(op["seed"]).random(total) < op["frac"])
        elif mode == "group":
            lab = np.flatnonzero(model._cols[0] == op["value"])
        else:  # every live row
            lab = np.flatnonzero(~model._deleted)
        a["labels"] = lab.astype(np.int64)
    elif kind in ("get_rows_at",):
        a["labels"] = np.array(op["labels"], dtype=np.int64)
    if "nq" in op:
        a["qs"] = _queries(op, d)
    if kind == "search_mask":
        a["mask"] = (np.random.default_rng(op["mask_seed"]).random(total) < op["p"]).astype(np.uint8)
    if op.get("program") is not None:
        a["program"] = program_of(op["program"])
    if "programs" in op:
        a["programs"] = [program_of(p) for p in op["programs"]]
        if "of" in op:
            a["of"] = np.array(op["of"], dtype=np.int32)
    if kind == "facet_bins" or (kind == "refuse" and op["which"] == "edges_unsorted"):
        a["edges"] = np.array(op["edges"], dtype=np.float64 if op["float"] else np.int64)
    if kind == "pair_distances":
        rng = np.random.default_rng(op["label_seed"])
        a["labels"] = rng.integers(-1, max(total, 0), (op["nq"], op["m"])) if total else np.full((op["nq"], op["m"]), -1)
        a["labels"] = a["labels"].astype(np.int64)
    if kind in NEW_MUTATIONS + NEW_QUERIES or (kind == "refuse" and op["which"] in WIDE_REFUSALS):
        _materialise_wide(model, op, a)
    return a


def call(e, op: dict, a: dict):
    """The one engine call of an op (``e``: a ``HipScanEngine``, a ``MultiDeviceEngine`` or the model)."""
    kind = op["op"]
    if kind == "append":
        return e.append(a["rows"])
    if kind == "set_attr":
        return e.set_attr(op["attr"], op["first"], a["values"])
    if kind == "define_attr":
        return e.define_attr(op["attr"], op["kind"])
    if kind == "tombstone":
        return e.tombstone(a["labels"])
    if kind == "compact":
        return e.compact()
    if kind == "reset":
        return e.reset(op["space"])
    if kind == "set_strategy":
        return e.set_strategy(op["strategy"])
    if kind == "set_tuning":
        return e.set_tuning(**{op["key"]: op["value"]})
    if kind == "search":
        return e.search(a["qs"], op["k"])
    if kind == "search64":
        return e.search64(a["qs"], op["k"])
    if kind == "search_mask":
        return e.search64(a["qs"], op["k"], a["mask"])
    if kind == "search_where":
        return e.search64(a["qs"], op["k"], where=a["program"])
    if kind == "search_each":
        return e.search_each(a["qs"], op["k"], a["programs"], a["of"], want64=True)
    if kind == "range":
        return e.range(a["qs"], op["radius"], op["capacity"], op["truncate"])
    if kind == "range_where":
        return e.range(a["qs"], op["radius"], op["capacity"], op["truncate"], where=a["program"])
    if kind == "range_each":
        return e.range_each(a["qs"], op["radius"], op["capacity"], a["programs"], a["of"], op["truncate"])
    if kind == "search_distinct":
        return e.search_distinct(a["qs"], op["k"], op["attr"], 0, a.get("program"), want64=True)
    if kind == "facet_values":
        return e.facet_values(op["attr"], op["max_values"], a.get("program"))
    if kind == "facet_bins":
        return e.facet_bins(op["attr"], a["edges"], a.get("program"))
    if kind == "where_count":
        return e.where_count(a["program"])
    if kind == "where_labels":
        return e.where_labels(a["program"])
    if kind == "count_each":
        return e.count_each(a["programs"])
    if kind == "pair_distances":
        return e.pair_distances(a["qs"], a["labels"])
    if kind == "get_rows":
        return e.get_rows(op["first"], op["n"])
    if kind == "get_rows_at":
        return e.get_rows_at(a["labels"])
    if kind == "get_attr":
        return e.get_attr(op["attr"], op["first"], op["n"], np.float64 if op["float"] else np.int64)
    if kind == "counts":
        return e.counts()
    if kind == "refuse":
        return _refusal(e, op, a)
    if kind in _WIDE_CALLS:
        return _WIDE_CALLS[kind](e, op, a)
    if kind in _recent().CALLS:
        return _recent().CALLS[kind](e, op, a)
    raise ValueError(f"unknown op {kind!r}")


def _recent():
    """tests/history_recent_helpers.py: the ops of the third wave (it imports this module: looked up when first needed)."""
    from tests import history_recent_helpers

    return history_recent_helpers


def _status_of(err):
    """The ABI status behind a ``RuntimeError``: the model's ``Refused`` carries it, ``HipScanEngine._check`` writes it as
    "<call> failed (<status>): ..."; None for an error raised in Python."""
    if isinstance(err, Refused):
        return err.status
    m = re.search(r" failed \((\d+)\): ", str(err))
    return int(m.group(1)) if m else None


def _refusal(e, op, a):
    """A call the ABI rejects before any launch, or one that ends in MLVDB_ERR_OVERFLOW -> what came of it, comparable: a
    refusal carries its status, so that a call that was launched and came back with MLVDB_ERR_HIP is no refusal."""
    which = op["which"]
    if which == "range_small":  # capacity below the hit counts, no truncation: the wrapper repeats the call with the size reported
        return e.range(a["qs"], op["radius"], op["capacity"], False)
    try:
        if which == "k0":
            e.search(a["qs"], 0)
        elif which == "distinct_float":
            e.search_distinct(a["qs"], 5, 1)
        elif which == "facet_max0":
            e.facet_values(0, 0)
        elif which == "edges_unsorted":
            e.facet_bins(2, a["edges"])
        elif which == "undefined":
            e.where_count(a["program"])
        elif which == "facet_overflow":
            e.facet_values(op["attr"], op["max_values"])
        else:
            _wide_refusal(e, op, a)
    except FacetOverflow as err:
        return ("overflow", err.matched, err.absent)
    except RuntimeError as err:
        return ("refused", _status_of(err))
    return ("accepted",)


# ---------------------------------------------------------------- comparison of one answer
def _max_err64(got64, want64, tag, stats):
    fin = np.isfinite(want64)
    assert np.array_equal(np.isfinite(got64), fin), f"{tag}: fp64 padding differs"
    if fin.any():
        err = float(np.abs(got64[fin] - want64[fin]).max())
        stats["max_err64"] = max(stats["max_err64"], err)
        assert err <= SCORE_ATOL, f"{tag}: max |d64 - oracle| {err}"


def _same(got, want, tag, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{tag}: {what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    bits = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    if not np.array_equal(np.ascontiguousarray(got).view(bits), np.ascontiguousarray(want).view(bits)):
        bad = np.flatnonzero(np.ascontiguousarray(got).view(bits).ravel() != np.ascontiguousarray(want).view(bits).ravel())
        raise AssertionError(f"{tag}: {what} differ at {bad.size} places, first {bad[:5]}: got {got.ravel()[bad[:5]]} "
                             f"want {want.ravel()[bad[:5]]}")


def compare(e, op, a, got, want, tag, stats):
    kind = op["op"]
    if kind in NEW_MUTATIONS + NEW_QUERIES:
        assert _compare_wide(e, op, a, got, want, tag, stats), f"{tag}: returned {got!r}, the model {want!r}"
    elif kind in ("append", "tombstone"):
        assert got == want, f"{tag}: returned {got}, the model {want}"
    elif kind == "compact":
        _same(got, want, tag, "old_labels")
    elif kind == "search":
        assert_knn_matches(tuple(got[:3]), tuple(want[:3]), tag)
    elif kind in ("search64", "search_mask", "search_where", "search_each"):
        assert_knn_matches(tuple(got[:3]), tuple(want[:3]), tag)
        _max_err64(got[3], want[3], tag, stats)
    elif kind in ("range", "range_where", "range_each") or (kind == "refuse" and op["which"] == "range_small"):
        assert_range_matches(got, want, tag)
    elif kind == "search_distinct":  # the rules of tests/test_gpu_distinct.py: _check
        lab, dist, cnt, d64, grp = got
        wl, _, wc, wd, wg = want
        ok = np.array_equal(lab, wl) and np.array_equal(cnt, wc) and np.array_equal(grp, wg)
        if not ok:
            bad = np.flatnonzero((lab != wl).any(axis=1) | (cnt != wc) | (grp != wg).any(axis=1))
            raise AssertionError(f"{tag}: {bad.size} queries differ, first {bad[0]}: got {lab[bad[0]]} ({cnt[bad[0]]}) "
                                 f"want {wl[bad[0]]} ({wc[bad[0]]})")
        _max_err64(d64, wd, tag, stats)
        assert np.array_equal(np.isfinite(dist), np.isfinite(wd)), f"{tag}: padding differs"
        assert np.array_equal(dist.view(np.int32), d64.astype(np.float32).view(np.int32)), f"{tag}: fp32 is not the rounded fp64"
        p64, p32 = e.pair_distances(a["qs"], lab)
        assert np.array_equal(p64.view(np.int64), d64.view(np.int64)), f"{tag}: fp64 differs from pair_distances"
        assert np.array_equal(p32.view(np.int32), dist.view(np.int32)), f"{tag}: fp32 differs from pair_distances"
    elif kind == "facet_values":
        _same(got[0], want[0], tag, "values")
        _same(got[1], want[1], tag, "counts")
        assert tuple(got[2:]) == tuple(want[2:]), f"{tag}: matched / absent {got[2:]}, the model {want[2:]}"
    elif kind == "facet_bins":
        _same(got[0], want[0], tag, "bin counts")
        assert tuple(got[1:]) == tuple(want[1:]), f"{tag}: matched / absent {got[1:]}, the model {want[1:]}"
    elif kind == "where_count":
        assert got == want, f"{tag}: {got} rows, the model {want}"
    elif kind in ("where_labels", "count_each"):
        _same(got, want, tag, "labels" if kind == "where_labels" else "counts")
    elif kind == "pair_distances":
        _max_err64(got[0], want[0], tag, stats)
        assert np.array_equal(got[1].view(np.int32), got[0].astype(np.float32).view(np.int32)), f"{tag}: fp32 is not the rounded fp64"
    elif kind in ("get_rows", "get_rows_at"):
        _same(got, want, tag, "rows")
    elif kind == "get_attr":
        _same(got, want, tag, "values")
    elif kind == "counts":
        assert tuple(got) == tuple(want), f"{tag}: counts {got}, the model {want}"
    elif kind == "refuse":
        assert tuple(got) == tuple(want), f"{tag}: {got}, the model {want}"
    elif kind in _recent().CALLS:
        _recent().compare(e, op, a, got, want, tag, stats)
    else:
        assert got is None and want is None, f"{tag}: returned {got!r}"


def _evidence(x, prefix, out):
    if hasattr(x, "present"):  # a ListColumn / SparseColumn
        for name, y in vars(x).items():
            _evidence(y, f"{prefix}_{name}", out)
    elif isinstance(x, (tuple, list)) or hasattr(x, "offsets"):
        for i, y in enumerate(x):
            _evidence(y, f"{prefix}_{i}", out)
    elif x is not None:
        try:
            out[prefix] = np.asarray(x)
        except Exception:
            pass


def run_history(engine, ops, expected, tag):
    """Apply ``ops`` to ``engine`` one by one and compare each answer with ``expected`` at once.  On the first mismatch: the ops up
    to that step go to history_<tag>.json in the mismatch directory of tests/conftest.py (the arrays to mismatch_history_<tag>.npz), then an AssertionError names
    the history (its tag carries the seed), the step and the op.  Nothing is retried and nothing more is started on the engine;
    the caller closes it.  Returns {"steps", "max_err64"}."""
    stats = {"steps": 0, "max_err64": 0.0}
    for step, (op, exp) in enumerate(zip(ops, expected)):
        got = None
        try:
            got = call(engine, op, exp["args"])
            compare(engine, op, exp["args"], got, exp["want"], f"{tag}/step{step}/{op['op']}", stats)
            if op["op"] in WIDE_MUTATIONS:
                counts = tuple(engine.counts())
                assert counts == tuple(exp["counts"]), f"counts {counts} after the op, the model {exp['counts']}"
        except Exception as err:
            from tests import conftest

            path, dumped = conftest.OUT_DIR / f"history_{tag}.json", ""
            try:
                conftest.OUT_DIR.mkdir(exist_ok=True)
                path.write_text(json.dumps({"tag": tag, "failed_step": step, "ops": ops[:step + 1]}))
            except Exception as why:  # the mismatch is what matters; say that its record is missing
                dumped = f" (the ops could NOT be written to {path.name}: {type(why).__name__}: {why})"
            arrays = {}
            _evidence(got, "got", arrays)
            _evidence(exp["want"], "want", arrays)
            conftest.dump_mismatch(f"history_{tag}", **arrays)
            short = {k: (v if not isinstance(v, list) or len(v) <= 8 else f"[{len(v)} entries]") for k, v in op.items()}
            raise AssertionError(f"history {tag}: step {step}, op {short}: {type(err).__name__}: {err}{dumped}") from err
        stats["steps"] = step + 1
    print(f"history {tag}: {stats['steps']} steps, max |d64 - oracle| = {stats['max_err64']:.3e}")
    return stats


# ---------------------------------------------------------------- generation
def _leaf(op, attr, a=0, b=0):
    return [int(op), int(attr), int(a), int(b)]


def _gaps_ok(s: np.ndarray) -> bool:
    """No two consecutive *different* distances of the ascending ``s`` within TIE_REL max(1, |d|) of each other."""
    gaps = np.diff(s)
    return not ((gaps > 0) & (gaps <= TIE_REL * np.maximum(1.0, np.abs(s[1:])))).any()


class _Generator:
    def __init__(self, seed, space, d, scale):
        assert space in SPACES and scale in SCALES + WIDE_SCALES
        self.seed, self.d, self.scale = seed, d, scale
        self.rng = np.random.default_rng([seed, d, SPACES.index(space), (SCALES + WIDE_SCALES).index(scale)])
        self.model = (WideHistoryModel if scale in WIDE_SCALES else HistoryModel)(d, space)
        self.ops, self.expected = [], []
        self.capacity = 0
        self.drawn = self.redraws = 0
        self.last_first = 0
        self.defined3 = False

    # -- plumbing
    def _seed(self):
        return int(self.rng.integers(1 << 31))

    def emit(self, op):
        args = materialise(self.model, op)
        want = call(self.model, op, args)
        exp = {"args": args, "want": want}
        if op["op"] in WIDE_MUTATIONS:
            exp["counts"] = self.model.counts()
        if self.scale in WIDE_SCALES:  # (used, capacity, live values) of every pooled attribute after the op
            exp["pools"] = self.model.pools()
        self.ops.append(op)
        self.expected.append(exp)
        return want

    @property
    def total(self):
        return self.model._rows.shape[0]

    @property
    def live(self):
        return np.flatnonzero(~self.model._deleted)

    def attrs(self):
        return sorted(self.model._cols)

    # -- mutations
    def append(self, mode=None, n=None):
        mode = mode or ("one", "sixteen", "hundreds", "cross")[self.rng.integers(4)]
        if n is None:
            n = {"one": 1, "sixteen": int(self.rng.integers(15, 18)), "hundreds": int(self.rng.integers(200, 500)),
                 "cross": self.capacity - self.total + int(self.rng.integers(1, 40)) if self.capacity else 300}[mode]
        if self.scale not in ("large", "wide_large") and self.total + n > MAX_ROWS_SMALL:  # keep the corpus small: drop most rows first
            self.emit({"op": "tombstone", "mode": "frac", "seed": self._seed(), "frac": 0.7})
            self.compact()
            if mode == "cross":
                n = self.capacity - self.total + int(self.rng.integers(1, 40))
        copies = []
        if self.total and self.rng.random() < 0.6:
            copies = [[int(self.rng.integers(n)), int(self.rng.integers(self.total))] for _ in range(min(n, 3))]
        self.last_first = self.total
        self.capacity = capacity_after(self.capacity, self.total + n)
        self.emit({"op": "append", "n": int(n), "seed": self._seed(), "copies": copies})

    def set_attr(self, attr=None, first=None):
        if not self.attrs():
            return self.define()
        attr = int(self.rng.choice(self.attrs())) if attr is None else attr
        if first is None:  # a span that reaches back over older (some tombstoned) rows and covers the freshly appended ones
            first = max(0, self.last_first - int(self.rng.integers(0, 60))) if self.rng.random() < 0.7 else \
                int(self.rng.integers(0, self.total + 1))
        first = min(first, self.total)
        self.emit({"op": "set_attr", "attr": attr, "first": int(first), "n": int(self.total - first), "seed": self._seed()})

    def set_attrs(self):
        first = max(0, self.last_first - int(self.rng.integers(0, 60)))
        for attr in self.attrs():
            self.set_attr(attr, first)

    def define(self):
        if self.scale != "multi" and not self.defined3 and self.total:
            self.defined3 = True
            return self.emit({"op": "define_attr", "attr": 3, "kind": "int64"})
        attr = int(self.rng.integers(3))  # the same definition again: accepted, changes nothing
        self.emit({"op": "define_attr", "attr": attr, "kind": ("int64", "float64", "int64")[attr]})

    def tombstone(self, mode=None):
        mode = mode or ("few", "frac", "group", "again", "few", "frac")[self.rng.integers(6)]
        dead = np.flatnonzero(self.model._deleted)
        if self.total == 0:
            return self.emit({"op": "tombstone", "mode": "labels", "labels": []})
        if mode == "again" and dead.size:
            return self.emit({"op": "tombstone", "mode": "labels", "labels": self.rng.choice(dead, 4).tolist()})
        if mode == "group" and 0 in self.model._cols and self.live.size:
            value = int(self.model._cols[0][self.rng.choice(self.live)])
            if value != ABSENT:
                return self.emit({"op": "tombstone", "mode": "group", "value": value})
        if mode == "frac":
            return self.emit({"op": "tombstone", "mode": "frac", "seed": self._seed(), "frac": 0.3})
        if mode == "all":
            return self.emit({"op": "tombstone", "mode": "all"})
        self.emit({"op": "tombstone", "mode": "labels", "labels": self.rng.integers(0, self.total, 5).tolist()})

    def compact(self):
        total, deleted = self.model.counts()
        self.capacity = capacity_after_compact(self.capacity, total - deleted, deleted)
        self.emit({"op": "compact"})
        self.last_first = min(self.last_first, self.total)

    def reset(self, other=None):
        other = self.rng.random() < 0.5 if other is None else other
        space = SPACES[(SPACES.index(self.model.space) + 1 + int(self.rng.integers(2))) % 3] if other else None
        self.emit({"op": "reset", "space": space})
        self.last_first = 0

    def strategy(self, s=None):
        self.emit({"op": "set_strategy", "strategy": s or ("auto", "exact", "filter")[self.rng.integers(3)]})

    def tuning(self, key=None, value=None):
        if key is None:
            key = ("WHERE_GATHER", "DISTINCT_OVERSAMPLE")[self.rng.integers(2)]
            value = int(self.rng.choice(WHERE_GATHER_VALUES if key == "WHERE_GATHER" else (0, 4)))
        self.emit({"op": "set_tuning", "key": key, "value": int(value)})

    def mutate(self, kind):
        {"append": self.append, "set_attr": self.set_attr, "define_attr": self.define, "tombstone": self.tombstone,
         "compact": self.compact, "reset": self.reset, "set_strategy": self.strategy, "set_tuning": self.tuning}[kind]()

    def ensure_rows(self, least=150):
        if self.live.size < least:
            self.append("hundreds")
            self.set_attrs()

    # -- programs (JSON form)
    def program(self, which=None):
        which = which or ("nothing", "few", "half", "groups", "score", "no_group", "attr3")[self.rng.integers(7)]
        if which == "attr3" and not self.defined3:
            which = "few"
        if which == "nothing":
            ops, table = [_leaf(W.EQ, 2, 999)], []
        elif which == "few":
            ops, table = [_leaf(W.EQ, 2, self.rng.integers(16))], []
        elif which == "half":
            ops, table = [_leaf(W.LT, 2, 8)], []
        elif which == "groups":
            table = sorted(int(v) for v in self.rng.integers(0, max(1, self.total // 20), 3))
            ops = [_leaf(W.IN, 0, 0, 3)]
        elif which == "score":
            ops, table = [_leaf(W.GT, 1, W.float_bits(0.0)), _leaf(W.GE, 2, 4), _leaf(W.AND, 0)], []
        elif which == "no_group":
            ops, table = [_leaf(W.EXISTS, 0), _leaf(W.NOT, 0)], []
        else:
            ops, table = [_leaf(W.EQ, 3, self.rng.integers(8))], []
        return {"ops": ops, "set": table}

    def each(self, nq, which=None):
        """Programs that match nothing, a few rows and half the rows, plus unfiltered queries, in one call."""
        programs = [self.program(w) for w in (which or ("nothing", "few", "half", "score"))]
        of = [-1 if i % 4 == 3 else i % len(programs) for i in range(nq)]
        return programs, of

    # -- queries, redrawn while a near-tie could make the order ambiguous
    def _dist(self, qs):
        return exact_scan.exact_distances(qs, self.model._rows, self.model.space)

    def _allowed(self, op, nq):
        """bool [nq, n]: the rows each query of the op may return."""
        m = self.model
        if op["op"] == "search_mask":
            mask = materialise(m, op)["mask"] != 0
            return np.broadcast_to(mask & ~m._deleted, (nq, self.total))
        if op.get("program") is not None:
            return np.broadcast_to(m.match(program_of(op["program"])), (nq, self.total))
        if "of" in op:
            each = [m.match(program_of(p)) for p in op["programs"]]
            return np.stack([~m._deleted if j < 0 else each[j] for j in op["of"]])
        return np.broadcast_to(~m._deleted, (nq, self.total))

    def _knn_ok(self, op):
        if self.total < 2:
            return True
        dist = self._dist(_queries(op, self.d))
        allowed = self._allowed(op, op["nq"])
        if op["op"] == "search_distinct":
            groups = self.model._cols[op["attr"]]
            for i in range(op["nq"]):
                idx = np.flatnonzero(allowed[i] & (groups != ABSENT))
                order = idx[np.lexsort((idx, dist[i, idx]))]
                first = np.sort(np.unique(groups[order], return_index=True)[1])
                cut = int(first[op["k"]]) + 1 if first.size > op["k"] else order.size
                if not _gaps_ok(dist[i, order[:cut]]):
                    return False
            return True
        return all(_gaps_ok(np.sort(dist[i, allowed[i]])[:op["k"] + 1]) for i in range(op["nq"]))

    def knn(self, kind, nq=None, k=None, **extra):
        nq = int(nq or (1, 3, 9, 12, 40)[self.rng.integers(5)])
        k = int(k or (1, 10, 64, 100)[self.rng.integers(4)])
        if kind == "search_distinct":
            k = min(k, 64)
        while True:
            self.drawn += 1
            op = {"op": kind, "nq": nq, "k": k, "seed": self._seed(), **extra}
            if kind == "search_mask":
                op.update(mask_seed=self._seed(), p=float(self.rng.choice([0.05, 0.5, 0.9])))
            if self._knn_ok(op):
                return self.emit(op)
            self.redraws += 1

    def ranged(self, kind, nq=None, capacity=64, truncate=None, **extra):
        nq = int(nq or (1, 3, 9)[self.rng.integers(3)])
        truncate = bool(self.rng.random() < 0.3) if truncate is None else truncate
        while True:
            self.drawn += 1
            op = {"op": kind, "nq": nq, "seed": self._seed(), "capacity": capacity, "truncate": truncate, **extra}
            radius = np.float32(1.0)
            ok = True
            if self.total:
                dist = self._dist(_queries(op, self.d))
                allowed = self._allowed(op, nq)
                j = int(self.rng.integers(nq))
                s = np.sort(dist[j, allowed[j]])
                if s.size:  # the float32 midpoint between two consecutive distances of one query of the call
                    m = min(int(self.rng.choice([0, 3, 40, 300])), s.size - 1)
                    radius = np.float32((s[m - 1] + s[m]) / 2) if m else np.nextafter(np.float32(s[0]), np.float32(-np.inf))
                r = float(radius)
                ok = not (np.abs(dist[:, ~self.model._deleted] - r) <= TIE_REL * max(1.0, abs(r))).any()
            if ok:
                op["radius"] = float(radius)
                return self.emit(op)
            self.redraws += 1

    def query(self, kind, **kw):
        rng, total = self.rng, self.total
        if kind in ("search", "search64", "search_mask"):
            return self.knn(kind, **kw)
        if kind == "search_where":
            return self.knn(kind, program=kw.pop("program", None) or self.program(), **kw)
        if kind == "search_each":
            nq = kw.pop("nq", (3, 9, 12)[rng.integers(3)])
            programs, of = self.each(nq, kw.pop("which", None))
            return self.knn(kind, nq=nq, k=kw.pop("k", (1, 10, 64, 100)[rng.integers(4)]), programs=programs, of=of)
        if kind == "range":
            return self.ranged(kind, **kw)
        if kind == "range_where":
            return self.ranged(kind, program=self.program(), **kw)
        if kind == "range_each":
            nq = (3, 9)[rng.integers(2)]
            programs, of = self.each(nq)
            return self.ranged(kind, nq=nq, programs=programs, of=of)
        if kind == "search_distinct":
            attr = kw.pop("attr", 0)
            program = self.program(("half", "score", "no_group")[rng.integers(3)]) if rng.random() < 0.5 else None
            return self.knn(kind, nq=(1, 9, 12)[rng.integers(3)], attr=attr, program=kw.pop("program", program), **kw)
        if kind == "facet_values":
            program = self.program() if rng.random() < 0.5 else None
            return self.emit({"op": kind, "attr": kw.get("attr", (0, 2)[rng.integers(2)]), "max_values": 4096, "program": program})
        if kind == "facet_bins":
            program = self.program() if rng.random() < 0.5 else None
            if rng.random() < 0.5:
                return self.emit({"op": kind, "attr": 1, "float": True, "edges": [-1.0, 0.0, 0.5, 1.5], "program": program})
            return self.emit({"op": kind, "attr": (0, 2)[rng.integers(2)], "float": False, "edges": [0, 2, 8, 50], "program": program})
        if kind in ("where_count", "where_labels"):
            return self.emit({"op": kind, "program": kw.get("program") or self.program()})
        if kind == "count_each":
            return self.emit({"op": kind, "programs": [self.program() for _ in range(5)]})
        if kind == "pair_distances":
            return self.emit({"op": kind, "nq": 3, "seed": self._seed(), "m": 7, "label_seed": self._seed()})
        if kind == "get_rows":
            first = int(rng.integers(0, total + 1))
            return self.emit({"op": kind, "first": first, "n": int(min(total - first, rng.integers(0, 40)))})
        if kind == "get_rows_at":
            return self.emit({"op": kind, "labels": rng.integers(0, total, 6).tolist() if total else []})
        if kind == "get_attr":
            attr = int(rng.choice(self.attrs()))
            first = int(rng.integers(0, total + 1))
            return self.emit({"op": kind, "attr": attr, "float": attr == 1, "first": first,
                              "n": int(min(total - first, rng.integers(0, 300)))})
        if kind == "counts":
            return self.emit({"op": kind})
        raise ValueError(kind)

    def refuse(self, which):
        if which == "range_small":
            return self.ranged("refuse", which=which, capacity=2, truncate=False)
        op = {"op": "refuse", "which": which}
        if which in ("k0", "distinct_float"):
            op.update(nq=3, seed=self._seed())
        elif which == "edges_unsorted":
            op.update(edges=[5, 3], float=False)
        elif which == "undefined":
            op["program"] = {"ops": [_leaf(W.EQ, 9, 1)], "set": []}
        elif which == "facet_overflow":
            op.update(attr=2, max_values=2)
        return self.emit(op)

    # -- the schedule
    def small(self):
        rng, seed = self.rng, self.seed
        for attr, kind in ((0, "int64"), (1, "float64"), (2, "int64")):  # defined before the first append
            self.emit({"op": "define_attr", "attr": attr, "kind": kind})
        self.append("hundreds")
        self.set_attrs()
        items = [lambda m=m, q=q: (self.ensure_rows(), self.mutate(m), self.query(q)) for m, q in PAIRS[seed % PAIR_SLICES::PAIR_SLICES]]

        def regrowth():  # (a)
            self.ensure_rows()
            for _ in range(2):
                self.append("cross")
                self.set_attrs()
            self.query("facet_values")
            self.query("search_where")

        def filter_route(x):  # (b)
            self.ensure_rows()
            self.strategy("filter")
            self.query("search", nq=12)
            {"append": self.append, "tombstone": self.tombstone, "compact": self.compact,
             "reset": lambda: self.reset(False), "reset_other": lambda: self.reset(True)}[x]()
            self.query("search64", nq=12)
            self.strategy("auto")

        def masks():  # (c)
            self.ensure_rows()
            for kind, kw in (("search_mask", {}), ("search_where", {"program": self.program("half")}),
                             ("search_each", {"which": ("half", "few")})):
                self.query(kind, **kw)
                self.query("search64")
            self.query("search_mask")
            self.tombstone("few")
            self.query("search")

        def ranges():  # (d)
            self.ensure_rows()
            self.tombstone("few")
            if rng.random() < 0.5:
                self.query("range")
            else:
                self.query("search", k=100)
            self.append("sixteen")
            self.query("range")
            self.compact()
            self.query("range")

        def refusals():  # (e)
            self.ensure_rows()
            for i, which in enumerate(REFUSALS):
                if i % 2 == seed % 2:
                    self.refuse(which)
                    self.query(("search64", "facet_values", "where_count", "search_distinct")[rng.integers(4)])

        def empty(how):  # (f)
            self.ensure_rows()
            if how == "compact":
                self.tombstone("all")
                self.compact()
            else:
                self.reset(False)
            for _ in range(2):
                for kind in ("search64", "range", "where_count", "facet_values", "search_distinct"):
                    self.query(kind)
                if self.total == 0:
                    self.append("hundreds")

        def l2_offsets():  # (h)
            if self.model.space != "l2":
                self.emit({"op": "reset", "space": "l2"})
            self.ensure_rows()
            self.strategy("filter")
            self.query("search", nq=12, k=10)
            self.query("search", nq=40, k=10)
            self.tombstone("few")
            self.query("search", nq=12, k=10)
            self.strategy("auto")

        def late_column():  # (i)
            self.ensure_rows()
            self.define()
            self.set_attr(3, 0)
            self.query("facet_values", attr=3)
            self.query("search_distinct", attr=3)
            self.query("where_count", program=self.program("attr3"))

        def knobs():  # (j)
            self.ensure_rows()
            for value in (0, 4):
                self.tuning("DISTINCT_OVERSAMPLE", value)
                self.query("search_distinct")
            for value in WHERE_GATHER_VALUES[::-1]:
                self.tuning("WHERE_GATHER", value)
                self.query("search_each")

        xs = ("append", "tombstone", "compact", "reset", "reset_other")
        items += [regrowth, late_column, refusals, lambda: filter_route(xs[seed % 5]), lambda: filter_route(xs[(seed + 2) % 5]),
                  masks if seed % 2 == 0 else ranges, lambda: empty("compact" if seed % 2 == 0 else "reset")]
        if seed % 3 != 2:
            items.append(knobs)
        if self.model.space == "l2":
            items.append(l2_offsets)
        items += [lambda: (self.ensure_rows(), self.query(QUERIES[rng.integers(len(QUERIES))])) for _ in range(4)]
        for i in rng.permutation(len(items)):
            items[i]()

    def large(self):
        """Appends of 12,000 rows until past 32,768 live rows (`auto` changes route at nq = 12 and 40), tombstones, a compaction
        back below the threshold, growth again; few query steps, for the fp64 oracle's sake."""
        for attr, kind in ((0, "int64"), (1, "float64"), (2, "int64")):
            self.emit({"op": "define_attr", "attr": attr, "kind": kind})
        self.append(n=12000)
        self.set_attrs()
        self.query("search", nq=12, k=10)  # below the threshold: the exact scan
        for _ in range(2):
            self.append(n=12000)
            self.set_attrs()
        self.query("search", nq=12, k=10)
        self.query("search64", nq=40, k=10)
        self.query("search", nq=3, k=10)
        self.query("range", nq=3)
        self.query("search_mask", nq=12, k=10)
        self.query("search", nq=12, k=64)
        self.emit({"op": "tombstone", "mode": "frac", "seed": self._seed(), "frac": 0.35})
        self.query("search64", nq=12, k=10)
        self.compact()
        assert self.total < FILTER_MIN_ROWS
        self.query("search", nq=12, k=10)
        self.query("search_where", nq=12, k=10, program=self.program("half"))
        self.append(n=12000)
        assert self.total > FILTER_MIN_ROWS
        self.set_attrs()
        self.query("search64", nq=40, k=64)
        self.query("search", nq=12, k=100)
        self.query("search_distinct", k=10)
        self.query("search_each", nq=12, k=10)
        self.query("facet_values")
        self.query("range_each")

    def multi(self):
        """The ops ``MultiDeviceEngine`` implements (those of tests/test_host_fuzz.py, and its range, pair and row reads), in a
        random order."""
        rng = self.rng
        self.append("hundreds")
        for _ in range(40):
            r = rng.random()
            if self.total == 0 or r < 0.25:
                self.append(("one", "sixteen", "hundreds")[rng.integers(3)])
            elif r < 0.40:
                self.tombstone(("few", "frac", "again")[rng.integers(3)])
            elif r < 0.50:
                self.compact()
            else:
                self.query(MULTI_QUERIES[rng.integers(len(MULTI_QUERIES))])


# ================================================================ the wide histories: the nine newer entry families
NEW_MUTATIONS = ("set_attr_at", "update_where", "tombstone_where", "set_attr_list", "set_attr_list_at", "update_where_list",
                 "set_attr_sparse", "set_attr_sparse_at")
NEW_QUERIES = ("where_ordered", "search_mmr", "search_grouped", "search_like", "search_maxsim", "get_attr_list", "list_stats",
               "facet_list_values", "get_attr_sparse", "search_batch_sparse")
WIDE_MUTATIONS = MUTATIONS + NEW_MUTATIONS
WIDE_QUERIES = QUERIES + NEW_QUERIES
WIDE_PAIRS = [(m, q) for m in WIDE_MUTATIONS for q in WIDE_QUERIES if m in NEW_MUTATIONS or q in NEW_QUERIES]
WIDE_PAIR_SLICES = 12  # wide history `seed` carries WIDE_PAIRS[seed % 12::12]
WIDE_REFUSALS = ("mmr_fetch", "grouped_g0", "grouped_g65", "like_label", "maxsim_t0", "maxsim_t129", "ordered_window",
                 "set_at_repeat", "set_attr_on_list", "set_list_on_sparse", "sparse_on_list")
INNER_SEARCHES = ("search_mmr", "search_like", "search_grouped", "search_distinct")  # they run the plain search inside
MASKABLE = ("search_mmr", "search_like", "search_grouped", "search_maxsim", "search_batch_sparse")
LIST_READERS = ("get_attr_list", "facet_list_values", "get_attr_sparse", "search_batch_sparse", "list_stats")
LIST_A, SPARSE_A, LATE_LIST, LATE_SPARSE = 4, 5, 6, 7
POOLED = {LIST_A: "int64_list", SPARSE_A: "sparse", LATE_LIST: "int64_list", LATE_SPARSE: "sparse"}
TAG_VALUES = 8
SPARSE_VOCAB = 64
ORDER_MAX_ROWS = order_helpers.MAX_ROWS
INT64_MAX = 2 ** 63 - 1
LIKE_COSINE_GAP = 2.0 ** -21
# The device builds a cosine like-query q' that may differ from the helper's q by one float32 spacing per component:
# |q'_c - q_c| <= 2^-23 |q_c|, so |q' - q| <= 2^-23 |q|.  The cosine distance reads the direction u = q / |q| alone, and
# u' - u = (dq - u (u . dq)) / |q| to first order: a projection of dq, so |u' - u| <= 2^-23.  A distance 1 - u . x / |x| then
# moves by at most |u' - u| <= 2^-23 and the gap between two of them by at most 2^-22; 2^-21 leaves a factor of two for the
# second-order terms.  A like-query on a cosine index is kept only if its gaps exceed this PLUS the plain TIE_REL rule.


def pool_capacity_after(cap: int, used_after: int) -> int:
    """Capacity of a list / sparse pool after ``list_pool_reserve`` made room for ``used_after`` values (api.hip): unchanged
    while they fit, else max(needed, 2 x capacity, 1024)."""
    return cap if used_after <= cap else max(used_after, 2 * cap, 1024)


class WideHistoryModel(HistoryModel, SparseOracleEngine, order_helpers.OrderOracleEngine, GroupedOracleEngine, MmrOracleEngine,
                       LikeOracleEngine, MaxSimOracleEngine):
    """``HistoryModel`` + the entries added since (ordered queries, diversified / grouped / by-example / late-interaction
    kNN, updates and filtered deletes, list and sparse columns), composed from their oracle engines, plus a ``reset`` that
    empties the lists, the capacity of every pool mirrored, and the refusals the C ABI makes before any launch."""

    def __init__(self, dim, space):
        super().__init__(dim, space)
        self._pool_cap = {}

    # -- definitions, reset, pools
    def define_attr(self, attr, kind):
        super().define_attr(attr, kind)
        if attr in self._lists:
            self._pool_cap.setdefault(attr, 0)

    def reset(self, space=None):
        super().reset(space)
        self.reset_lists()  # used = 0, the allocation (the capacity) stays

    def compact(self):
        old = super().compact()
        for a in self._lists:  # the repack: a pool of exactly the live values
            self._pool_cap[a] = self._pool_used[a]
        return old

    def pools(self):
        return {a: (self._pool_used[a], self._pool_cap[a], self.list_stats(a)[1]) for a in sorted(self._lists)}

    def _grown(self, attr):
        self._pool_cap[attr] = pool_capacity_after(self._pool_cap[attr], self._pool_used[attr])

    def _list_col(self, attr, sparse, what):
        if attr not in self._lists or (attr in self._sparse) != sparse:
            raise Refused(f"{what}: attribute {attr} is no {'sparse' if sparse else 'list'} column")

    def _labels_ok(self, labels, what):
        labels = np.asarray(labels, dtype=np.int64).ravel()
        if labels.size and (labels.min() < 0 or labels.max() >= self._rows.shape[0] or np.unique(labels).size != labels.size):
            raise Refused(f"{what}: labels must be distinct and in [0, total)")

    def set_attr(self, attr, first, values):
        self._col(attr)
        if attr in self._lists:
            raise Refused("attr_set: a list or sparse column")
        return super().set_attr(attr, first, values)

    def set_attr_at(self, attr, labels, values):
        if attr in self._lists:
            raise Refused("attr_set_at: a list or sparse column")
        self._labels_ok(labels, "attr_set_at")
        return super().set_attr_at(attr, labels, values)

    def update_where(self, program, assigns):
        if any(attr in self._lists for attr, _, _ in assigns):
            raise Refused("attr_update_where: a list or sparse column")
        return super().update_where(program, assigns)

    def set_attr_list(self, attr, first, col):
        self._list_col(attr, False, "attr_list_set")
        super().set_attr_list(attr, first, col)
        self._grown(attr)

    def set_attr_list_at(self, attr, labels, col):
        self._list_col(attr, False, "attr_list_set_at")
        self._labels_ok(labels, "attr_list_set_at")
        n = super().set_attr_list_at(attr, labels, col)
        self._grown(attr)
        return n

    def update_where_list(self, program, attr, values):
        self._list_col(attr, False, "attr_list_update_where")
        n = super().update_where_list(program, attr, values)
        self._grown(attr)
        return n

    def get_attr_list(self, attr, first, n):
        self._list_col(attr, False, "attr_list_get")
        return super().get_attr_list(attr, first, n)

    def facet_list_values(self, attr, max_values, where=None):
        self._list_col(attr, False, "facet_list_values")
        if max_values < 1:
            raise Refused("max_values must be in 1..MLVDB_FACET_MAX_VALUES")
        return super().facet_list_values(attr, max_values, where)

    def set_attr_sparse(self, attr, first, col):
        self._list_col(attr, True, "sparse_set")
        super().set_attr_sparse(attr, first, col)
        self._grown(attr)

    def set_attr_sparse_at(self, attr, labels, col):
        self._list_col(attr, True, "sparse_set_at")
        self._labels_ok(labels, "sparse_set_at")
        n = super().set_attr_sparse_at(attr, labels, col)
        self._grown(attr)
        return n

    def get_attr_sparse(self, attr, first, n):
        self._list_col(attr, True, "sparse_get")
        return super().get_attr_sparse(attr, first, n)

    def search_batch_sparse(self, attr, queries, k, where=None):
        self._list_col(attr, True, "search_batch_sparse")
        if k < 1:
            raise Refused("k must be >= 1")
        return super().search_batch_sparse(attr, queries, k, where)

    # -- the scalar-column queries: their limits
    def _group_col(self, attr, what):
        if attr in self._lists or self._col(attr).dtype != np.int64:
            raise Refused(f"{what} needs an int64 column")

    def where_ordered(self, attr, limit, where=None, descending=False, offset=0):
        if attr in self._lists:
            raise Refused("where_ordered: a list or sparse column")
        self._col(attr)
        if offset < 0 or limit < 1 or offset + limit > ORDER_MAX_ROWS:
            raise Refused("where_ordered: 0 <= offset, 1 <= limit, offset + limit <= MLVDB_ORDER_MAX_ROWS")
        return super().where_ordered(attr, limit, where, descending, offset)

    def search_mmr(self, queries, k, fetch_k, lam, where=None, want64=False):
        if not 1 <= k <= fetch_k or not 0.0 <= lam <= 1.0:
            raise Refused("search_mmr: 1 <= k <= fetch_k, 0 <= lambda <= 1")
        return super().search_mmr(queries, k, fetch_k, lam, where, want64)

    def search_grouped(self, queries, k, group_size, attr, max_groups=0, where=None, want64=False):
        self._group_col(attr, "grouped")
        if k < 1 or group_size < 1:
            raise Refused("search_grouped: k >= 1, group_size >= 1")
        if group_size > MAX_GROUP_SIZE:
            raise Unsupported("search_grouped: group_size above MLVDB_GROUPED_MAX_SIZE")
        return super().search_grouped(queries, k, group_size, attr, max_groups, where, want64)

    def search_like(self, labels, weights, offsets, k, *, base=None, exclude=True, where=None, want64=False, want_queries=False):
        labels = np.asarray(labels, np.int64)
        if k < 1 or (labels.size and (labels.min() < 0 or labels.max() >= self._rows.shape[0])):
            raise Refused("search_like: k >= 1 and every example label in [0, total)")
        if base is None and (np.diff(np.asarray(offsets, np.int64)) < 1).any():
            raise Refused("search_like: a query with no example and no base row")
        return super().search_like(labels, weights, offsets, k, base=base, exclude=exclude, where=where, want64=want64,
                                   want_queries=want_queries)

    def search_maxsim(self, tokens, offsets, k, attr, where=None, want_matches=False):
        self._group_col(attr, "maxsim")
        lengths = np.diff(np.asarray(offsets, np.int64))
        if k < 1 or (lengths < 1).any() or (lengths > MAX_TOKENS).any():
            raise Refused("search_maxsim: k >= 1 and 1..MLVDB_MAXSIM_MAX_TOKENS tokens per query")
        return super().search_maxsim(tokens, offsets, k, attr, where, want_matches)


# ---------------------------------------------------------------- wide ops: arrays
def wide_lists(rng, n):
    """n rows of the tag column: 10 % without a list, a few long lists (16 / 17 / 64 values of 100..199), the rest 0 to 5 draws
    (repeats happen) of TAG_VALUES tags."""
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.10:
            out.append(None)
        elif r < 0.13:
            out.append(rng.choice(np.arange(100, 200), int(rng.choice((16, 17, 64))), replace=False).tolist())
        else:
            out.append(rng.integers(0, TAG_VALUES, int(rng.integers(0, 6))).tolist())
    return out


def _labels_of(op, rng, total):
    if "labels" in op:
        return np.array(op["labels"], dtype=np.int64)
    lo = min(op.get("lo", 0), total)
    return rng.choice(np.arange(lo, total), min(op["n"], total - lo), replace=False).astype(np.int64)


def _sparse_queries(rng, n):
    lengths = (0, 1, 5, 20, SPARSE_VOCAB)
    return sparse_csr([random_vector(rng, lengths[int(rng.integers(len(lengths)))], SPARSE_VOCAB, True) for _ in range(n)])


def _materialise_wide(model, op, a):
    kind, d = op["op"], model.dim
    total = model._rows.shape[0]
    rng = np.random.default_rng(op["seed"]) if "seed" in op else None
    if kind == "refuse":
        which = op["which"]
        if which == "like_label":
            a.update(labels=np.array([op["label"]], np.int64), weights=np.ones(1), offsets=np.array([0, 1], np.int64))
        elif which in ("maxsim_t0", "maxsim_t129"):
            lengths = [2, 0, 1] if which == "maxsim_t0" else [MAX_TOKENS + 1]
            a.update(tokens=rng.standard_normal((sum(lengths), d), dtype=np.float32), offsets=offsets_of(lengths))
        elif which in ("set_attr_on_list", "set_at_repeat"):
            a["values"] = np.array([1, 2], np.int64)
        elif which == "set_list_on_sparse":
            a["col"] = csr([[1, 2]])
        elif which == "sparse_on_list":
            a["sq"] = _sparse_queries(rng, 2)
    elif kind == "set_attr_at":
        a["labels"] = _labels_of(op, rng, total)
        a["values"] = (np.array(op["values"], dtype=np.float64 if op["attr"] == 1 else np.int64) if "values" in op
                       else column_values(op["attr"], a["labels"].size, rng, total))
    elif kind == "set_attr_list":
        a["col"] = csr(wide_lists(rng, op["n"]))
    elif kind == "set_attr_list_at":
        a["labels"] = _labels_of(op, rng, total)
        a["col"] = csr(wide_lists(rng, a["labels"].size))
    elif kind == "set_attr_sparse":
        a["col"] = sparse_csr(random_corpus(rng, op["n"], SPARSE_VOCAB, True))
    elif kind == "set_attr_sparse_at":
        a["labels"] = _labels_of(op, rng, total)
        a["col"] = sparse_csr(random_corpus(rng, a["labels"].size, SPARSE_VOCAB, True))
    elif kind == "search_like":
        a["labels"] = np.array([l for g in op["groups"] for l in g], np.int64)
        a["weights"] = np.array([w for g in op["weights"] for w in g], np.float64)
        a["offsets"] = offsets_of([len(g) for g in op["groups"]])
        # what the comparison needs of the model's state at this step: the hits are checked against the oracle's search of
        # the queries the DEVICE built
        allowed = ~model._deleted if op.get("program") is None else model.match(program_of(op["program"]))
        a.update(rows=model._rows, allowed=allowed.copy(), space=model.space)
    elif kind == "search_maxsim":
        a["tokens"] = rng.standard_normal((sum(op["lengths"]), d), dtype=np.float32)
        a["offsets"] = offsets_of(op["lengths"])
    elif kind == "search_batch_sparse":
        a["sq"] = _sparse_queries(rng, op["nsq"])


def _facet_list(e, attr, max_values, program):
    try:
        return e.facet_list_values(attr, max_values, program)
    except FacetOverflow as err:  # MLVDB_ERR_OVERFLOW: matched and absent are still exact
        return ("overflow", err.matched, err.absent)


_WIDE_CALLS = {
    "set_attr_at": lambda e, op, a: e.set_attr_at(op["attr"], a["labels"], a["values"]),
    "update_where": lambda e, op, a: e.update_where(a["program"], [tuple(x) for x in op["assigns"]]),
    "tombstone_where": lambda e, op, a: e.tombstone_where(a["program"]),
    "set_attr_list": lambda e, op, a: e.set_attr_list(op["attr"], op["first"], a["col"]),
    "set_attr_list_at": lambda e, op, a: e.set_attr_list_at(op["attr"], a["labels"], a["col"]),
    "update_where_list": lambda e, op, a: e.update_where_list(
        a["program"], op["attr"], None if op["values"] is None else np.array(op["values"], np.int64)),
    "set_attr_sparse": lambda e, op, a: e.set_attr_sparse(op["attr"], op["first"], a["col"]),
    "set_attr_sparse_at": lambda e, op, a: e.set_attr_sparse_at(op["attr"], a["labels"], a["col"]),
    "where_ordered": lambda e, op, a: e.where_ordered(op["attr"], op["limit"], a.get("program"), op["descending"], op["offset"]),
    "search_mmr": lambda e, op, a: e.search_mmr(a["qs"], op["k"], op["fetch_k"], op["lam"], a.get("program"), want64=True),
    "search_grouped": lambda e, op, a: e.search_grouped(a["qs"], op["k"], op["g"], op["attr"], 0, a.get("program"), want64=True),
    "search_like": lambda e, op, a: e.search_like(a["labels"], a["weights"], a["offsets"], op["k"], where=a.get("program"),
                                                  want64=True, want_queries=True),
    "search_maxsim": lambda e, op, a: e.search_maxsim(a["tokens"], a["offsets"], op["k"], op["attr"], a.get("program"),
                                                      want_matches=True),
    "get_attr_list": lambda e, op, a: e.get_attr_list(op["attr"], op["first"], op["n"]),
    "list_stats": lambda e, op, a: e.list_stats(op["attr"]),
    "facet_list_values": lambda e, op, a: _facet_list(e, op["attr"], op["max_values"], a.get("program")),
    "get_attr_sparse": lambda e, op, a: e.get_attr_sparse(op["attr"], op["first"], op["n"]),
    "search_batch_sparse": lambda e, op, a: e.search_batch_sparse(op["attr"], a["sq"], op["k"], a.get("program")),
}


def _wide_refusal(e, op, a):
    """The call of a WIDE_REFUSALS op; every one must end in a ``RuntimeError`` with MLVDB_ERR_INVALID_ARG (a group size of 65:
    MLVDB_ERR_UNSUPPORTED)."""
    which = op["which"]
    if which == "mmr_fetch":
        e.search_mmr(a["qs"], 10, 9, 0.5)
    elif which == "grouped_g0":
        e.search_grouped(a["qs"], 3, 0, 0)
    elif which == "grouped_g65":
        e.search_grouped(a["qs"], 3, MAX_GROUP_SIZE + 1, 0)
    elif which == "like_label":
        e.search_like(a["labels"], a["weights"], a["offsets"], 5)
    elif which in ("maxsim_t0", "maxsim_t129"):
        e.search_maxsim(a["tokens"], a["offsets"], 5, 0)
    elif which == "ordered_window":
        e.where_ordered(2, ORDER_MAX_ROWS - 5, None, False, 6)
    elif which == "set_at_repeat":
        e.set_attr_at(2, np.array([0, 0], np.int64), a["values"])
    elif which == "set_attr_on_list":
        e.set_attr(LIST_A, 0, a["values"][:1])
    elif which == "set_list_on_sparse":
        e.set_attr_list(SPARSE_A, 0, a["col"])
    elif which == "sparse_on_list":
        e.search_batch_sparse(LIST_A, a["sq"], 5)
    else:
        raise ValueError(which)


# ---------------------------------------------------------------- wide ops: comparison
def _same_column(got, want, tag, fields):
    for name in fields:
        g, w = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert g.dtype == w.dtype and g.shape == w.shape, f"{tag}: {name}: {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        assert g.tobytes() == w.tobytes(), f"{tag}: {name} differ"


def _oracle_search64(rows, allowed, space, qs, k):
    from oracle.engine import OracleScanEngine

    o = OracleScanEngine(rows.shape[1], space)
    o._rows, o._deleted = rows, ~allowed
    return o.search64(qs, k)


def _compare_wide(e, op, a, got, want, tag, stats):
    """One branch per new kind, by that feature's own rule (imported from its helpers); True when the kind was one of them."""
    kind = op["op"]
    if kind in ("set_attr_at", "set_attr_list_at", "set_attr_sparse_at", "update_where_list", "list_stats", "update_where"):
        got = tuple(got) if isinstance(got, tuple) else got
        assert got == want, f"{tag}: returned {got}, the model {want}"
    elif kind == "tombstone_where":
        _same(got, want, tag, "labels")
    elif kind == "where_ordered":
        _same(got[0], want[0], tag, "labels")
        _same(got[1], want[1], tag, "values")
        assert tuple(got[2:]) == tuple(want[2:]), f"{tag}: matched / absent {got[2:]}, the model {want[2:]}"
    elif kind == "facet_list_values":
        assert isinstance(got[0], str) == isinstance(want[0], str), f"{tag}: {got[0]!r}, the model {want[0]!r}"
        if isinstance(want[0], str):
            assert tuple(got) == tuple(want), f"{tag}: {got}, the model {want}"
        else:
            _same(got[0], want[0], tag, "values")
            _same(got[1], want[1], tag, "counts")
            assert tuple(got[2:]) == tuple(want[2:]), f"{tag}: matched / absent {got[2:]}, the model {want[2:]}"
    elif kind == "get_attr_list":
        _same_column(got, want, tag, ("offsets", "values", "present"))
    elif kind == "get_attr_sparse":
        _same_column(got, want, tag, ("offsets", "terms", "weights", "present"))
    elif kind == "search_batch_sparse":  # exact weights on both sides: every score is the same fp64 sum in any order
        lab, s32, cnt, s64 = got
        _same(lab, want[0], tag, "labels")
        _same(cnt, want[2], tag, "counts")
        _same(s64, want[3], tag, "score64")
        _same(s32, s64.astype(np.float32), tag, "fp32 against the rounded fp64")
    elif kind == "search_grouped":
        wl, _, wc, wgc, wd, wg = want
        check_grouped(e, a["qs"], op["k"], op["g"], got, (wl, wd, wc, wgc, wg), tag)
        _max_err64(got[4], wd, tag, stats)
    elif kind == "search_maxsim":
        wg, _, wc, ws, wml, wmd = want
        check_maxsim(e, a["tokens"], a["offsets"], op["k"], got, (wg, ws, wc, wml, wmd), tag)
    elif kind == "search_mmr":
        lab, dist, cnt, d64, rank, obj = got
        wl, _, wc, wd, wrank, wobj = want
        if not (np.array_equal(lab, wl) and np.array_equal(rank, wrank) and np.array_equal(cnt, wc)):
            bad = np.flatnonzero((lab != wl).any(axis=1) | (rank != wrank).any(axis=1) | (cnt != wc))
            raise AssertionError(f"{tag}: picks differ in {bad.size} queries, first {bad[0]}: got rank {rank[bad[0]]} "
                                 f"want {wrank[bad[0]]}")
        _max_err64(d64, wd, tag, stats)
        _same(dist, d64.astype(np.float32), tag, "fp32 against the rounded fp64")
        fin = np.isfinite(wobj)
        assert np.array_equal(np.isfinite(obj), fin), f"{tag}: objective padding differs"
        if fin.any():
            err = float(np.abs(obj[fin] - wobj[fin]).max())
            # lam * d(q, i) - (1 - lam) * min_s d(s, i) with 0 <= lam <= 1 inherits at most lam * e + (1 - lam) * e = e from
            # its two distances, e <= D64_BOUND being the premise tests/test_gpu_mmr.py asserts of a device distance
            assert err <= D64_BOUND, f"{tag}: max |objective - oracle| {err}"
    elif kind == "search_like":
        lab, d32, cnt, d64, qs = got
        assert qs.dtype == np.float32 and qs.shape == want[4].shape, f"{tag}: queries {qs.dtype}{qs.shape}"
        if a["space"] != "cosine":
            _same(qs, want[4], tag, "synthesised queries")
        else:
            _, scale = like_queries(a["rows"], a["labels"], a["weights"], a["offsets"], "cosine")
            err = np.abs(qs.astype(np.float64) - want[4].astype(np.float64))
            assert (err <= cosine_query_bound(want[4], scale)).all(), f"{tag}: synthesised queries off by {float(err.max())}"
        most = most_examples(a["labels"], a["offsets"])
        plain = _oracle_search64(a["rows"], a["allowed"], a["space"], qs, op["k"] + most)
        wl, wd32, wc, wd = like_strip(*plain, example_sets(a["labels"], a["offsets"]), op["k"])
        assert_knn_matches((lab, d32, cnt), (wl, wd32, wc), tag)
        _max_err64(d64, wd, tag, stats)
    else:
        return kind in ("set_attr_list", "set_attr_sparse") and got is None and want is None
    return True


# ---------------------------------------------------------------- wide ops: generation
class _WideGenerator(_Generator):
    """The generator over WIDE_MUTATIONS / WIDE_QUERIES: the columns of DESIGN.md 11.5 (0 group, 1 float, 2 tenant, 3 late
    int64, 4 tags, 5 sparse, 6 late tags, 7 late sparse), a program pool with the list ops, and a schedule of its own."""

    def __init__(self, seed, space, d, scale):
        super().__init__(seed, space, d, scale)
        self.defined6 = self.defined7 = False

    # -- columns
    def attrs(self):  # the scalar columns (what the inherited set_attr / get_attr draw from)
        return sorted(a for a in self.model._cols if a not in self.model._lists)

    def pooled(self, sparse=None):
        return sorted(a for a in self.model._lists if sparse is None or (a in self.model._sparse) == sparse)

    def set_pooled(self, attr, first):
        first = min(first, self.total)
        kind = "set_attr_sparse" if attr in self.model._sparse else "set_attr_list"
        self.emit({"op": kind, "attr": int(attr), "first": int(first), "n": int(self.total - first), "seed": self._seed()})

    def set_attrs(self):
        first = max(0, self.last_first - int(self.rng.integers(0, 60)))
        for attr in self.attrs():
            self.set_attr(attr, first)
        for attr in self.pooled():
            self.set_pooled(attr, first)

    def define_late(self):
        for attr in (LATE_LIST, LATE_SPARSE):
            self.emit({"op": "define_attr", "attr": attr, "kind": POOLED[attr]})
        self.defined6 = self.defined7 = True

    # -- programs: the inherited kinds and the list ops, tag leaves AND-ed with scalar ones, EXISTS on a sparse column
    PROGRAMS = ("nothing", "few", "half", "groups", "score", "no_group", "attr3", "has", "has_any", "has_all", "len",
                "tag_and_scalar", "sparse_exists", "late_has")

    def program(self, which=None):
        rng = self.rng
        which = which or self.PROGRAMS[rng.integers(len(self.PROGRAMS))]
        if which == "late_has" and not self.defined6:
            which = "has"
        table = []
        if which == "has":
            ops = [_leaf(W.HAS, LIST_A, rng.integers(TAG_VALUES + 1))]
        elif which == "has_any":
            table = sorted({int(v) for v in rng.integers(0, TAG_VALUES + 2, 3)})
            ops = [_leaf(W.HAS_ANY, LIST_A, 0, len(table))]
        elif which == "has_all":
            table = sorted({int(v) for v in rng.integers(0, TAG_VALUES, 2)})
            ops = [_leaf(W.HAS_ALL, LIST_A, 0, len(table))]
        elif which == "len":
            lo = int(rng.integers(0, 4))
            ops = [_leaf(W.LEN, LIST_A, lo, lo + int(rng.integers(0, 3)))]
        elif which == "tag_and_scalar":
            ops = [_leaf(W.HAS, LIST_A, rng.integers(TAG_VALUES)), _leaf(W.LT, 2, 8), _leaf(W.AND, 0)]
        elif which == "sparse_exists":
            ops = [_leaf(W.EXISTS, SPARSE_A)]
        elif which == "late_has":
            ops = [_leaf(W.HAS, LATE_LIST, rng.integers(TAG_VALUES))]
        elif which == "true":
            ops = [_leaf(W.TRUE, 0)]
        else:
            return super().program(which)
        return {"ops": ops, "set": table}

    def each(self, nq, which=None):
        return super().each(nq, which or ("nothing", "has", "half", "tag_and_scalar"))

    # -- mutations
    def update_where(self, assigns=None, program=None):
        rng = self.rng
        if assigns is None:
            assigns = ([[2, _native.SET_ASSIGN, int(rng.integers(16))]], [[0, _native.SET_ADD, 1]],
                       [[1, _native.SET_ADD, W.float_bits(0.5)]], [[0, _native.SET_ASSIGN, int(ABSENT)]],
                       [[2, _native.SET_ADD, -1], [1, _native.SET_ASSIGN, W.float_bits(-0.0)]])[rng.integers(5)]
        return self.emit({"op": "update_where", "program": program or self.program(), "assigns": assigns})

    def set_attr_at(self, attr=None, **extra):
        attr = int(self.rng.choice(self.attrs())) if attr is None else attr
        return self.emit({"op": "set_attr_at", "attr": attr, "n": int(self.rng.integers(1, 40)), "seed": self._seed(), **extra})

    def set_pooled_at(self, attr, n=None, lo=0):
        kind = "set_attr_sparse_at" if attr in self.model._sparse else "set_attr_list_at"
        n = int(self.rng.integers(1, 60)) if n is None else int(n)
        return self.emit({"op": kind, "attr": int(attr), "n": n, "lo": int(lo), "seed": self._seed()})

    def reset_to(self, space):
        self.emit({"op": "reset", "space": space})
        self.last_first = 0

    def tombstone_where(self, which=None):
        which = which or ("few", "has_all", "groups", "tag_and_scalar", "len")[self.rng.integers(5)]
        return self.emit({"op": "tombstone_where", "program": self.program(which)})

    def mutate(self, kind):
        rng = self.rng
        if kind not in NEW_MUTATIONS:
            return super().mutate(kind)
        if kind == "set_attr_at":
            return self.set_attr_at()
        if kind == "update_where":
            return self.update_where()
        if kind == "tombstone_where":
            return self.tombstone_where()
        sparse = "sparse" in kind
        attr = int(rng.choice(self.pooled(sparse)))
        if kind in ("set_attr_list", "set_attr_sparse"):
            return self.set_pooled(attr, int(rng.integers(0, max(self.total, 1))))
        if kind in ("set_attr_list_at", "set_attr_sparse_at"):
            return self.set_pooled_at(attr)
        values = (None, [], [1, 7], [0, 2, 5])[rng.integers(4)]
        return self.emit({"op": "update_where_list", "attr": attr, "program": self.program(), "values": values})

    # -- near-ties of the new kNN kinds, from the oracle alone
    def _where_mask(self, op):
        m = self.model
        return ~m._deleted if op.get("program") is None else m.match(program_of(op["program"]))

    def _grouped_ok(self, op):
        """The distinct rule, then the rows of each picked group up to group_size + 1."""
        if not self._knn_ok({**op, "op": "search_distinct"}):
            return False
        m, k, g = self.model, op["k"], op["g"]
        dist = self._dist(_queries(op, self.d))
        groups, allowed = m._cols[op["attr"]], self._where_mask(op)
        _, _, counts, grp = distinct_helpers.distinct_knn(dist, groups, allowed, k)
        for i in range(op["nq"]):
            for code in grp[i, :counts[i]].tolist():
                idx = np.flatnonzero(allowed & (groups == code))
                if not _gaps_ok(np.sort(dist[i, idx])[:g + 1]):
                    return False
        return True

    def _maxsim_ok(self, op):
        """Neighbouring document scores among the first k + 1, and the best and second-best row of every (token, picked
        document) pair, more than TIE_REL max(1, |s|) apart (or equal: the order is then by code / by label on both sides)."""
        m, k = self.model, op["k"]
        a = materialise(m, op)
        groups, allowed = m._cols[op["attr"]], self._where_mask(op)
        dist = exact_scan.exact_distances(a["tokens"], m._rows, m.space)
        grp, s64, counts, _, _ = maxsim_oracle(dist, groups, allowed, a["offsets"], k + 1)
        off = a["offsets"]
        for i in range(len(op["lengths"])):
            c = int(counts[i])
            if not _gaps_ok(s64[i, :c]):
                return False
            for code in grp[i, :min(c, k)].tolist():
                idx = np.flatnonzero(allowed & (groups == code))
                if idx.size > 1:
                    two = np.sort(dist[off[i]:off[i + 1]][:, idx], axis=1)[:, :2]
                    gap = two[:, 1] - two[:, 0]
                    if ((gap > 0) & (gap <= TIE_REL * np.maximum(1.0, np.abs(two[:, 1])))).any():
                        return False
        return True

    def _mmr_ok(self, op):
        """The plain rule on the first fetch_k + 1 candidates, and every step's best and runner-up objective either equal (bit
        copies of a row: both sides then take the better-ranked one) or more than GAP_MIN apart."""
        if not self._knn_ok({**op, "k": op["fetch_k"]}):
            return False
        m = self.model
        where = None if op.get("program") is None else program_of(op["program"])
        cl, _, cc, cd64 = m.search64(_queries(op, self.d), op["fetch_k"], where=where)
        gaps = []
        for i in range(op["nq"]):
            c = cl[i, :cc[i]]
            if c.size:
                mmr_select(cd64[i, :cc[i]], exact_scan.exact_distances(m._rows[c], m._rows[c], m.space), op["k"], op["lam"], gaps)
        gaps = np.array(gaps)
        return not ((gaps > 0) & (gaps <= GAP_MIN)).any()

    def _like_ok(self, op):
        """The plain rule at k + M + 1 on the helper's queries; on cosine the gaps must also exceed LIKE_COSINE_GAP."""
        m = self.model
        if self.total < 2 or not op["groups"]:
            return True
        a = materialise(m, op)
        qs, _ = like_queries(m._rows, a["labels"], a["weights"], a["offsets"], m.space)
        dist = self._dist(qs)
        extra = LIKE_COSINE_GAP if m.space == "cosine" else 0.0
        cut = op["k"] + most_examples(a["labels"], a["offsets"]) + 1
        for i in range(qs.shape[0]):
            s = np.sort(dist[i, a["allowed"]])[:cut]
            gaps = np.diff(s)
            if ((gaps > 0) & (gaps <= extra + TIE_REL * np.maximum(1.0, np.abs(s[1:])))).any():
                return False
        return True

    def _draw(self, make, ok):
        while True:
            self.drawn += 1
            op = make()
            if self.total < 2 or ok(op):
                return self.emit(op)
            self.redraws += 1

    # -- queries
    def query(self, kind, **kw):
        rng, total = self.rng, self.total
        if kind == "search_distinct" and "program" not in kw:  # (the inherited branch draws from the scalar kinds alone)
            kw["program"] = self.program(("has", "tag_and_scalar", "half", "no_group", "has_any", "len")[rng.integers(6)]) \
                if rng.random() < 0.5 else None
        if kind not in NEW_QUERIES:
            return super().query(kind, **kw)
        program = kw.pop("program", "random")
        if program == "random":
            program = self.program() if rng.random() < 0.5 else None
        group_attr = kw.pop("attr", None)
        if kind == "where_ordered":
            attr = int(rng.choice(self.attrs())) if group_attr is None else group_attr
            limit, offset = ((1, 0), (20, 0), (5, 7), (ORDER_MAX_ROWS, 0), (50, ORDER_MAX_ROWS - 50))[rng.integers(5)]
            return self.emit({"op": kind, "attr": attr, "limit": limit, "offset": offset, "descending": bool(rng.random() < 0.5),
                              "program": program})
        if kind == "search_mmr":
            nq = int(kw.pop("nq", (1, 3, 12)[rng.integers(3)]))
            k, fetch_k = ((1, 1), (5, 5), (5, 40), (10, 100), (32, 256), (64, 64))[rng.integers(6)]
            lam = float((0.0, 0.3, 0.7, 1.0)[rng.integers(4)])
            return self._draw(lambda: {"op": kind, "nq": nq, "k": k, "fetch_k": fetch_k, "lam": lam, "seed": self._seed(),
                                       "program": program}, self._mmr_ok)
        if kind == "search_grouped":
            nq = int(kw.pop("nq", (1, 3, 12)[rng.integers(3)]))
            k, g = ((1, 1), (5, 3), (10, 2), (3, 64), (64, 1))[rng.integers(5)]
            attr = 0 if group_attr is None else group_attr
            return self._draw(lambda: {"op": kind, "nq": nq, "k": k, "g": g, "attr": attr, "seed": self._seed(),
                                       "program": program}, self._grouped_ok)
        if kind == "search_like":
            nq = int(kw.pop("nq", (1, 3, 12)[rng.integers(3)])) if total else 0
            k = int((1, 5, 10)[rng.integers(3)])
            pool = kw.pop("examples", None)

            def make():
                groups, weights = [], []
                for _ in range(nq):
                    m = min(int((1, 1, 2, 4, 16)[rng.integers(5)]), total)
                    src = np.arange(total) if pool is None else np.asarray(pool)
                    groups.append(rng.choice(src, min(m, src.size), replace=False).tolist())
                    weights.append([1.0] + [float(w) for w in rng.choice([0.5, -0.25, 0.75, 2.0], len(groups[-1]) - 1)])
                return {"op": kind, "k": k, "groups": groups, "weights": weights, "program": program}
            return self._draw(make, self._like_ok)
        if kind == "search_maxsim":
            lengths = [int(x) for x in rng.choice([1, 3, 8, 9], int(kw.pop("nq", (1, 3)[rng.integers(2)])))]
            k = int((1, 5, 10)[rng.integers(3)])
            attr = 0 if group_attr is None else group_attr
            return self._draw(lambda: {"op": kind, "lengths": lengths, "k": k, "attr": attr, "seed": self._seed(),
                                       "program": program}, self._maxsim_ok)
        sparse = kind in ("get_attr_sparse", "search_batch_sparse") or (kind == "list_stats" and rng.random() < 0.5)
        attr = int(rng.choice(self.pooled(sparse))) if group_attr is None else group_attr
        if kind in ("get_attr_list", "get_attr_sparse"):
            first = int(kw.pop("first", rng.integers(0, total + 1)))
            return self.emit({"op": kind, "attr": attr, "first": first, "n": int(min(total - first, kw.pop("n", rng.integers(0, 300))))})
        if kind == "list_stats":
            return self.emit({"op": kind, "attr": attr})
        if kind == "facet_list_values":
            return self.emit({"op": kind, "attr": attr, "max_values": int(kw.pop("max_values", (4096, 4096, 3)[rng.integers(3)])),
                              "program": program})
        if kind == "search_batch_sparse":
            return self.emit({"op": kind, "attr": attr, "nsq": int((1, 5, 9)[rng.integers(3)]), "k": int((1, 10, 64)[rng.integers(3)]),
                              "seed": self._seed(), "program": program})
        raise ValueError(kind)

    def refuse(self, which, **extra):
        if which not in WIDE_REFUSALS:
            return super().refuse(which)
        op = {"op": "refuse", "which": which, **extra}
        if which in ("mmr_fetch", "grouped_g0", "grouped_g65"):
            op.update(nq=3, seed=self._seed())
        elif which in ("maxsim_t0", "maxsim_t129", "sparse_on_list"):
            op["seed"] = self._seed()
        elif which == "like_label" and "label" not in op:
            op["label"] = self.total
        return self.emit(op)

    # -- the schedule (the coverage conditions k to w of tests/test_history_host.py)
    READS = ("get_attr_list", "get_attr_sparse", "where_count", "facet_list_values", "search_batch_sparse")

    def _read_pooled(self, list_attr, sparse_attr, stats=True):
        which = "has" if list_attr == LIST_A else "late_has"
        self.query("get_attr_list", attr=list_attr, first=0, n=200)
        self.query("get_attr_sparse", attr=sparse_attr, first=0, n=200)
        self.query("where_count", program=self.program(which))
        self.query("facet_list_values", attr=list_attr, program=None, max_values=4096)
        self.query("search_batch_sparse", attr=sparse_attr, program=None)
        if stats:
            self.query("list_stats", attr=list_attr)
            self.query("list_stats", attr=sparse_attr)

    def _tag_query(self, attr):
        if attr in self.model._sparse:
            self.query("search_batch_sparse", attr=attr, program=None)
        else:
            self.query("where_count", program=self.program("has" if attr == LIST_A else "late_has"))

    def wide(self):
        rng, seed = self.rng, self.seed
        for attr, kind in ((0, "int64"), (1, "float64"), (2, "int64"), (LIST_A, "int64_list"), (SPARSE_A, "sparse")):
            self.emit({"op": "define_attr", "attr": attr, "kind": kind})
        self.append("hundreds")
        self.set_attrs()
        items = [lambda m=m, q=q: (self.ensure_rows(), self.mutate(m), self.query(q))  # (k)
                 for m, q in WIDE_PAIRS[seed % WIDE_PAIR_SLICES::WIDE_PAIR_SLICES]]

        def garbage(attr, tombstones):  # (l)
            self.ensure_rows()
            if not tombstones and self.model.counts()[1]:
                self.compact()
            for _ in range(2):  # half the rows overwritten twice: their old values stay behind in the pool
                self.set_pooled_at(attr, n=max(1, self.live.size // 2))
            if tombstones:
                self.tombstone("frac")
            self.compact()
            self._tag_query(attr)
            self.query("list_stats", attr=attr)

        def doubling(attr):  # (m)
            self.ensure_rows(300)
            self.compact()  # capacity = used = the live values
            lo = self.total // 2  # rows [0, lo) keep what they held before the first regrowth
            cap, grown = self.model._pool_cap[attr], 0
            for _ in range(16):
                used = self.model._pool_used[attr]
                self.set_pooled_at(attr, n=self.total - lo, lo=lo)
                if self.model._pool_cap[attr] != cap and used > 0:
                    cap, grown = self.model._pool_cap[attr], grown + 1
                if grown >= 2:
                    break
            assert grown >= 2
            self.query("get_attr_sparse" if attr in self.model._sparse else "get_attr_list", attr=attr, first=0, n=lo)
            self._tag_query(attr)

        def regrowth():  # (n)
            self.ensure_rows()
            for _ in range(2):
                self.append("cross")
                self.set_attrs()
            self._read_pooled(LIST_A, SPARSE_A, stats=False)

        def reset(other):  # (o)
            self.ensure_rows()
            self.reset(other)
            self.append("hundreds")
            self._read_pooled(LIST_A, SPARSE_A)
            self.set_attrs()
            self._read_pooled(LIST_A, SPARSE_A)

        def filter_inner(inner, x):  # (p)
            self.ensure_rows()
            self.strategy("filter")
            self.query(inner)
            {"tombstone_where": self.tombstone_where, "tombstone": self.tombstone, "append": self.append, "compact": self.compact}[x]()
            self.query(inner)
            self.strategy("auto")

        def l2_inner():  # (p), the offsets plane
            if self.model.space != "l2":
                self.reset_to("l2")
            self.ensure_rows()
            self.strategy("filter")
            self.query("search_mmr", nq=12)
            self.query("search_like", nq=3)
            self.tombstone_where("few")
            self.query("search", nq=12, k=10)
            self.strategy("auto")

        def masked(kind):  # (q)
            self.ensure_rows()
            for after in ("search64", kind):
                self.query(kind, program=self.program(("half", "has", "tag_and_scalar")[rng.integers(3)]))
                if after == kind:
                    self.query(kind, program=None)
                else:
                    self.query("search64")

        def late_columns():  # (r)
            self.ensure_rows()
            self.define_late()
            self._read_pooled(LATE_LIST, LATE_SPARSE, stats=False)
            self.set_pooled(LATE_LIST, 0)
            self.set_pooled(LATE_SPARSE, 0)
            self._read_pooled(LATE_LIST, LATE_SPARSE, stats=False)

        def group_column(writer, reader):  # (s)
            self.ensure_rows()
            if writer == "update_where":  # rows of many groups move into one: a program that matches some
                program = self.program(("half", "has", "few")[rng.integers(3)])
                if not self.model.where_count(program_of(program)):
                    program = self.program("true")
                self.update_where([[0, _native.SET_ASSIGN, int(rng.integers(0, 5))]], program)
            else:
                self.set_attr_at(0)
            self.query(reader, attr=0)

        def float_add():  # (s)
            self.ensure_rows()
            self.update_where([[1, _native.SET_ADD, W.float_bits(0.5)]], self.program("half"))
            self.query("where_ordered", attr=1)

        def refused_update():  # (t)
            self.ensure_rows()
            label = int(rng.choice(self.live))
            self.set_attr_at(2, labels=[label], values=[INT64_MAX - 1])  # the one row whose sum cannot be stored
            matched, refused = self.update_where([[2, _native.SET_ADD, 5], [0, _native.SET_ASSIGN, 7]],
                                                 {"ops": [_leaf(W.GE, 2, 0)], "set": []})
            assert refused > 0
            self.emit({"op": "get_attr", "attr": 2, "float": False, "first": 0, "n": self.total})
            self.emit({"op": "get_attr", "attr": 0, "float": False, "first": 0, "n": self.total})
            self.set_attr_at(2, labels=[label], values=[3])

        def renumbered():  # (u)
            self.ensure_rows()
            dead = [int(x) for x in rng.choice(self.live[:self.live.size // 2], 5, replace=False)]
            self.emit({"op": "tombstone", "mode": "labels", "labels": dead})
            self.query("search_like", examples=dead, program=None)
            self.emit({"op": "get_rows_at", "labels": dead})
            old_total = self.total
            self.compact()
            self.query("search_like", program=None)
            self.emit({"op": "get_rows_at", "labels": rng.integers(0, self.total, 6).tolist()})
            self.refuse("like_label", label=old_total - 1)
            self.query("search64")

        def refusals():  # (v)
            self.ensure_rows()
            for i, which in enumerate(WIDE_REFUSALS):
                if i % 2 == seed % 2:
                    self.refuse(which)
                    self.query(("search64", "search_grouped", "where_ordered", "search_batch_sparse", "facet_list_values")[rng.integers(5)])

        def empty(how):  # (w)
            self.ensure_rows()
            if how == "compact":
                self.tombstone_where("true")
                self.compact()
            else:
                self.reset(False)
            for _ in range(2):
                for kind in NEW_QUERIES:
                    self.query(kind)
                if self.total == 0:
                    self.append("hundreds")
                    self.set_attrs()

        def deaths():  # filtered deletes, then the two entries whose inner search must not return them
            self.ensure_rows()
            self.tombstone_where("half")
            self.query("search_mmr", program=None)
            self.query("search_like", program=None)

        xs = ("tombstone_where", "tombstone", "append", "compact")
        combos = [(inner, x) for inner in INNER_SEARCHES for x in xs]
        items += [lambda c=combos[(8 * seed + i) % 16]: filter_inner(*c) for i in range(8)]
        writers = [(w, r) for w in ("update_where", "set_attr_at") for r in ("search_grouped", "search_maxsim", "search_distinct", "where_ordered")]
        items += [lambda c=c: group_column(*c) for c in writers[seed % 2::2]]
        if seed % 2 == 0:  # (every history: documents that changed under a late-interaction search)
            items.append(lambda: group_column("update_where", "search_maxsim"))
        items += [lambda: garbage(LIST_A, seed % 2 == 0), lambda: garbage(SPARSE_A, seed % 2 == 1), lambda: doubling(LIST_A),
                  lambda: doubling(SPARSE_A), regrowth, lambda: reset(seed % 2 == 1), late_columns, float_add, refused_update, renumbered,
                  refusals, lambda: empty("compact" if seed // 2 % 2 == 0 else "reset"), deaths]
        items += [lambda kind=kind: masked(kind) for kind in MASKABLE]
        if self.model.space == "l2":
            items.append(l2_inner)
        items += [lambda: (self.ensure_rows(), self.query(WIDE_QUERIES[rng.integers(len(WIDE_QUERIES))])) for _ in range(4)]
        for i in rng.permutation(len(items)):
            items[i]()

    def wide_large(self):
        """The pattern of ``large()`` over the newer entries: appends of 12,000 rows until past 32,768 (`auto` moves the inner
        search of search_mmr / search_like / search_grouped and the tag-filtered search_each to the filter route at nq = 12 and
        40), a ``tombstone_where`` of about a third of the rows, a compaction back below the threshold, growth again."""
        for attr, kind in ((0, "int64"), (1, "float64"), (2, "int64"), (LIST_A, "int64_list"), (SPARSE_A, "sparse")):
            self.emit({"op": "define_attr", "attr": attr, "kind": kind})
        self.append(n=12000)
        self.set_attrs()
        self.query("search_mmr", nq=12, program=None)  # below the threshold: the exact scan inside
        for _ in range(2):
            self.append(n=12000)
            self.set_attrs()
        self.query("search_mmr", nq=12, program=None)
        self.query("search_like", nq=12, program=self.program("has"))
        self.query("search_grouped", nq=40, program=None)
        self.query("search_maxsim", program=self.program("half"))
        self.query("search_each", nq=12, k=10)
        self.query("search_each", nq=40, k=10)
        third = {"ops": [_leaf(W.HAS, LIST_A, 3), _leaf(W.LT, 2, 2), _leaf(W.OR, 0)], "set": []}
        self.emit({"op": "tombstone_where", "program": third})
        self.query("search_mmr", nq=40, program=self.program("tag_and_scalar"))
        self.query("search_like", nq=12, program=None)
        self.compact()
        assert self.total < FILTER_MIN_ROWS
        self.query("search_grouped", nq=12, program=self.program("has"))
        self.query("search_like", nq=12, program=None)
        self.query("search_mmr", nq=12, program=None)
        self.append(n=12000)
        assert self.total > FILTER_MIN_ROWS
        self.set_attrs()
        self.query("search_mmr", nq=12, program=None)
        self.query("search_like", nq=12, program=self.program("tag_and_scalar"))
        self.query("search_grouped", nq=12, program=None)
        self.query("search_maxsim", program=None)
        self.query("search_each", nq=12, k=10)
        self.query("search_distinct", k=10)
        self.query("search_batch_sparse", attr=SPARSE_A)
        self.query("facet_list_values", attr=LIST_A, max_values=4096)


@functools.lru_cache(maxsize=None)
def _history(seed, space, d, scale):
    if scale in _recent().RECENT_SCALES:
        g = _recent()._RecentGenerator(seed, space, d, scale)
    else:
        g = (_WideGenerator if scale in WIDE_SCALES else _Generator)(seed, space, d, scale)
    getattr(g, scale)()
    return g


def make_history(seed: int, space: str, d: int, scale: str = "small"):
    """(ops, expected) of one history: ``ops[i]`` is a dict of plain parameters, ``expected[i]`` = {"args": the arrays the op is
    called with, "want": the model's answer, "counts": (total, deleted) after a mutation}.  Deterministic per (seed, space, d,
    scale); cached (the expected answers are shared and must not be written to)."""
    g = _history(seed, space, d, scale)
    return g.ops, g.expected


def redraw_counts(seed, space, d, scale="small"):
    """(queries drawn, of them redrawn because of a near-tie) while the history was generated."""
    g = _history(seed, space, d, scale)
    return g.drawn, g.redraws


# The committed seed set: (seed, space, d, scale).
SMALL = [(2 * i + j, space, d, "small") for i, (space, d) in
         enumerate([("l2", 20), ("cosine", 64), ("ip", 128), ("l2", 256), ("cosine", 100)]) for j in range(2)]
LARGE = [(100 + i, space, 64, "large") for i, space in enumerate(SPACES)]
MULTI = [(200, "cosine", 48, "multi")]
HISTORIES = SMALL + LARGE + MULTI
WIDE = [(300 + 2 * i + j, space, d, "wide") for i, (space, d) in
        enumerate([("l2", 20), ("cosine", 64), ("ip", 128), ("l2", 256), ("cosine", 100), ("ip", 48)]) for j in range(2)]
WIDE_LARGE = [(400 + i, space, 64, "wide_large") for i, space in enumerate(SPACES)]


def history_tag(seed, space, d, scale):
    return f"{scale}_{space}_d{d}_seed{seed}"
