"""Seeded call histories on ONE engine handle, replayed against a NumPy model of the whole engine.

``HistoryModel`` is one oracle engine with every entry point of ``HipScanEngine``; ``make_history`` builds a list of plain,
JSON-serialisable ops from a shuffled schedule (the coverage conditions of tests/test_history_host.py) padded with random
steps, running the model as it goes, and returns the ops with the model's answers; ``run_history`` applies them to an engine
one by one and compares every answer at once.  Nothing here needs a GPU."""
from __future__ import annotations

import functools
import json
import re

import numpy as np

from mlvectordb_amd import where as W
from mlvectordb_amd.engine import FacetOverflow
from oracle import exact_scan
from tests.distinct_helpers import ABSENT, DistinctOracleEngine
from tests.facet_helpers import FacetOracleEngine
from tests.helpers import SCORE_ATOL, assert_knn_matches, assert_range_matches
from tests.where_helpers import FLOAT_POOL, EachOracleEngine, EachRangeOracleEngine

SPACES = ("l2", "cosine", "ip")
SCALES = ("small", "large", "multi")
TILE_ROWS = 768          # layout.h: kTileRows, the granule of the row capacity
FILTER_MIN_ROWS = 32768  # api.hip: use_filter, the corpus at which `auto` takes the filter route for nq >= 12
MAX_ROWS_SMALL = 6000
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
    raise ValueError(f"unknown op {kind!r}")


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
            raise ValueError(which)
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
    if kind in ("append", "tombstone"):
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
    else:
        assert got is None and want is None, f"{tag}: returned {got!r}"


def _evidence(x, prefix, out):
    if isinstance(x, (tuple, list)) or hasattr(x, "offsets"):
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
            if op["op"] in MUTATIONS:
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
        assert space in SPACES and scale in SCALES
        self.seed, self.d, self.scale = seed, d, scale
        self.rng = np.random.default_rng([seed, d, SPACES.index(space), SCALES.index(scale)])
        self.model = HistoryModel(d, space)
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
        if op["op"] in MUTATIONS:
            exp["counts"] = self.model.counts()
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
        if self.scale != "large" and self.total + n > MAX_ROWS_SMALL:  # keep the corpus small: drop most rows first
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


@functools.lru_cache(maxsize=None)
def _history(seed, space, d, scale):
    g = _Generator(seed, space, d, scale)
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


def history_tag(seed, space, d, scale):
    return f"{scale}_{space}_d{d}_seed{seed}"
