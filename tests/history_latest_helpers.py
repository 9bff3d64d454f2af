"""The fourth wave of call histories: scored kNN, recommend / discover, the dense and the bit-code similarity
join, bit-code range search and clustering on ONE handle, interleaved with every mutation and query of the recent wave.
``LatestHistoryModel`` is ``RecentHistoryModel`` composed with the six families' own oracle engines, ``_LatestGenerator``
extends the recent generator by two int64 columns (12 cluster, 13 late cluster), two mutations (clustering that writes a
column), seven queries and two program kinds, and the ``latest`` / ``latest_large`` schedules carry the coverage conditions of
tests/test_history_host.py.  ``history_helpers.call`` / ``compare`` / ``_history`` dispatch here for the new op kinds and
scales; the op lists of every earlier key are untouched.  Nothing here needs a GPU.

How an answer is compared (no tolerance of this module's own):
  scored, examples   every output in every bit against the family's model (``scored_topk`` / ``model_search``) fed with the
                     MODEL's state -- live rows, columns, cond masks, example labels -- and the engine's own ``pair_distances``,
                     which is the rule of tests/test_gpu_scored.py and tests/test_gpu_examples.py.
  clustering         candidates, sizes, iterations, converged and the centroids (a function of the rows and the assignment
                     alone) in every bit against the model; costs in every bit against the model's loop on the engine's own
                     ``pair_distances``; after a writing call the whole column is read back and equals the model's.  The
                     generator redraws (counted) a call in which a candidate's two best centroids are a near-tie.
  join_within        labels, counts, offsets and order exactly, distances by ``assert_range_matches``; the generator redraws a
                     radius within TIE_REL of a distance, or hits of one left row that are a near-tie.
  bits               labels, counts, offsets, fp32 and fp64 distances in every bit."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import _native as N
from mlvectordb_amd import score as S
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import RangeHits
from oracle import exact_scan
from tests import history_helpers as H
from tests import history_recent_helpers as R
from tests.bits_helpers import METRICS
from tests.bits_range_helpers import MAX_HITS, BitsRangeOracleEngine, range_bits
from tests.cluster_helpers import (NO_CANDIDATE, ClusterOracleEngine, centroid_vectors, model_assign, model_kmeans, model_means,
                                   model_sizes_costs)
from tests.examples_helpers import BEST, CONTEXT, DISCOVER, NEG, POS, TARGET, ExamplesOracleEngine, example_vectors, model_search, random_bags
from tests.helpers import assert_range_matches
from tests.history_helpers import TIE_REL, Refused, Unsupported, _gaps_ok, _leaf, _same
from tests.join_helpers import LATER, OTHERS, JoinOracleEngine, native_join
from tests.scored_helpers import ScoredOracleEngine, score_eval, scored_topk

LATEST_SCALES = ("latest", "latest_large")
CLUSTER_A, LATE_CLUSTER = 12, 13
MAX_TOPK = R.MAX_TOPK
WRITERS = ("assign_write", "kmeans_write")  # clustering with assign_attr >= 0: the two new mutations
LATEST_MUTATIONS = R.RECENT_MUTATIONS + WRITERS
LATEST_NEW_QUERIES = ("search_scored", "search_examples", "join_within", "range_bits", "join_within_bits", "assign_nearest", "kmeans")
LATEST_QUERIES = R.RECENT_QUERIES + LATEST_NEW_QUERIES
KMEANS_KINDS = ("kmeans_write", "kmeans")  # refused on an ip index: their pairs and programs go to the l2 / cosine histories
LATEST_PAIRS = [(m, q) for m in LATEST_MUTATIONS for q in LATEST_QUERIES if m in WRITERS or q in LATEST_NEW_QUERIES]
PAIRS_ANY = [p for p in LATEST_PAIRS if not set(p) & set(KMEANS_KINDS)]
PAIRS_KMEANS = [p for p in LATEST_PAIRS if set(p) & set(KMEANS_KINDS)]
LATEST_PROGRAMS = ("cluster", "cluster_absent")
NEW_TAKING = LATEST_NEW_QUERIES + WRITERS  # every new entry takes a program
PROGRAM_TAKING = R.PROGRAM_TAKING + NEW_TAKING
SCORES = ("dist_attr", "dist_float", "match", "cluster_operand", "min_abs")
MODES = (BEST, DISCOVER, CONTEXT)
JOIN_MODES = (OTHERS, LATER)
# one per distinct host refusal of the six headers: name -> status (MLVDB_ERR_INVALID_ARG 1, MLVDB_ERR_UNSUPPORTED 6).  The two
# capacity refusals of mlvdb_join_within are asked of the C entry itself (``join_helpers.native_join``, as tests/test_gpu_join.py
# does): ``HipScanEngine.join_within`` clamps the capacity into 1 .. MLVDB_JOIN_MAX_CAPACITY before the call.
LATEST_REFUSALS = {
    "scored_k0": 1, "scored_k65": 6, "scored_no_ops": 1, "scored_underflow": 1,
    "examples_k0": 1, "examples_k65": 6, "examples_bag65": 6, "examples_empty_bag": 1, "examples_label": 1, "examples_roles": 1,
    "examples_nan": 1, "examples_mode": 1,
    "join_unsorted": 1, "join_label": 1, "join_mode": 1,
    "cluster_m0": 1, "cluster_m_max": 1, "cluster_label": 1, "cluster_attr_float": 1, "cluster_attr_undefined": 1, "cluster_nan": 1,
    "cluster_iter0": 1, "cluster_iter_max": 6, "kmeans_ip": 6,
    "bits_range_capacity0": 1, "bits_range_capacity_max": 6, "bits_range_nan": 1, "bits_range_not_bits": 1, "bits_range_words0": 1,
    "bits_join_unsorted": 1, "bits_join_label": 1, "bits_join_words0": 1, "bits_join_capacity_max": 6, "bits_join_nan": 1,
    "bits_join_mode": 1, "bits_join_not_bits": 1,
    "join_capacity0": 1, "join_capacity_max": 6,
}


# ---------------------------------------------------------------- the model
def score_of(s) -> S.ScoreProgram:
    """A ``score.ScoreProgram`` from its JSON form {"ops": [[op, attr, a], ...], "conds": [program, ...]}."""
    return S.ScoreProgram(np.array([tuple(o) for o in s["ops"]], dtype=S.OP_DTYPE).reshape(-1), [H.program_of(c) for c in s["conds"]])


def score_depths(ops):
    """The stack depth after every op of a score program, or None where an op pops more than the stack holds."""
    depth, out = 0, []
    for op, _, _ in ops:
        pops = 0 if op in (S.CONST, S.DIST, S.ATTR, S.MATCH) else 1 if op in (S.NEG, S.ABS) else 2
        if depth < pops:
            return None
        depth += 1 - pops
        out.append(depth)
    return out


class LatestHistoryModel(R.RecentHistoryModel, ScoredOracleEngine, ExamplesOracleEngine, JoinOracleEngine, ClusterOracleEngine,
                         BitsRangeOracleEngine):
    """``RecentHistoryModel`` + the six newest families, composed from their oracle engines.  Where the engines disagree it is
    resolved here, once: every cond, filter and candidate set goes through the ONE ``match`` of the recent model (the scored
    engine evaluates its conds with the scalar evaluator, the cluster engine asks ``match``), and the host refusals of the six
    headers are raised as ``Refused`` / ``Unsupported`` before any state changes."""

    def _program(self, where):
        if where is not None:
            self.match(where)  # (raises for an undefined column or a leaf the column's kind does not take)

    def _stored(self, labels, what, low=-1):
        labels = np.asarray(labels, np.int64)
        if labels.size and (labels.min() < low or labels.max() >= self._rows.shape[0]):
            raise Refused(f"{what}: a label outside [{low}, total)")

    # -- scored kNN
    def search_scored(self, queries, k, program, where=None, want64=False):
        ops = program.ops.tolist()
        if k < 1:
            raise Refused("search_scored: k >= 1")
        if k > MAX_TOPK:
            raise Unsupported("search_scored: k above MLVDB_MAX_TOPK")
        depths = score_depths(ops) if ops else None
        if not 1 <= len(ops) <= S.MAX_OPS or depths is None or depths[-1] != 1 or max(depths) > S.MAX_DEPTH or len(program.conds) > S.MAX_CONDS:
            raise Refused("search_scored: a bad score program")
        for op, attr, a in ops:
            if op == S.ATTR and (attr in self._lists or self._is(attr, "geo") or attr not in self._cols):
                raise Refused("search_scored: ATTR needs an int64 or float64 column")
            if op == S.MATCH and not 0 <= a < len(program.conds):
                raise Refused("search_scored: MATCH of a cond that is not there")
        for c in program.conds:
            self._program(c)
        self._program(where)
        D = exact_scan.exact_distances(queries, self._rows, self.space)
        masks = [self.match(c) for c in program.conds]
        out = scored_topk(score_eval(program, D, self._cols, masks), k, self._mask(where), D)
        return out if want64 else out[:3]

    # -- recommend / discover
    def search_examples(self, mode, labels, vectors, roles, offsets, k, *, exclude=True, where=None):
        labels, roles, offsets = np.asarray(labels, np.int64), np.asarray(roles), np.asarray(offsets, np.int64)
        sizes = np.diff(offsets)
        if k < 1 or mode not in MODES or (sizes < 1).any():
            raise Refused("search_examples: k >= 1, a known mode, no empty bag")
        self._stored(labels, "search_examples")
        if vectors is not None and not np.isfinite(np.asarray(vectors)[labels < 0]).all():
            raise Refused("search_examples: a non-finite raw vector")
        for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
            r = roles[a:b].tolist()
            head = 1 if mode == DISCOVER else 0
            ok = set(r) <= {POS, NEG} if mode == BEST else (r[:head] == [TARGET] * head and r[head:] == [POS, NEG] * ((b - a - head) // 2)
                                                            and (b - a - head) % 2 == 0 and (mode == DISCOVER or b - a >= 2))
            if not ok and b - a <= N.EXAMPLES_MAX:
                raise Refused("search_examples: a role sequence the mode does not allow")
        self._program(where)
        if k > MAX_TOPK or (sizes > N.EXAMPLES_MAX).any():
            raise Unsupported("search_examples: k or a bag above its limit")
        return super().search_examples(mode, labels, vectors, roles, offsets, k, exclude=exclude, where=where)

    # -- the dense join
    def join_within(self, labels, mode, radius, capacity, where=None, truncate=False):
        left = np.asarray(labels, np.int64)
        if mode not in JOIN_MODES or capacity < 1 or (np.diff(left) <= 0).any():
            raise Refused("join_within: a known mode, capacity >= 1, labels that ascend strictly")
        self._stored(left, "join_within", 0)
        self._program(where)
        if capacity > N.JOIN_MAX_CAPACITY:
            raise Unsupported("join_within: capacity above MLVDB_JOIN_MAX_CAPACITY")
        return super().join_within(left, mode, radius, capacity, where, truncate)

    # -- clustering
    def _centroid_args(self, labels, vectors, assign_attr, where, what):
        m = len(labels) if labels is not None else len(vectors)
        if not 1 <= m <= N.CLUSTER_MAX:
            raise Refused(f"{what}: m outside 1 .. MLVDB_CLUSTER_MAX")
        if labels is not None:
            self._stored(labels, what)
            raw = np.asarray(labels) < 0
            if raw.any() and (vectors is None or not np.isfinite(np.asarray(vectors)[raw]).all()):
                raise Refused(f"{what}: a raw centroid without a finite vector")
        elif not np.isfinite(np.asarray(vectors)).all():
            raise Refused(f"{what}: a non-finite raw centroid")
        if assign_attr != -1 and (assign_attr not in self._cols or assign_attr in self._lists or self._is(assign_attr, "geo")
                                  or self._cols[assign_attr].dtype != np.int64):
            raise Refused(f"{what}: assign_attr is neither -1 nor a defined int64 column")
        self._program(where)

    def assign_nearest(self, labels, vectors=None, *, where=None, assign_attr=-1):
        self._centroid_args(labels, vectors, assign_attr, where, "assign_nearest")
        return super().assign_nearest(labels, vectors, where=where, assign_attr=assign_attr)

    def kmeans(self, labels, vectors=None, *, max_iterations=25, where=None, assign_attr=-1):
        if max_iterations < 1:
            raise Refused("kmeans: max_iterations < 1")
        self._centroid_args(labels, vectors, assign_attr, where, "kmeans")
        if max_iterations > N.CLUSTER_MAX_ITERATIONS or self.space == "ip":
            raise Unsupported("kmeans: max_iterations above the limit, or an ip index")
        return super().kmeans(labels, vectors, max_iterations=max_iterations, where=where, assign_attr=assign_attr)

    # -- bit codes: range search and the join
    def _bits_args(self, attr, words, metric, radius, capacity, where, what):
        self._bits_col(attr, what, words)
        if metric not in METRICS or radius != radius or capacity < 1:
            raise Refused(f"{what}: a known metric, a radius that is a number, capacity >= 1")
        self._program(where)
        if capacity > MAX_HITS:
            raise Unsupported(f"{what}: capacity above MLVDB_BITS_RANGE_MAX_HITS")

    def range_bits(self, attr, queries, radius, metric="hamming", capacity=MAX_HITS, where=None, count_only=False):
        self._bits_args(attr, np.asarray(queries).shape[1], metric, radius, capacity, where, "range_bits")
        return super().range_bits(attr, queries, radius, metric, capacity, where, count_only)

    def join_within_bits(self, attr, labels, mode, radius, capacity=MAX_HITS, metric="hamming", where=None, words=None):
        """The rule of tests/test_gpu_bits_join.py: ``range_bits`` for the stored code of every left row that is live and holds a
        code of ``words`` words (any other label has no partners), the row itself or every label <= it dropped, THEN the
        capacity: a row with more partners than that keeps its exact count and an empty segment."""
        left = np.asarray(labels, np.int64)
        if mode not in JOIN_MODES or (np.diff(left) <= 0).any():
            raise Refused("join_within_bits: a known mode, labels that ascend strictly")
        self._stored(left, "join_within_bits", 0)
        self._bits_args(attr, words, metric, radius, capacity, where, "join_within_bits")
        holds = self.candidates(attr, None, words)
        asked = [int(a) for a in left.tolist() if holds[a]]
        codes = np.array([self._lists[attr][a] for a in asked], dtype=np.uint64).reshape(len(asked), words)
        ref = {}
        if asked:
            cand = self.candidates(attr, where, words)
            idx = np.flatnonzero(cand)
            from tests.bits_helpers import distances

            rows = np.array([self._lists[attr][i] for i in idx.tolist()], dtype=np.uint64).reshape(idx.size, words)
            dist = distances(codes, rows, metric) if idx.size else np.zeros((len(asked), 0))
            for i, a in enumerate(asked):
                hit = np.flatnonzero(dist[i] <= radius)
                order = hit[np.lexsort((idx[hit], dist[i, hit]))]
                ref[a] = (idx[order], dist[i, order])
        none = (np.zeros(0, np.int64), np.zeros(0))
        out_l, out_d, counts = [], [], np.zeros(left.size, np.int64)
        for i, a in enumerate(left.tolist()):
            lab, d = ref.get(a, none)
            keep = (lab > a) if mode == LATER else (lab != a)
            counts[i] = keep.sum()
            if counts[i] <= capacity:
                out_l.append(lab[keep])
                out_d.append(d[keep])
        offsets = np.concatenate([[0], np.cumsum(np.where(counts <= capacity, counts, 0))]).astype(np.int64)
        d64 = np.concatenate(out_d + [none[1]])
        return RangeHits(np.concatenate(out_l + [none[0]]).astype(np.int64), d64.astype(np.float32), offsets), d64, counts


# ---------------------------------------------------------------- ops: arrays, calls
def _centroids(model, op, rng):
    """(labels int64 [m], vectors float32 [m, d]): stored and raw centroids mixed; ``near``: raw centroids next to stored rows."""
    total, m = model._rows.shape[0], op["m"]
    vectors = rng.standard_normal((m, model.dim)).astype(np.float32)
    if not total:
        return np.full(m, -1, np.int64), vectors
    pool = np.flatnonzero(~model._deleted) if op.get("pool") == "live" and (~model._deleted).any() else np.arange(total)
    labels = rng.choice(pool, m, replace=pool.size < m).astype(np.int64)
    raw = rng.random(m) < op.get("raw_share", 0.3)
    raw[0] = False
    vectors[raw] = (model._rows[labels[raw]] + 0.25 * vectors[raw]).astype(np.float32)
    labels[raw] = -1
    if op.get("far") and model.space == "cosine":  # a copy of centroid 0: every tie goes to the lower j, it has no member
        labels[-1] = labels[0]
    elif op.get("far"):  # far from every row: a cluster without members, which keeps its centroid
        vectors[-1] = 1.0e3
        labels[-1] = -1
    return labels, vectors


def materialise(model, op):
    """``history_recent_helpers.materialise`` + the arrays of the new kinds, and the state of the model that the comparison of
    a scored, by-example or clustering answer reads (copies: the state BEFORE the op)."""
    a = R.materialise(model, op)
    kind = op["op"]
    total = model._rows.shape[0]
    rng = np.random.default_rng(op["seed"]) if "seed" in op else None
    where = a.get("program")
    if kind == "search_scored":
        a["score"] = score_of(op["score"])
        a.update(cols={x: model._cols[x].copy() for _, x, _ in [o for o in op["score"]["ops"] if o[0] == S.ATTR]},
                 masks=[model.match(c) for c in a["score"].conds], live=model._mask(where).copy())
    elif kind == "search_examples":
        pool = {"all": None, "live": np.flatnonzero(~model._deleted), "dead": np.flatnonzero(model._deleted)}[op["pool"]]
        if pool is not None and pool.size == 0:
            pool = None
        bags = random_bags(rng, op["mode"], op["sizes"], total, model.dim, raw_share=op["raw_share"], pool=pool)
        a.update(zip(("labels", "vectors", "roles", "offsets"), bags), rows=model._rows, live=model._mask(where).copy())
    elif kind == "join_within":
        a["labels"] = left_labels(model, op, rng)
    elif kind in ("range_bits",):
        a["bq"] = R.bits_codes(rng, op["nbq"], op["words"])
    elif kind == "join_within_bits":
        a["labels"] = left_labels(model, op, rng)
    elif kind in ("assign_nearest", "kmeans") + WRITERS:
        a["labels"], a["vectors"] = _centroids(model, op, rng)
        a.update(rows=model._rows, live=model._mask(where).copy(), space=model.space)
    elif kind == "refuse_latest":
        a["qs"] = rng.standard_normal((2, model.dim), dtype=np.float32)
        a["bq"] = R.bits_codes(rng, 2, R.WORDS)
    return a


def left_labels(model, op, rng):
    """The left rows of a join: ``n_left`` distinct labels, ascending; ``left`` says which rows they are drawn from."""
    total = model._rows.shape[0]
    if "labels" in op:
        return np.array(op["labels"], np.int64)
    pool = np.arange(total)
    if op.get("left") == "dead" and model._deleted.any():
        dead, live = np.flatnonzero(model._deleted), np.flatnonzero(~model._deleted)
        pool = np.concatenate([dead[:max(1, op["n_left"] // 2)], live])
    return np.sort(rng.choice(pool, min(op["n_left"], pool.size), replace=False)).astype(np.int64)


def _cluster_call(e, op, a):
    attr = op["assign_attr"]
    if op["op"] in ("assign_nearest", "assign_write"):
        return e.assign_nearest(a["labels"], a["vectors"], where=a.get("program"), assign_attr=attr)
    return e.kmeans(a["labels"], a["vectors"], max_iterations=op["max_iterations"], where=a.get("program"), assign_attr=attr)


def _refusal(e, op, a):
    """The call of a LATEST_REFUSALS op -> ("refused", status) when it ends in a ``RuntimeError``, else ("accepted",).  Every
    call breaks ONE rule of its header."""
    which, qs, bq = op["which"], a["qs"], a["bq"]
    d = qs.shape[1]
    dist = score_of({"ops": [[S.DIST, 0, 0]], "conds": []})
    one = lambda x, dtype=np.int64: np.array(x, dtype)  # noqa: E731
    bag = lambda labels, roles, vectors=None: (one(labels), vectors, one(roles, np.int32), one([0, len(labels)]))  # noqa: E731
    raw = np.ones((3, d), np.float32)
    try:
        if which == "scored_k0":
            e.search_scored(qs, 0, dist)
        elif which == "scored_k65":
            e.search_scored(qs, MAX_TOPK + 1, dist)
        elif which == "scored_no_ops":
            e.search_scored(qs, 5, S.ScoreProgram(np.zeros(0, S.OP_DTYPE), []))
        elif which == "scored_underflow":
            e.search_scored(qs, 5, score_of({"ops": [[S.DIST, 0, 0], [S.ADD, 0, 0]], "conds": []}))
        elif which == "examples_k0":
            e.search_examples(BEST, *bag([0], [POS]), 0)
        elif which == "examples_k65":
            e.search_examples(BEST, *bag([0], [POS]), MAX_TOPK + 1)
        elif which == "examples_bag65":
            e.search_examples(BEST, *bag([0] * (N.EXAMPLES_MAX + 1), [POS] * (N.EXAMPLES_MAX + 1)), 5)
        elif which == "examples_empty_bag":
            e.search_examples(BEST, one([0]), None, one([POS], np.int32), one([0, 0, 1]), 5)
        elif which == "examples_label":
            e.search_examples(BEST, *bag([op["total"]], [POS]), 5)
        elif which == "examples_roles":
            e.search_examples(DISCOVER, *bag([0, 1, 2], [POS, POS, NEG]), 5)
        elif which == "examples_nan":
            e.search_examples(BEST, *bag([-1, 0, 1], [POS, POS, NEG], raw * np.float32("nan")), 5)
        elif which == "examples_mode":
            e.search_examples(17, *bag([0], [POS]), 5)
        elif which == "join_unsorted":
            e.join_within(one([1, 1]), OTHERS, 1.0, 8, None, True)
        elif which == "join_label":
            e.join_within(one([0, op["total"]]), OTHERS, 1.0, 8, None, True)
        elif which == "join_mode":
            e.join_within(one([0, 1]), 9, 1.0, 8, None, True)
        elif which in ("join_capacity0", "join_capacity_max"):
            capacity = 0 if which == "join_capacity0" else N.JOIN_MAX_CAPACITY + 1
            if hasattr(e, "_lib"):  # (the wrapper clamps the capacity: the C entry is asked, room for 16 hits, nothing written)
                rc = native_join(e, one([0, 1]), OTHERS, 1.0, capacity, 16)[0]
                return ("accepted",) if rc == N.OK else ("refused", int(rc))
            e.join_within(one([0, 1]), OTHERS, 1.0, capacity, None, True)
        elif which == "cluster_m0":
            e.assign_nearest(one([]), None)
        elif which == "cluster_m_max":
            e.assign_nearest(np.zeros(N.CLUSTER_MAX + 1, np.int64), None)
        elif which == "cluster_label":
            e.assign_nearest(one([0, op["total"]]), None)
        elif which == "cluster_attr_float":
            e.assign_nearest(one([0, 1]), None, assign_attr=1)
        elif which == "cluster_attr_undefined":
            e.assign_nearest(one([0, 1]), None, assign_attr=40)
        elif which == "cluster_nan":
            e.assign_nearest(one([0, -1, 1]), raw * np.float32("inf"))
        elif which == "cluster_iter0":
            e.kmeans(one([0, 1]), None, max_iterations=0)
        elif which == "cluster_iter_max":
            e.kmeans(one([0, 1]), None, max_iterations=N.CLUSTER_MAX_ITERATIONS + 1)
        elif which == "kmeans_ip":
            e.kmeans(one([0, 1]), None, max_iterations=2, assign_attr=CLUSTER_A)
        elif which == "bits_range_capacity0":
            e.range_bits(R.BITS_A, bq, 3.0, "hamming", 0)
        elif which == "bits_range_capacity_max":
            e.range_bits(R.BITS_A, bq, 3.0, "hamming", MAX_HITS + 1)
        elif which == "bits_range_nan":
            e.range_bits(R.BITS_A, bq, float("nan"))
        elif which == "bits_range_not_bits":
            e.range_bits(2, bq, 3.0)
        elif which == "bits_range_words0":
            e.range_bits(R.BITS_A, bq[:, :0], 3.0)
        elif which == "bits_join_unsorted":
            e.join_within_bits(R.BITS_A, one([1, 0]), OTHERS, 3.0, words=R.WORDS)
        elif which == "bits_join_label":
            e.join_within_bits(R.BITS_A, one([0, op["total"]]), OTHERS, 3.0, words=R.WORDS)
        elif which == "bits_join_words0":
            e.join_within_bits(R.BITS_A, one([0, 1]), OTHERS, 3.0, words=0)
        elif which == "bits_join_capacity_max":
            e.join_within_bits(R.BITS_A, one([0, 1]), OTHERS, 3.0, MAX_HITS + 1, words=R.WORDS)
        elif which == "bits_join_nan":
            e.join_within_bits(R.BITS_A, one([0, 1]), OTHERS, float("nan"), words=R.WORDS)
        elif which == "bits_join_mode":
            e.join_within_bits(R.BITS_A, one([0, 1]), 9, 3.0, words=R.WORDS)
        elif which == "bits_join_not_bits":
            e.join_within_bits(2, one([0, 1]), OTHERS, 3.0, words=R.WORDS)
        else:
            raise ValueError(which)
    except RuntimeError as err:
        return ("refused", H._status_of(err))
    return ("accepted",)


CALLS = {
    "search_scored": lambda e, op, a: e.search_scored(a["qs"], op["k"], a["score"], a.get("program"), want64=True),
    "search_examples": lambda e, op, a: e.search_examples(op["mode"], a["labels"], a["vectors"], a["roles"], a["offsets"], op["k"],
                                                          exclude=op["exclude"], where=a.get("program")),
    "join_within": lambda e, op, a: e.join_within(a["labels"], op["mode"], op["radius"], op["capacity"], a.get("program"), op["truncate"]),
    "range_bits": lambda e, op, a: e.range_bits(op["attr"], a["bq"], op["radius"], op["metric"], op["capacity"], a.get("program"),
                                                op["count_only"]),
    "join_within_bits": lambda e, op, a: e.join_within_bits(op["attr"], a["labels"], op["mode"], op["radius"], op["capacity"],
                                                            op["metric"], a.get("program"), op["words"]),
    "assign_nearest": _cluster_call, "kmeans": _cluster_call, "assign_write": _cluster_call, "kmeans_write": _cluster_call,
    "refuse_latest": _refusal,
}


# ---------------------------------------------------------------- comparison of one answer
def _all_pairs(e, vectors, n):
    """float64 [m, n]: the engine's own ``pair_distances`` of every vector to every stored row."""
    vectors = np.ascontiguousarray(vectors, np.float32)
    if not n or not vectors.shape[0]:
        return np.zeros((vectors.shape[0], n))
    return e.pair_distances(vectors, np.ascontiguousarray(np.broadcast_to(np.arange(n, dtype=np.int64), (vectors.shape[0], n))))[0]


def _packed(got, want, tag):
    """(RangeHits, dist64, counts) of the two bit-code entries: every bit."""
    _same(got[2], want[2], tag, "counts")
    _same(got[0].offsets, want[0].offsets, tag, "offsets")
    _same(got[0].labels, want[0].labels, tag, "labels")
    _same(got[1], want[1], tag, "dist64")
    _same(got[0].dist, want[0].dist, tag, "dist32")


def compare(e, op, a, got, want, tag, stats):
    """One branch per new kind, by that family's own committed rule."""
    kind = op["op"]
    n = a["rows"].shape[0] if "rows" in a else None
    if kind == "search_scored":
        n = a["live"].size
        D = _all_pairs(e, a["qs"], n)
        own = scored_topk(score_eval(a["score"], D, a["cols"], a["masks"]), op["k"], a["live"], D)
        for name, g, w in zip(("labels", "scores", "counts", "dist64"), got, own):
            _same(g, w, tag, f"{name} against the model on the engine's own distances")
        _same(got[2], want[2], tag, "counts")
        H._max_err64(np.where(got[0] >= 0, got[3], np.inf), np.where(got[0] >= 0, _own_dist(a, got[0]), np.inf), tag, stats)
    elif kind == "search_examples":
        D = _all_pairs(e, example_vectors(a["rows"], a["labels"], a["vectors"]), n)
        own = model_search(op["mode"], D, a["labels"], a["roles"], a["offsets"], op["k"], a["live"], op["exclude"])
        for name, g, w in zip(("labels", "tiers", "values", "counts"), got, own):
            _same(g, w, tag, f"{name} against the model on the engine's own distances")
        _same(got[3], want[3], tag, "counts")
    elif kind == "join_within":
        hits, counts = got
        _same(counts, want[1], tag, "counts")
        _same(hits.offsets, want[0].offsets, tag, "offsets")
        assert_range_matches(hits, want[0], tag)
        end = int(want[0].offsets[-1])  # (the engine's arrays may be longer than the hits they hold)
        if end:  # what the bar of assert_range_matches is held against: recorded, the largest is printed
            w = want[0].dist[:end].astype(np.float64)
            dev = float(np.max(np.abs(hits.dist[:end].astype(np.float64) - w) / np.maximum(1.0, np.abs(w))))
            if dev > stats.get("join_dev", -1.0):
                stats["join_dev"] = dev
                print(f"{tag}: join distance deviation {dev:.3e}")
    elif kind == "range_bits":
        if op["count_only"]:
            _same(got, want, tag, "counts")
        else:
            _packed(got, want, tag)
    elif kind == "join_within_bits":
        _packed(got, want, tag)
    elif kind in ("assign_nearest", "assign_write", "kmeans", "kmeans_write"):
        c0 = centroid_vectors(a["rows"], a["labels"], a["vectors"])
        dist = lambda c: _all_pairs(e, c, n)  # noqa: E731
        if kind.startswith("assign"):
            assign, best = model_assign(dist(c0), a["live"])
            own = model_sizes_costs(assign, best, c0.shape[0])
            sizes, costs, matched = got
            assert matched == want[2], f"{tag}: {matched} candidates, the model {want[2]}"
            _same(sizes, want[0], tag, "sizes")
        else:
            cent, sizes, costs, t, converged, matched = got
            own_c, own_sizes, own_costs, own_t, own_conv, _ = model_kmeans(dist, a["rows"], a["live"], c0, a["space"], op["max_iterations"])
            own = (own_sizes, own_costs)
            assert (t, converged, matched) == tuple(want[3:]), f"{tag}: (iterations, converged, candidates) {(t, converged, matched)}, the model {want[3:]}"
            assert (own_t, bool(own_conv)) == (t, converged), f"{tag}: the loop on the engine's own distances ends at {(own_t, own_conv)}"
            _same(cent, want[0], tag, "centroids")
            _same(cent, own_c, tag, "centroids against the loop on the engine's own distances")
            _same(sizes, want[1], tag, "sizes")
        _same(sizes, own[0], tag, "sizes against the model on the engine's own distances")
        _same(costs, own[1], tag, "costs against the model on the engine's own distances")
        if op["assign_attr"] >= 0:
            _same(e.get_attr(op["assign_attr"], 0, n), a["column_after"], tag, "the column read back")
    elif kind == "refuse_latest":
        assert tuple(got) == tuple(want), f"{tag}: {got}, the model {want}"
    else:
        raise ValueError(kind)


def _own_dist(a, labels):
    """The oracle's fp64 distance of every (query, returned label): what dist64 is held against by the suite's bar."""
    D = exact_scan.exact_distances(a["qs"], a["rows_now"], a["space"]) if a["rows_now"].shape[0] else np.zeros((a["qs"].shape[0], 0))
    return np.take_along_axis(D, np.maximum(labels, 0), axis=1) if D.shape[1] else np.full(labels.shape, np.inf)


# ---------------------------------------------------------------- generation
class _LatestGenerator(R._RecentGenerator):
    """The generator over LATEST_MUTATIONS / LATEST_QUERIES: the recent columns and 12 cluster, 13 late cluster (int64); the
    recent program pool and LATEST_PROGRAMS in every program-taking op; schedules of its own."""

    PROGRAMS = R._RecentGenerator.PROGRAMS + LATEST_PROGRAMS
    TAKES_PROGRAM = R._RecentGenerator.TAKES_PROGRAM + NEW_TAKING

    def __init__(self, seed, space, d, scale):
        assert scale in LATEST_SCALES
        super().__init__(seed, space, d, "recent_large" if scale == "latest_large" else "recent")
        self.rng = np.random.default_rng([seed, d, H.SPACES.index(space), 32 + LATEST_SCALES.index(scale)])
        self.model = LatestHistoryModel(d, space)
        self.defined13 = False
        self.last_kind = None  # the program kind of the program drawn last

    def _materialise(self, op):
        return materialise(self.model, op)

    def emit(self, op):
        kind = op["op"]
        want = super().emit(op)
        exp = self.expected[-1]
        if kind == "search_scored":  # (the rows as they are now: dist64 goes by the suite's bar against the oracle)
            exp["args"].update(rows_now=self.model._rows, space=self.model.space)
        if kind in WRITERS:
            exp["counts"] = self.model.counts()
        if kind in LATEST_NEW_QUERIES + WRITERS:  # (read by the coverage conditions: the rows that were tombstoned)
            exp["args"]["dead_mask"] = self.model._deleted.copy()
        if kind in ("assign_nearest", "kmeans") + WRITERS and op["assign_attr"] >= 0:
            exp["args"]["column_after"] = self.model._cols[op["assign_attr"]].copy()
        return want

    # -- programs
    def program(self, which=None):
        pool = self.PROGRAMS
        which = which or (pool[self.rng.integers(len(pool))] if not self.only_recent else None)
        self.last_kind = which
        if which == "cluster":
            return {"ops": [_leaf(W.EQ, CLUSTER_A, int(self.rng.integers(3)))], "set": []}
        if which == "cluster_absent":
            return {"ops": [_leaf(W.EXISTS, CLUSTER_A), _leaf(W.NOT, 0)], "set": []}
        return super().program(which)

    def _define(self):
        super()._define()
        self.emit({"op": "define_attr", "attr": CLUSTER_A, "kind": "int64"})

    # -- near-ties of the clustering calls, from the oracle alone
    def _cluster_ok(self, op):
        m = self.model
        a = materialise(m, op)
        if self.total < 1:
            return True
        c = centroid_vectors(m._rows, a["labels"], a["vectors"])
        live = a["live"]
        rounds = 1 if op["op"].startswith("assign") else op["max_iterations"]
        if not op["op"].startswith("assign") and m.space == "ip":
            return True
        prev = None
        for t in range(1, rounds + 1):
            D = exact_scan.exact_distances(c, m._rows, m.space)[:, live]
            if D.shape[0] > 1 and D.shape[1]:
                two = np.sort(D, axis=0)[:2]
                gap = two[1] - two[0]
                if ((gap > 0) & (gap <= TIE_REL * np.maximum(1.0, np.abs(two[1])))).any():
                    return False
            assign, _ = model_assign(exact_scan.exact_distances(c, m._rows, m.space), live)
            c = model_means(m._rows, assign, c.shape[0], m.space, c)
            if t >= 2 and np.array_equal(assign, prev):
                break
            prev = assign
        return True

    def _join_ok(self, op):
        m = self.model
        left = left_labels(m, op, np.random.default_rng(op["seed"]))
        if not left.size or self.total < 2:
            return True
        D = exact_scan.exact_distances(m._rows[left], m._rows, m.space)
        r = float(np.float32(op["radius"]))
        if (np.abs(D - r) <= TIE_REL * max(1.0, abs(r))).any():
            return False
        return all(_gaps_ok(np.sort(D[i][D[i] <= r])) for i in range(left.size))

    def _join_radius(self, n_left, seed, left):
        """The float32 midpoint between two consecutive distances of one left row to the others: a few partners per row."""
        m = self.model
        labels = left_labels(m, {"n_left": n_left, "left": left}, np.random.default_rng(seed))
        if not labels.size or self.total < 3:
            return 1.0
        j = int(self.rng.integers(labels.size))
        s = np.sort(exact_scan.exact_distances(m._rows[labels[j:j + 1]], m._rows, m.space)[0])
        at = min(int(self.rng.choice([1, 2, 4, 12])), s.size - 2)
        return float(np.float32((s[at] + s[at + 1]) / 2))

    # -- the two new mutations
    def cluster(self, kind, program="random", **kw):
        rng = self.rng
        writes = kind in WRITERS
        if program == "random":
            program = self.program() if rng.random() < 0.5 else None
        if kind.startswith("kmeans") and self.model.space == "ip":
            return self.refuse("kmeans_ip")
        attr = kw.pop("assign_attr", CLUSTER_A if writes else -1)
        m = int(kw.pop("m", (1, 3, 5)[rng.integers(3)]))
        op = {"op": kind, "m": m, "assign_attr": int(attr), "max_iterations": int(kw.pop("max_iterations", (1, 2, 4)[rng.integers(3)])),
              "raw_share": 0.3, "pool": kw.pop("pool", ("all", "live")[rng.integers(2)]), "program": program,
              "program_kind": self.last_kind if program is not None else None, **kw}
        return self._draw(lambda: {**op, "seed": self._seed()}, self._cluster_ok)

    def mutate(self, kind):
        if kind in WRITERS:
            return self.cluster(kind)
        return super().mutate(kind)

    # -- queries
    def score(self, which=None):
        which = which or SCORES[self.rng.integers(len(SCORES))]
        c = W.float_bits
        if which == "dist_attr":      # distance + 0.01 * tenant
            ops, conds = [[S.DIST, 0, 0], [S.ATTR, 2, c(0.0)], [S.CONST, 0, c(0.01)], [S.MUL, 0, 0], [S.ADD, 0, 0]], []
        elif which == "dist_float":   # distance * |score| (absent: 1); the hostile floats make NaN and inf scores
            ops, conds = [[S.DIST, 0, 0], [S.ATTR, 1, c(1.0)], [S.ABS, 0, 0], [S.MUL, 0, 0]], []
        elif which == "match":        # distance - 0.5 for the rows two conds match: the conds' set table
            ops = [[S.DIST, 0, 0], [S.MATCH, 0, 0], [S.MATCH, 0, 1], [S.ADD, 0, 0], [S.CONST, 0, c(0.5)], [S.MUL, 0, 0], [S.SUB, 0, 0]]
            conds = [self.program("groups"), self.program(("half", "has_any", "cluster")[self.rng.integers(3)])]
        elif which == "cluster_operand":  # distance + the cluster column (absent: NaN -> the row is dropped)
            ops, conds = [[S.DIST, 0, 0], [S.ATTR, CLUSTER_A, c(float("nan"))], [S.ADD, 0, 0]], []
        else:                         # min(distance, |group| / 8)
            ops, conds = [[S.DIST, 0, 0], [S.ATTR, 0, c(3.0)], [S.ABS, 0, 0], [S.CONST, 0, c(8.0)], [S.DIV, 0, 0], [S.MIN, 0, 0]], []
        return {"ops": ops, "conds": [{k: v for k, v in p.items() if k != "radii"} for p in conds], "which": which}

    def query(self, kind, **kw):
        rng, total = self.rng, self.total
        if kind not in LATEST_NEW_QUERIES:
            return super().query(kind, **kw)
        if kind in ("assign_nearest", "kmeans"):
            return self.cluster(kind, **kw)
        program = kw.pop("program", "random")
        if program == "random":
            program = self.program() if rng.random() < 0.5 else None
        tagged = {"program": program, "program_kind": self.last_kind if program is not None else None}
        if kind == "search_scored":
            return self.emit({"op": kind, "nq": int(kw.pop("nq", (1, 3, 9)[rng.integers(3)])), "k": int(kw.pop("k", (1, 10, 64)[rng.integers(3)])),
                              "seed": self._seed(), "score": self.score(kw.pop("score", None)), **tagged})
        if kind == "search_examples":
            sizes = kw.pop("sizes", None) or [int(x) for x in rng.choice([1, 2, 3, 9, 17, 33], int((1, 3, 5)[rng.integers(3)]))]
            return self.emit({"op": kind, "mode": int(kw.pop("mode", MODES[rng.integers(3)])), "sizes": sizes,
                              "k": int((1, 10, 64)[rng.integers(3)]), "exclude": bool(kw.pop("exclude", rng.random() < 0.7)),
                              "pool": kw.pop("pool", ("all", "live", "dead")[rng.integers(3)]),
                              "raw_share": float(kw.pop("raw_share", (0.0, 0.3)[rng.integers(2)])), "seed": self._seed(), **tagged})
        if kind == "join_within":
            n_left = int(kw.pop("n_left", (1, 5, 12, 40)[rng.integers(4)]))
            left = kw.pop("left", ("any", "dead")[rng.integers(2)])
            capacity, truncate = kw.pop("cut", None) or ((64, False), (64, True), (2, True), (2, False))[rng.integers(4)]
            mode = int(kw.pop("mode", JOIN_MODES[rng.integers(2)]))

            def make():
                seed = self._seed()
                return {"op": kind, "n_left": n_left, "left": left, "mode": mode, "capacity": capacity, "truncate": truncate,
                        "seed": seed, "radius": self._join_radius(n_left, seed, left), **tagged}
            return self._draw(make, self._join_ok)
        words = int(kw.pop("words", (R.WORDS, R.WORDS, R.WORDS_FEW)[rng.integers(3)]))
        metric = kw.pop("metric", METRICS[rng.integers(2)])
        frac = float(kw.pop("frac", (0.0, 0.42, 0.47, 1.0)[rng.integers(4)]))
        radius = frac * 64 * words if metric == "hamming" else (0.0, 0.6, 0.64, 1.0)[(0.0, 0.42, 0.47, 1.0).index(frac)]
        capacity = int(kw.pop("capacity", (MAX_HITS, MAX_HITS, 3)[rng.integers(3)]))
        attr = kw.pop("attr", R.BITS_A)
        if kind == "range_bits":
            return self.emit({"op": kind, "attr": attr, "nbq": int((1, 3, 9)[rng.integers(3)]), "words": words, "metric": metric,
                              "radius": float(radius), "capacity": capacity, "count_only": bool(kw.pop("count_only", rng.random() < 0.3)),
                              "seed": self._seed(), **tagged})
        if kind == "join_within_bits":
            return self.emit({"op": kind, "attr": attr, "n_left": int(kw.pop("n_left", (1, 7, 40)[rng.integers(3)])),
                              "left": ("any", "dead")[rng.integers(2)], "mode": int(JOIN_MODES[rng.integers(2)]), "words": words,
                              "metric": metric, "radius": float(radius if frac < 1.0 else 0.44 * 64 * words if metric == "hamming" else 0.62),
                              "capacity": capacity, "seed": self._seed(), **tagged})
        raise ValueError(kind)

    def refuse(self, which, **extra):
        if which not in LATEST_REFUSALS:
            return super().refuse(which, **extra)
        return self.emit({"op": "refuse_latest", "which": which, "seed": self._seed(), "total": self.total})

    def _ask_latest(self):
        """The seven new queries without a program (kmeans: assign_nearest again on an ip index)."""
        for kind in LATEST_NEW_QUERIES:
            if kind == "kmeans" and self.model.space == "ip":
                kind = "assign_nearest"
            self.query(kind, program=None)

    # -- the schedules
    def latest(self):
        rng, seed = self.rng, self.seed
        euclid = self.model.space != "ip"
        rank = (seed - LATEST[0][0]) % len(LATEST)  # the committed seeds: their position in LATEST
        others = [i for i, key in enumerate(LATEST) if key[1] != "ip"]
        nth = others.index(rank) if rank in others else rank % 8
        self._define()
        self.append("hundreds")
        self.set_attrs()
        pairs = PAIRS_ANY[rank::len(LATEST)] + (PAIRS_KMEANS[nth::8] if euclid else [])
        def rows_for(*kinds):  # k-means is refused on an ip index: its pairs and programs run in another space
            if self.model.space == "ip" and set(kinds) & set(KMEANS_KINDS):
                self.reset_to("l2")
            self.ensure_rows()

        items = [lambda m=m, q=q: (rows_for(m, q), self.mutate(m), self.query(q)) for m, q in pairs]
        takers = [(k, p) for k in NEW_TAKING for p in self.PROGRAMS]
        mine = [c for c in takers if not c[0].startswith("kmeans")][rank::len(LATEST)] + \
            ([c for c in takers if c[0].startswith("kmeans")][nth::8] if euclid else [])

        def with_program(kind, which):  # every program kind in every new entry
            rows_for(kind)
            p = self.program(which)
            self.cluster(kind, program=p) if kind in WRITERS else self.query(kind, program=p)

        def readers(writer):  # clustering writes the column; each reader of it follows at once
            self.ensure_rows()
            writer = writer if self.model.space != "ip" else "assign_write"
            leaf = {"ops": [_leaf(W.EQ, CLUSTER_A, 0)], "set": []}
            for reader in ("filter", "facet_values", "attr_stats", "search_distinct", "search_grouped", "where_ordered", "search_scored",
                           "cluster"):
                self.cluster(writer, program=None, m=3, max_iterations=2)
                if reader == "filter":
                    self.query("where_count", program=leaf)
                elif reader == "facet_values":
                    self.query("facet_values", attr=CLUSTER_A)
                elif reader == "attr_stats":
                    self.query("attr_stats", attr=1, by=CLUSTER_A, max_groups=16, program=None)
                elif reader == "search_scored":
                    self.query("search_scored", score="cluster_operand", program=None)
                elif reader == "cluster":  # the `where` reads the column the call writes: evaluated once, before any write
                    self.cluster(writer, program=leaf, m=2, max_iterations=2)
                    self.emit({"op": "get_attr", "attr": CLUSTER_A, "float": False, "first": 0, "n": self.total})
                else:
                    self.query(reader, attr=CLUSTER_A)

        def untouched():  # a filter and tombstones: the rows that are no candidates keep what they held
            self.ensure_rows()
            self.tombstone("frac")
            self.emit({"op": "set_attr", "attr": CLUSTER_A, "first": 0, "n": self.total, "seed": self._seed()})
            self.cluster("assign_write", program=self.program("half"), m=3)
            self.emit({"op": "get_attr", "attr": CLUSTER_A, "float": False, "first": 0, "n": self.total})
            self.cluster("assign_write", program=None, m=2, far=True, raw_share=0.0)
            self.query("facet_values", attr=CLUSTER_A)

        def emptied_cluster():  # a cluster that loses all its members keeps its centroid
            if self.model.space == "ip":
                return
            self.ensure_rows()
            self.cluster("kmeans_write", program=None, m=3, far=True, max_iterations=1 if self.model.space == "cosine" else 3)
            assert self.expected[-1]["want"][1][-1] == 0, "the far centroid has members"
            self.emit({"op": "get_attr", "attr": CLUSTER_A, "float": False, "first": 0, "n": self.total})

        def workspace_shapes():  # cosine k-means (28 B per row) directly after l2-shaped use (20 B), and the reverse
            self.ensure_rows()
            other = "cosine" if self.model.space != "cosine" else "l2"
            for space in (other, self.model.space if euclid else "l2"):
                self.cluster("assign_write", program=None, m=3)
                if self.model.space != "ip":
                    self.cluster("kmeans", program=None, m=3, max_iterations=2)
                self.reset_to(space)
                self.append("hundreds")
                self.cluster("kmeans_write", program=None, m=3, max_iterations=2, assign_attr=CLUSTER_A)
                self.emit({"op": "get_attr", "attr": CLUSTER_A, "float": False, "first": 0, "n": self.total})
            self.set_attrs()

        def cluster_regrowth():  # cl_ws grows only: after a row regrowth, and after a compaction that shrinks the corpus
            self.ensure_rows()
            self.cluster("assign_write", program=None, m=3)
            self.append("cross")
            self.set_attrs()
            self.cluster("assign_write", program=None, m=5)
            self.query("facet_values", attr=CLUSTER_A)
            self.tombstone("frac")
            self.compact()
            self.cluster("kmeans_write" if self.model.space != "ip" else "assign_write", program=None, m=3, max_iterations=2)
            self.query("facet_values", attr=CLUSTER_A)

        def late_cluster():  # a cluster column defined after rows exist
            self.ensure_rows()
            self.emit({"op": "define_attr", "attr": LATE_CLUSTER, "kind": "int64"})
            self.defined13 = True
            self.query("facet_values", attr=LATE_CLUSTER)
            self.cluster("assign_write", program=self.program("half"), m=3, assign_attr=LATE_CLUSTER)
            self.query("facet_values", attr=LATE_CLUSTER)
            self.emit({"op": "get_attr", "attr": LATE_CLUSTER, "float": False, "first": 0, "n": self.total})

        def join_and_range():  # labels_in is shared with plain range search; the shadows are built lazily
            self.ensure_rows()
            self.query("join_within", program=None)
            self.query("range")
            self.query("join_within", program=None)
            self.query("range_each")
            self.query("join_within", program=None)
            self.query("join_within", cut=(2, True), n_left=12, program=None)   # a cut join, then a complete one
            self.query("join_within", cut=(64, False), n_left=12, program=None)

        def across(x):  # the join and the by-example search before and after each mutation
            self.ensure_rows()
            self.query("join_within", program=None, left="any")
            self.query("search_examples", program=None)
            if x == "regrowth":
                self.append("cross")
            elif x == "compact":
                self.tombstone("few")
                self.compact()
            else:
                {"tombstone_where": self.tombstone_where, "tombstone": self.tombstone, "append": self.append}[x]()
            self.query("join_within", program=None, left="dead")
            self.query("search_examples", program=None, pool="dead" if x.startswith("tombstone") else "all")

        def renumbered():  # tombstoned left / example labels, then the labels a compaction has renumbered
            self.ensure_rows()
            dead = sorted(int(x) for x in rng.choice(self.live[:self.live.size // 2], 5, replace=False))
            self.emit({"op": "tombstone", "mode": "labels", "labels": dead})
            self.query("search_examples", pool="dead", raw_share=0.0, program=None, exclude=True)
            self.query("join_within", left="dead", program=None)
            self.query("join_within_bits", program=None)
            self.compact()
            self.query("search_examples", pool="all", raw_share=0.0, program=None, exclude=True, sizes=[3, 17])
            self.query("join_within", program=None)
            self.query("join_within_bits", program=None)

        def bits_garbage():  # the bits pool compacted with garbage in it
            self.ensure_rows()
            for _ in range(2):
                self.bits_set_at(R.BITS_A, n=max(1, self.live.size // 2))
            self.tombstone("frac")
            self.compact()
            self.query("range_bits", words=R.WORDS, program=None)
            self.query("join_within_bits", words=R.WORDS, program=None)

        def bits_doubling():  # the bits pool regrows twice under live codes
            self.ensure_rows(300)
            self.compact()
            lo = self.total // 2
            cap, grown = self.model._pool_cap[R.BITS_A], 0
            for _ in range(16):
                used = self.model._pool_used[R.BITS_A]
                self.bits_set_at(R.BITS_A, n=self.total - lo, lo=lo)
                if self.model._pool_cap[R.BITS_A] != cap and used > 0:
                    cap, grown = self.model._pool_cap[R.BITS_A], grown + 1
                if grown >= 2:
                    break
            assert grown >= 2
            self.query("range_bits", words=R.WORDS, program=None)
            self.query("join_within_bits", words=R.WORDS, program=None)

        def bits_width(p_absent):  # rows rewritten at the other width, or made absent
            self.ensure_rows()
            rows = self.model._lists[R.BITS_A]
            five = [int(i) for i in self.live if rows[i] is not None and len(rows[i]) == R.WORDS]
            if len(five) < 40:
                self.set_bits(R.BITS_A, 0)
                rows = self.model._lists[R.BITS_A]
                five = [int(i) for i in self.live if rows[i] is not None and len(rows[i]) == R.WORDS]
            labels = sorted(int(x) for x in rng.choice(five, min(40, len(five)), replace=False))
            self.bits_set_at(R.BITS_A, words=R.WORDS_FEW, p_absent=p_absent, labels=labels, n=len(labels))
            for words in (R.WORDS, R.WORDS_FEW):
                self.query("range_bits", words=words, frac=0.47, program=None, count_only=False)
                self.emit({"op": "join_within_bits", "attr": R.BITS_A, "labels": labels, "mode": int(OTHERS), "words": words,
                           "metric": "hamming", "radius": 0.47 * 64 * words, "capacity": MAX_HITS, "program": None, "program_kind": None})

        def bits_late():  # a bits column defined late: all absent, then written
            self.ensure_rows()
            if not self.defined10:
                self.emit({"op": "define_attr", "attr": R.LATE_BITS, "kind": "bits"})
            for phase in range(2):
                self.query("range_bits", attr=R.LATE_BITS, words=R.WORDS, program=None)
                self.query("join_within_bits", attr=R.LATE_BITS, words=R.WORDS, program=None)
                if phase == 0:
                    self.set_bits(R.LATE_BITS, 0)

        def empty(how):  # emptied: every new entry answers padding or zeros; rows again; their values; asked again
            self.ensure_rows()
            if how == "compact":
                self.tombstone_where("true")
                self.compact()
            else:
                self.reset(how == "reset_other")
            euclid_now = self.model.space != "ip"
            self._ask_latest()
            self.append("hundreds")
            self._ask_latest()  # rows appended and the entries asked before any code or value is written
            self.set_attrs()
            self._ask_latest()
            assert euclid_now == (self.model.space != "ip")

        def masked(kind):  # the mask is handed back: a plain search, and the same call without a program
            self.ensure_rows()
            ask = (lambda **kw: self.cluster(kind, **kw)) if kind in WRITERS else (lambda **kw: self.query(kind, **kw))
            for after in ("search64", kind):
                ask(program=self.program(("half", "cluster", "geo_and_scalar", "has")[rng.integers(4)]))
                self.query("search64") if after == "search64" else ask(program=None)

        def score_table():  # score_prog keeps the conds' set table between calls: a table, then a program without one
            self.ensure_rows()
            self.query("search_scored", score="match", program=self.program("groups"))
            self.query("search_scored", score="dist_attr", program=None)
            self.query("search_where", program=self.program("groups"))
            self.query("search_scored", score="match", program=None)

        def refusals():  # every refusal is followed at once by a query
            self.ensure_rows()
            for i, which in enumerate(LATEST_REFUSALS):
                if i % 2 == seed % 2 and which != "kmeans_ip":
                    self.refuse(which)
                    self.query(("search64", "search_scored", "join_within", "range_bits", "search_examples", "assign_nearest")[rng.integers(6)])
            if self.model.space == "ip":
                self.refuse("kmeans_ip")
                self.query("assign_nearest")

        xs = ("tombstone", "tombstone_where", "append", "compact", "regrowth")
        items += [lambda c=c: with_program(*c) for c in mine]
        items += [lambda: readers(WRITERS[seed % 2]), untouched, emptied_cluster, cluster_regrowth, late_cluster, join_and_range,
                  renumbered, bits_garbage, bits_doubling, lambda: bits_width(0.0 if seed % 2 == 0 else 1.0), bits_late,
                  lambda: empty(("reset", "reset_other", "compact")[rank % 3]), score_table, refusals]
        items += [lambda x=x: across(x) for x in (xs[rank % 5], xs[(rank + 2) % 5], xs[(rank + 3) % 5])]
        items += [lambda k=k: masked(k) for k in [t for t in NEW_TAKING if euclid or not t.startswith("kmeans")][rank % 3::3]]
        if rank % 3 == 0:
            items.append(workspace_shapes)
        items += [lambda: (self.ensure_rows(), self.query(LATEST_QUERIES[rng.integers(len(LATEST_QUERIES))])) for _ in range(4)]
        for i in rng.permutation(len(items)):
            items[i]()
        self.finish()

    def latest_large(self):
        """Appends of 12,000 rows until past 32,768 (`auto` moves the join's range machinery to the filter route at 12 and 40
        left rows), a ``tombstone_where`` of about a third of the rows through a geo box and a compaction back below, growth
        again.  Shapes the small scale cannot reach: several 4,096-row listing blocks, clusters of more than 256 members
        (several segments), 17 and 65 centroids (more than one centroid tile), and a join of 257 left rows: the native call takes them
        in waves of ``_native.JOIN_WAVE`` = 256, so the boundary is reachable with any corpus above 256 rows; it is asked here,
        past the threshold of `auto`."""
        self._define()
        euclid = self.model.space != "ip"
        lat, lon = self.centre
        grow = "kmeans_write" if euclid else "assign_write"

        def both_sides():
            self.query("join_within", n_left=12, cut=(64, False), program=None, left="any")
            self.query("join_within", n_left=40, cut=(2, True), program=self.program("half"), left="any")
            self.query("search_examples", sizes=[3, 17], program=None)
            self.query("search_scored", nq=3, k=10, score="match", program=None)

        self.append(n=12000)
        self.set_attrs()
        both_sides()
        self.cluster("assign_write", program=None, m=17)
        self.query("facet_values", attr=CLUSTER_A)
        for _ in range(2):
            self.append(n=12000)
            self.set_attrs()
        both_sides()
        self.cluster(grow, program=None, m=3, max_iterations=2)
        self.query("facet_values", attr=CLUSTER_A)
        self.cluster("assign_nearest", program=self.program("cluster"), m=65)
        self.query("range_bits", words=R.WORDS, frac=0.42, capacity=MAX_HITS, program=None, count_only=False)
        self.query("join_within_bits", words=R.WORDS, n_left=40, frac=0.42, capacity=MAX_HITS, program=None)
        sw, ne = R.GH.quantise([lat - 2.0, lat + 2.0], [lon - 2.0, lon])
        self.emit({"op": "tombstone_where", "program": {"ops": [_leaf(W.GEO_BOX, R.GEO_A, sw, ne)], "set": []}})
        self.query("join_within", n_left=12, cut=(64, False), program=None, left="dead")
        self.cluster("assign_write", program=None, m=5)
        self.emit({"op": "get_attr", "attr": CLUSTER_A, "float": False, "first": 0, "n": self.total})
        self.compact()
        assert self.total < H.FILTER_MIN_ROWS
        both_sides()
        self.cluster(grow, program=self.program("half"), m=5, max_iterations=2)
        self.append(n=12000)
        assert self.total > H.FILTER_MIN_ROWS
        self.set_attrs()
        both_sides()
        self.cluster("assign_write", program=self.program("cluster_absent"), m=17)
        self.query("attr_stats", attr=1, by=CLUSTER_A, max_groups=32, program=None)
        self.query("range_bits", words=R.WORDS_FEW, frac=0.42, capacity=3, program=self.program("radius"), count_only=True)
        self.query("join_within_bits", words=R.WORDS_FEW, n_left=7, frac=0.42, capacity=MAX_HITS, program=None)
        self.query("join_within", n_left=N.JOIN_WAVE + 1, cut=(2, True), program=None, left="any")  # two waves of left rows
        self.finish()


# The committed seed set: (seed, space, d, scale).
LATEST = [(700 + 2 * i + j, space, d, "latest") for i, (space, d) in
          enumerate([("l2", 20), ("cosine", 64), ("ip", 128), ("l2", 256), ("cosine", 100), ("ip", 48)]) for j in range(2)]
LATEST_LARGE = [(800 + i, space, 64, "latest_large") for i, space in enumerate(H.SPACES)]
