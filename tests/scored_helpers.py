"""Shared by the scored-kNN tests (include/mlvdb_score.h): the score program evaluated with NumPy, one ufunc per op on float64
arrays; the ranking by (score, label); a seeded random expression generator bounded by the program limits; and an oracle
engine with ``search_scored``."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import score as S
from mlvectordb_amd import where as W
from oracle import exact_scan
from tests.where_helpers import WhereOracleEngine, eval_program, random_filter

GAP_MIN = 1e-9      # the convention of tests/mmr_helpers.py: consecutive oracle scores closer than this are not asked for


def _f64(bits: int) -> np.float64:
    return np.array([bits], dtype=np.int64).view(np.float64)[0]


def score_eval(program: S.ScoreProgram, D, columns, cond_masks) -> np.ndarray:
    """float64 [nq, n]: the program's value for every (query, row).  ``D`` [nq, n]: the distances DIST pushes; ``columns``:
    attribute -> the column as the device holds it (int64 with INT64_MIN absent, float64 with NaN absent) [n];
    ``cond_masks``: bool [n] per cond.  Every op is one NumPy ufunc on float64 arrays -- IEEE binary64, round to nearest
    even, nothing contracted; MIN / MAX are written out with ``np.where`` exactly as the header defines them."""
    D = np.asarray(D, dtype=np.float64)
    nan = np.float64("nan")
    stack = []
    with np.errstate(all="ignore"):
        for op, attr, a in program.ops.tolist():
            if op == S.CONST:
                stack.append(np.full((1, D.shape[1]), _f64(a)))
            elif op == S.DIST:
                stack.append(D)
            elif op == S.ATTR:
                col = np.asarray(columns[attr])
                if col.dtype == np.int64:
                    v = np.where(col == W.INT64_ABSENT, _f64(a), col.astype(np.float64))
                else:
                    v = np.where(np.isnan(col), _f64(a), col.astype(np.float64))
                stack.append(v[None, :])
            elif op == S.MATCH:
                stack.append(np.where(np.asarray(cond_masks[a], dtype=bool), 1.0, 0.0)[None, :])
            elif op in (S.NEG, S.ABS):
                x = stack.pop()
                stack.append(np.negative(x) if op == S.NEG else np.fabs(x))
            else:
                y, x = stack.pop(), stack.pop()
                if op == S.ADD:
                    r = np.add(x, y)
                elif op == S.SUB:
                    r = np.subtract(x, y)
                elif op == S.MUL:
                    r = np.multiply(x, y)
                elif op == S.DIV:
                    r = np.divide(x, y)
                elif op == S.MIN:
                    r = np.where(x <= y, x, np.where(y < x, y, nan))
                else:
                    r = np.where(x >= y, x, np.where(y > x, y, nan))
                stack.append(r)
    assert len(stack) == 1
    return np.ascontiguousarray(np.broadcast_to(stack[0], D.shape))


def scored_topk(scores, k: int, live, D=None):
    """The ranking of mlvdb_score.h: per query the min(k, candidates) rows of ``live`` (bool [n]: live and matching the
    outer filter) whose score is no NaN, by a stable sort on the score -- so -0.0 == +0.0 and ties keep label order.
    Returns (labels int64 [nq, k] padded -1, scores float64 padded +inf, counts int32, dist64 [nq, k] from ``D`` padded
    +inf, or None without ``D``)."""
    scores = np.asarray(scores, dtype=np.float64)
    nq = scores.shape[0]
    labels = np.full((nq, k), -1, np.int64)
    out = np.full((nq, k), np.inf)
    d64 = None if D is None else np.full((nq, k), np.inf)
    counts = np.zeros(nq, np.int32)
    live = np.asarray(live, dtype=bool)
    for q in range(nq):
        idx = np.flatnonzero(live & ~np.isnan(scores[q]))
        pick = idx[np.argsort(scores[q, idx], kind="stable")][:k]
        counts[q] = pick.size
        labels[q, :pick.size] = pick
        out[q, :pick.size] = scores[q, pick]
        if D is not None:
            d64[q, :pick.size] = np.asarray(D)[q, pick]
    return labels, out, counts, d64


# ---------------------------------------------------------------- random expressions
NUMBERS = (0, 1, -1, 0.5, 2, -0.0, 0.2, 10, 2024, 1e-3, 3.5, -7, 1e300, float("inf"))
NUMERIC_ATTRS = ("year", "price", "in_stock")  # of tests/where_helpers.SCHEMA


def random_leaf(rng):
    r = rng.random()
    if r < 0.3:
        return "$distance"
    if r < 0.55:
        return NUMBERS[rng.integers(len(NUMBERS))]
    if r < 0.85:
        e = {"$attr": NUMERIC_ATTRS[rng.integers(len(NUMERIC_ATTRS))]}
        if rng.random() < 0.6:
            e["$default"] = NUMBERS[rng.integers(len(NUMBERS))]
        return e
    return {"$match": random_filter(rng)}


def random_expression(rng, depth=0):
    r = rng.random()
    if depth >= 4 or r < 0.25:
        return random_leaf(rng)
    if r < 0.55:
        op = ("$add", "$mul", "$min", "$max")[rng.integers(4)]
        return {op: [random_expression(rng, depth + 1) for _ in range(rng.integers(1, 4))]}
    if r < 0.85:
        op = ("$sub", "$div")[rng.integers(2)]
        return {op: [random_expression(rng, depth + 1), random_expression(rng, depth + 1)]}
    return {("$neg", "$abs")[rng.integers(2)]: random_expression(rng, depth + 1)}


def random_score(rng, schema, strings=None):
    """(expression, compiled program): a seeded random expression within the limits -- one the compiler refuses as too
    long, too deep or with too many filters is drawn again."""
    while True:
        e = random_expression(rng)
        try:
            return e, S.compile_score(e, schema, strings)
        except ValueError as err:
            assert "at most" in str(err), err


# ---------------------------------------------------------------- the oracle engine
class ScoredOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``search_scored`` as ``HipScanEngine`` declares it: ``exact_scan.exact_distances`` for
    DIST, the model above for the rest."""

    def search_scored(self, queries, k, program, where=None, want64=False):
        assert 1 <= k <= 64
        n = self._rows.shape[0]
        D = exact_scan.exact_distances(queries, self._rows, self.space)
        masks = [eval_program(c, self._cols, n) & ~self._deleted for c in program.conds]
        live = ~self._deleted if where is None else self.match(where)
        labels, scores, counts, d64 = scored_topk(score_eval(program, D, self._cols, masks), k, live, D)
        return (labels, scores, counts, d64) if want64 else (labels, scores, counts)
