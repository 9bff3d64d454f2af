"""Shared by the search-by-example tests (include/mlvdb_like.h): the query rule restated in NumPy, a host strip of a ranked
list, and an oracle engine with ``search_like``."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd.index import Index
from tests.where_helpers import WhereOracleEngine


def like_queries(rows, labels, weights, offsets, space: str, base=None):
    """The queries of mlvdb_like.h from the stored float32 ``rows``: per query ``acc = base`` (or 0), then
    ``acc = acc + t_j * x_j`` example by example in the order given -- one rounded float64 product and one rounded float64
    addition per column (NumPy's elementwise operators, no fma) -- with ``t_j = w_j`` (l2, ip) or the once-rounded
    ``w_j * (1 / (|x_j| + 1e-30))`` (cosine; the norm summed here by NumPy, in another order than the device's), and the
    result rounded to float32 once.  Returns (queries float32 [nq, d], float64 [nq, d] of sum_j |t_j * x_jc|: the scale
    of the cosine tolerance)."""
    rows = np.asarray(rows, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    weights = np.asarray(weights, dtype=np.float64)
    offsets = np.asarray(offsets, dtype=np.int64)
    nq, d = offsets.size - 1, rows.shape[1]
    out = np.zeros((nq, d), dtype=np.float32)
    scale = np.zeros((nq, d), dtype=np.float64)
    for i in range(nq):
        acc = np.zeros(d, np.float64) if base is None else np.asarray(base[i], dtype=np.float32).astype(np.float64)
        for j in range(int(offsets[i]), int(offsets[i + 1])):
            x = rows[labels[j]].astype(np.float64)
            t = np.float64(weights[j])
            if space == "cosine":
                t = t * (np.float64(1.0) / (np.sqrt(np.sum(x * x)) + np.float64(1e-30)))
            p = t * x
            acc = acc + p
            scale[i] += np.abs(p)
        out[i] = acc.astype(np.float32)
    return out, scale


def cosine_query_bound(want, scale):
    """What a component of a device-built cosine query may differ from ``like_queries``' by: one float32 spacing (the norm
    is summed in another order, so the fp64 sum can land on the other side of a rounding boundary) + 1e-12 of the summed
    |terms|."""
    return np.spacing(np.abs(want)).astype(np.float64) + 1e-12 * scale


def example_sets(labels, offsets):
    labels = np.asarray(labels, dtype=np.int64)
    return [set(labels[int(a):int(b)].tolist()) for a, b in zip(offsets[:-1], offsets[1:])]


def most_examples(labels, offsets) -> int:
    """M of mlvdb_like.h: the most distinct example labels of one query."""
    return max((len(s) for s in example_sets(labels, offsets)), default=0)


def like_strip(lab, d32, cnt, d64, sets, k: int):
    """The ranked lists of a plain search (labels / float32 / counts / float64, [nq, F]) with each query's example labels
    removed, the order kept, the first ``k`` entries: (labels [nq, k], float32, counts, float64), padded -1 / +inf."""
    nq = lab.shape[0]
    out_l = np.full((nq, k), -1, np.int64)
    out_d = np.full((nq, k), np.inf, np.float32)
    out_c = np.zeros(nq, np.int32)
    out_64 = np.full((nq, k), np.inf, np.float64)
    for i in range(nq):
        keep = [j for j in range(int(cnt[i])) if int(lab[i, j]) not in sets[i]][:k]
        out_c[i] = len(keep)
        out_l[i, :len(keep)], out_d[i, :len(keep)], out_64[i, :len(keep)] = lab[i, keep], d32[i, keep], d64[i, keep]
    return out_l, out_d, out_c, out_64


class LikeOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``search_like`` as ``HipScanEngine`` declares it."""

    def search_like(self, labels, weights, offsets, k, *, base=None, exclude=True, where=None, want64=False,
                    want_queries=False):
        labels, offsets = np.asarray(labels, np.int64), np.asarray(offsets, np.int64)
        counts = np.diff(offsets)
        assert k >= 1 and (counts <= 64).all() and ((labels >= 0) & (labels < self._rows.shape[0])).all()
        assert base is not None or (counts > 0).all()
        most = most_examples(labels, offsets)
        assert k + most <= 1024
        qs, _ = like_queries(self._rows, labels, weights, offsets, self.space, base)
        sets = example_sets(labels, offsets) if exclude else [set()] * len(counts)
        lab, d32, cnt, d64 = like_strip(*self.search64(qs, k + most if exclude else k, where=where), sets, k)
        return lab, d32, cnt, d64 if want64 else None, qs if want_queries else None


def oracle_index(attributes=None, space="l2", **kw) -> Index:
    return Index(space=space, engine_factory=LikeOracleEngine, attributes=attributes, **kw)
