"""Shared by the late-interaction tests (include/mlvdb_maxsim.h): the NumPy oracle, a brute-force restatement of it in Python
floats, and an oracle engine with ``search_maxsim``."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd.index import Index
from oracle import exact_scan
from tests.distinct_helpers import ABSENT
from tests.helpers import SCORE_ATOL
from tests.where_helpers import WhereOracleEngine

MAX_TOKENS = 128  # MLVDB_MAXSIM_MAX_TOKENS


def offsets_of(lengths) -> np.ndarray:
    """Token offsets [nq + 1] of queries of ``lengths`` tokens."""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def maxsim_oracle(dist: np.ndarray, groups: np.ndarray, allowed: np.ndarray, offsets: np.ndarray, k: int):
    """The k best documents per query from a float64 distance matrix ``dist`` [total tokens, n] (``exact_distances`` of the
    tokens): over the rows that are ``allowed`` (live, matching) and hold a present value, best(t, g) = the (distance, label)
    minimum of token t among the rows of document g; score = the sequential sum over the query's tokens, in order, from 0.0;
    documents by (score, code).  Returns (groups int64 [nq, k], score64 [nq, k], counts int32 [nq], match_labels int64
    [total tokens, k], match_dist64 [total tokens, k]), padded ABSENT / inf / -1 / inf."""
    offsets = np.asarray(offsets, dtype=np.int64)
    nq, ntok = offsets.size - 1, dist.shape[0]
    idx = np.flatnonzero(np.asarray(allowed, bool) & (groups != ABSENT))
    codes, inv = np.unique(groups[idx], return_inverse=True)
    out_g = np.full((nq, k), ABSENT, np.int64)
    out_s = np.full((nq, k), np.inf)
    counts = np.zeros(nq, np.int32)
    m_lab = np.full((ntok, k), -1, np.int64)
    m_d = np.full((ntok, k), np.inf)
    if codes.size == 0:
        return out_g, out_s, counts, m_lab, m_d
    # rows sorted by document, then label: the first minimum of a segment is the (distance, label) minimum
    order = np.lexsort((idx, inv))
    rows, seg_of = idx[order], inv[order]
    starts = np.searchsorted(seg_of, np.arange(codes.size))
    best = np.empty((ntok, codes.size))
    best_row = np.empty((ntok, codes.size), np.int64)
    for t in range(ntok):
        d = dist[t, rows]
        best[t] = np.minimum.reduceat(d, starts)
        hit = np.flatnonzero(d == best[t][seg_of])
        first = np.full(codes.size, -1, np.int64)
        first[seg_of[hit[::-1]]] = hit[::-1]  # (of repeated indices the last assignment stays: the lowest position)
        best_row[t] = np.where(first >= 0, rows[first], -1)
    for i in range(nq):
        t0, t1 = int(offsets[i]), int(offsets[i + 1])
        score = np.cumsum(np.vstack([np.zeros((1, codes.size)), best[t0:t1]]), axis=0)[-1]  # (((0.0 + b0) + b1) + ...)
        rank = np.lexsort((codes, score))[:k]
        rank = rank[~np.isnan(score[rank])]
        c = rank.size
        counts[i] = c
        out_g[i, :c], out_s[i, :c] = codes[rank], score[rank]
        m_lab[t0:t1, :c], m_d[t0:t1, :c] = best_row[t0:t1][:, rank], best[t0:t1][:, rank]
    return out_g, out_s, counts, m_lab, m_d


def maxsim_brute(dist: np.ndarray, groups: np.ndarray, allowed: np.ndarray, offsets, k: int):
    """The same answer by the definition itself, in Python floats: per query a list of (score, code, [(distance, row) per
    token])."""
    out = []
    for i in range(len(offsets) - 1):
        docs = {}
        for row in range(groups.size):
            code = int(groups[row])
            if allowed[row] and code != ABSENT:
                docs.setdefault(code, []).append(row)
        ranked = []
        for code, rows in docs.items():
            matches, score = [], 0.0
            for t in range(int(offsets[i]), int(offsets[i + 1])):
                d, row = min((float(dist[t, r]), r) for r in rows)
                matches.append((d, row))
                score = score + d
            ranked.append((score, code, matches))
        out.append(sorted(ranked)[:k])
    return out


class MaxSimOracleEngine(WhereOracleEngine):
    """``WhereOracleEngine`` + ``search_maxsim`` as ``HipScanEngine`` declares it; every call is recorded."""

    def __init__(self, dim: int, space: str) -> None:
        super().__init__(dim, space)
        self.maxsim_calls = []

    def search_maxsim(self, tokens, offsets, k, attr, where=None, want_matches=False):
        self.maxsim_calls.append(dict(tokens=np.array(tokens), offsets=np.array(offsets), k=k, attr=attr, where=where,
                                      want_matches=want_matches))
        col = self._cols[attr]
        assert col.dtype == np.int64
        allowed = ~self._deleted if where is None else self.match(where)
        dist = exact_scan.exact_distances(tokens, self._rows, self.space)
        grp, s64, counts, m_lab, m_d = maxsim_oracle(dist, col, allowed, offsets, k)
        return grp, s64.astype(np.float32), counts, s64, (m_lab if want_matches else None), (m_d if want_matches else None)


def _seq_sum(md, off, k):
    """[nq, k]: (((0.0 + d0) + d1) + ...) over each query's token rows of ``md`` [tokens, k]."""
    out = np.empty((off.size - 1, k))
    for i in range(off.size - 1):
        acc = np.zeros(k)
        for t in range(int(off[i]), int(off[i + 1])):
            acc = acc + md[t]
        out[i] = acc
    return out


def check_maxsim(eng, toks, off, k, got, want, tag, magnitudes=None):
    """``got``: what ``eng.search_maxsim(toks, off, k, attr, want_matches=True)`` returned, against the oracle's (groups,
    score64, counts, match labels, match dist64) for this k; the bit contracts.

    ``magnitudes`` (tests/test_gpu_magnitudes_families.py: inputs anywhere in the float32 range) = (rows, space, excluded
    queries): padding is then told by group INT64_MIN / label -1 alone -- a real document's fp32 score may be +-inf -- every
    match distance is held to magnitude_helpers.family_fp64_bar (the score is their sequential sum, bit for bit, below), and
    the ids of the ``excluded`` queries are not compared; the bit contracts hold for every query either way."""
    from tests.conftest import dump_mismatch

    grp, s32, cnt, s64, ml, md = got
    wg, ws, wc, wml, wmd = want
    off = np.asarray(off, dtype=np.int64)
    tok_query = np.repeat(np.arange(off.size - 1), np.diff(off))
    bad = np.union1d(np.flatnonzero((grp != wg).any(axis=1) | (cnt != wc)), tok_query[(ml != wml).any(axis=1)])
    if magnitudes is not None:
        bad = np.setdiff1d(bad, np.asarray(magnitudes[2], dtype=np.int64))
    if bad.size:
        dump_mismatch(f"maxsim_{tag}".replace("/", "_"), grp=grp, wg=wg, cnt=cnt, wc=wc, ml=ml, wml=wml, s64=s64, ws=ws, md=md,
                      wmd=wmd)
        i = int(bad[0])
        raise AssertionError(f"{tag}: {bad.size} queries differ in groups / counts / match labels (first {i}: got "
                             f"{grp[i].tolist()} ({cnt[i]}) want {wg[i].tolist()} ({wc[i]})); match labels equal: "
                             f"{np.array_equal(ml, wml)}")
    if magnitudes is None:
        fin = np.isfinite(ws)
        assert np.array_equal(np.isfinite(s64), fin) and np.array_equal(np.isfinite(s32), fin), f"{tag}: padding differs"
        assert np.array_equal(np.isfinite(md), np.isfinite(wmd)), f"{tag}: match padding differs"
        if fin.any():
            err = float((np.abs(s64[fin] - ws[fin]) / np.maximum(1.0, np.abs(ws[fin]))).max())
            print(f"{tag}: max |score64 - oracle| / max(1, |s|) = {err:.3e}")
            assert err <= SCORE_ATOL, f"{tag}: score error {err}"
    else:
        from tests.magnitude_helpers import assert_family_fp64

        pad = grp == ABSENT
        assert np.array_equal(pad, np.arange(k)[None, :] >= cnt[:, None]), f"{tag}: the padded groups are not the tail"
        assert np.isposinf(s64[pad]).all() and np.isposinf(s32[pad]).all(), f"{tag}: padding scores are not +inf"
        assert np.isfinite(s64[~pad]).all(), f"{tag}: an fp64 score of finite inputs is not finite"
        assert np.array_equal(ml < 0, pad[tok_query]), f"{tag}: match padding differs from the groups'"
        assert_family_fp64(md, None, toks, magnitudes[0], ml, magnitudes[1], tag)
    with np.errstate(over="ignore"):
        rounded = s64.astype(np.float32)
    assert np.array_equal(s32.view(np.int32), rounded.view(np.int32)), f"{tag}: fp32 is not the rounded fp64"
    p64, _ = eng.pair_distances(toks, ml)
    assert np.array_equal(p64.view(np.int64), md.view(np.int64)), f"{tag}: match distances differ from pair_distances"
    assert np.array_equal(_seq_sum(md, off, k).view(np.int64), s64.view(np.int64)), f"{tag}: score64 is not the sequential sum"
    return grp, cnt, s64, ml, md


def oracle_index(attributes, space="l2", **kw) -> Index:
    return Index(space=space, engine_factory=MaxSimOracleEngine, attributes=attributes, **kw)
