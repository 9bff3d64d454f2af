"""Shared test helpers (inputs are always regenerated from seeds)."""
from __future__ import annotations

import numpy as np

from oracle import exact_scan

SCORE_ATOL = 1e-5  # north star: scores within 1e-5 (fp32), ids bit-exact


def make_case(seed: int, n: int, d: int, nq: int, *, dup: bool = False, clustered: bool = False):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    if clustered:  # many near-ties: rows are small perturbations of a few centres
        centres = rng.standard_normal((8, d), dtype=np.float32)
        rows = centres[rng.integers(0, 8, n)] + 1e-3 * rows
    if dup and n >= 8:  # exact duplicates: tie-break by label must hold
        rows[n // 2] = rows[1]
        rows[n - 1] = rows[1]
        rows[3] = rows[2]
    qs = rng.standard_normal((nq, d), dtype=np.float32)
    if nq >= 2 and n >= 2:
        qs[0] = rows[1]  # a stored vector queried back: distance exactly 0 (l2) / similarity 1
    return rows, qs


def deleted_mask(seed: int, n: int, frac: float) -> np.ndarray:
    if frac <= 0:
        return np.zeros(n, dtype=bool)
    return np.random.default_rng(seed + 99).random(n) < frac


def assert_knn_matches(got, want, tag: str):
    gl, gd, gc = got
    wl, wd, wc = want
    if not (np.array_equal(gl, wl) and np.array_equal(gc, wc)):
        from tests.conftest import dump_mismatch

        dump_mismatch(tag.replace("/", "_"), got_labels=gl, want_labels=wl, got_dist=gd, want_dist=wd)
        bad = np.nonzero((gl != wl).any(axis=1))[0]
        raise AssertionError(f"{tag}: ids differ for {bad.size} queries, first {bad[:5]}: "
                             f"got {gl[bad[0]]} want {wl[bad[0]]} (d got {gd[bad[0]]} want {wd[bad[0]]})")
    fin = np.isfinite(wd)
    assert np.array_equal(np.isfinite(gd), fin), f"{tag}: padding differs"
    err = np.abs(gd[fin] - wd[fin]).max() if fin.any() else 0.0
    assert err <= SCORE_ATOL, f"{tag}: max |distance error| {err}"


def assert_range_matches(got, want, tag: str):
    """Range hits ``got`` (a ``RangeHits`` or a list of (labels, distances) per query) against the oracle's ``want``: the
    labels equal query by query, every distance within SCORE_ATOL * max(1, |d|) -- the 1e-5 bar, relative beyond 1 as in
    tests/test_pairwise.py (fp32 holds 1e-5 absolute only up to ~100)."""
    assert len(got) == len(want), f"{tag}: {len(got)} queries answered, {len(want)} asked"
    for i, ((gl, gd), (wl, wd)) in enumerate(zip(got, want)):
        gl, gd, wl, wd = np.asarray(gl), np.asarray(gd), np.asarray(wl), np.asarray(wd)
        if not np.array_equal(gl, wl):
            from tests.conftest import dump_mismatch

            dump_mismatch(tag.replace("/", "_"), query=np.int64(i), got_labels=gl, want_labels=wl, got_dist=gd, want_dist=wd)
            m = min(gl.size, wl.size)
            at = int(np.argmax(gl[:m] != wl[:m])) if (gl[:m] != wl[:m]).any() else m
            raise AssertionError(f"{tag}: query {i}: {gl.size} hits, the oracle has {wl.size}; first difference at rank {at}: "
                                 f"got {gl[at:at + 4]} (d {gd[at:at + 4]}) want {wl[at:at + 4]} (d {wd[at:at + 4]})")
        g64, w64 = gd.astype(np.float64), wd.astype(np.float64)
        with np.errstate(invalid="ignore"):
            err = np.where(g64 == w64, 0.0, np.abs(g64 - w64))  # (equal infinities: no error)
        bad = ~(err <= SCORE_ATOL * np.maximum(1.0, np.abs(w64)))
        if bad.any():
            j = int(np.argmax(bad))
            raise AssertionError(f"{tag}: query {i}: distance of label {wl[j]} is {gd[j]!r}, the oracle's {wd[j]!r}")


def oracle_knn(qs, rows, k, space, deleted=None):
    return exact_scan.knn(qs, rows, k, space, deleted=deleted)
