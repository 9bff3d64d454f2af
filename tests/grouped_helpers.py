"""Shared by the grouped-kNN tests (include/mlvdb_grouped.h): the NumPy oracle, a brute-force restatement of it, an oracle
engine with ``search_grouped``, and the member stage's host rules mirrored (the code table's size, the tiles and the rows per
list chunk), so a test can state which tiles a call takes and how many chunks a list is cut into."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd.index import Index
from oracle import exact_scan
from tests.distinct_helpers import ABSENT, DistinctOracleEngine, distinct_knn
from tests.helpers import SCORE_ATOL

# csrc/internal.h
GROUPED_BLOCKS = 2048    # kGroupedBlocks
GROUPED_MIN_CHUNK = 256  # kGroupedMinChunk
MAX_GROUP_SIZE = 64      # MLVDB_GROUPED_MAX_SIZE


def grouped_knn(dist: np.ndarray, groups: np.ndarray, allowed: np.ndarray, k: int, g: int):
    """``distinct_knn`` for the groups, then the first g rows of ``lexsort((label, distance))`` within each group.
    Returns (labels int64 [nq, k, g], dist64 [nq, k, g], counts int32 [nq], group_counts int32 [nq, k], groups int64 [nq, k]),
    padded -1 / inf / 0 / ABSENT."""
    nq = dist.shape[0]
    _, _, counts, grp = distinct_knn(dist, groups, allowed, k)
    ok = np.asarray(allowed, bool)
    labels = np.full((nq, k, g), -1, np.int64)
    d64 = np.full((nq, k, g), np.inf)
    gcnt = np.zeros((nq, k), np.int32)
    for i in range(nq):
        for j in range(counts[i]):
            idx = np.flatnonzero(ok & (groups == grp[i, j]))
            keep = idx[np.lexsort((idx, dist[i, idx]))][:g]
            gcnt[i, j] = keep.size
            labels[i, j, :keep.size], d64[i, j, :keep.size] = keep, dist[i, keep]
    return labels, d64, counts, gcnt, grp


def grouped_knn_brute(dist: np.ndarray, groups: np.ndarray, allowed: np.ndarray, k: int, g: int):
    """The same answer by the definition itself: every group's allowed rows sorted by (distance, label), the groups ranked by
    their first row, the first g rows of the first k groups.  Per query a list of (group, [(distance, row), ...])."""
    out = []
    for i in range(dist.shape[0]):
        members = {}
        for row in range(groups.size):
            code = int(groups[row])
            if allowed[row] and code != ABSENT:
                members.setdefault(code, []).append((float(dist[i, row]), row))
        ranked = sorted((sorted(rows)[0], code) for code, rows in members.items())[:k]
        out.append([(code, sorted(members[code])[:g]) for _, code in ranked])
    return out


class GroupedOracleEngine(DistinctOracleEngine):
    """``DistinctOracleEngine`` + ``search_grouped`` as ``HipScanEngine`` declares it."""

    def search_grouped(self, queries, k, group_size, attr, max_groups=0, where=None, want64=False):
        col = self._cols[attr]
        assert col.dtype == np.int64
        allowed = ~self._deleted if where is None else self.match(where)
        dist = exact_scan.exact_distances(queries, self._rows, self.space)
        labels, d64, counts, gcnt, grp = grouped_knn(dist, col, allowed, k, group_size)
        if max_groups:
            assert counts.max(initial=0) <= max_groups
        d32 = d64.astype(np.float32)
        return (labels, d32, counts, gcnt, d64, grp) if want64 else (labels, d32, counts, gcnt, grp)


def check_grouped(eng, qs, k, g, got, want, tag, magnitudes=None):
    """``got``: what ``eng.search_grouped(qs, k, g, attr, want64=True)`` returned, against the oracle's (labels, d64, counts,
    group counts, groups) for this k and g: everything but the distances exactly, the fp64 distances within SCORE_ATOL, the
    fp32 ones the rounded fp64, both bit-equal to ``pair_distances`` of the same handle.

    ``magnitudes`` (tests/test_gpu_magnitudes_families.py: inputs anywhere in the float32 range) = (rows, space, excluded
    queries): padding is then told by label -1 alone -- a real row's fp32 distance may be +-inf -- the fp64 distances are held
    to magnitude_helpers.family_fp64_bar in place of the absolute SCORE_ATOL, and the ids of the ``excluded`` queries (those
    the model itself answers differently under another order of summation) are not compared; the bit contracts hold for
    every query either way."""
    from tests.conftest import dump_mismatch

    lab, dist, cnt, gcnt, d64, grp = got
    wl, wd, wc, wgc, wg = want
    bad = np.flatnonzero((lab != wl).any(axis=(1, 2)) | (cnt != wc) | (gcnt != wgc).any(axis=1) | (grp != wg).any(axis=1))
    if magnitudes is not None:
        bad = np.setdiff1d(bad, np.asarray(magnitudes[2], dtype=np.int64))
    if bad.size:
        dump_mismatch(f"grouped_{tag}".replace("/", "_"), lab=lab, wl=wl, cnt=cnt, wc=wc, gcnt=gcnt, wgc=wgc, grp=grp, wg=wg,
                      d64=d64, wd=wd)
        raise AssertionError(f"{tag}: {bad.size} queries differ, first {bad[0]}: got {lab[bad[0]].tolist()} ({cnt[bad[0]]}, "
                             f"{gcnt[bad[0]].tolist()}) want {wl[bad[0]].tolist()} ({wc[bad[0]]}, {wgc[bad[0]].tolist()})")
    if magnitudes is None:
        fin = np.isfinite(wd)
        assert np.array_equal(np.isfinite(d64), fin) and np.array_equal(np.isfinite(dist), fin), f"{tag}: padding differs"
        if fin.any():
            err = float(np.abs(d64[fin] - wd[fin]).max())
            print(f"{tag}: max |d64 - oracle| = {err:.3e}")
            assert err <= SCORE_ATOL, f"{tag}: distance error {err}"
    else:
        from tests.magnitude_helpers import assert_family_fp64

        pad = lab < 0
        assert np.isposinf(d64[pad]).all() and np.isposinf(dist[pad]).all(), f"{tag}: padding distances are not +inf"
        assert_family_fp64(d64, None, qs, magnitudes[0], lab, magnitudes[1], tag)
    # the fp32 output is the fp64 distance rounded once (an absolute bound cannot be asked of fp32 itself beyond 128)
    with np.errstate(over="ignore"):
        rounded = d64.astype(np.float32)
    assert np.array_equal(dist.view(np.int32), rounded.view(np.int32)), f"{tag}: fp32 is not the rounded fp64"
    nq = qs.shape[0]
    p64, p32 = eng.pair_distances(qs, lab.reshape(nq, k * g))
    assert np.array_equal(p64.view(np.int64), d64.reshape(nq, k * g).view(np.int64)), f"{tag}: fp64 differs from pair_distances"
    assert np.array_equal(p32.view(np.int32), dist.reshape(nq, k * g).view(np.int32)), f"{tag}: fp32 differs from pair_distances"
    return lab, cnt, gcnt, grp


def oracle_index(attributes, space="l2", **kw) -> Index:
    return Index(space=space, engine_factory=GroupedOracleEngine, attributes=attributes, **kw)


# ---------------------------------------------------------------- the member stage's host rules (api.hip: grouped_members)
def table_slots(ncodes: int) -> int:
    """Slots of the code table of a chunk: the smallest power of two >= 2 x the number of distinct picked codes."""
    slots = 1
    while slots < 2 * max(ncodes, 1):
        slots *= 2
    return slots


def chunk_rows(work: int) -> int:
    """Rows per chunk of a member list (grouped_chunk_rows): ``work`` = the sum over the tiles of their list's length; about
    GROUPED_BLOCKS blocks share it evenly, a chunk is a multiple of 64 rows and never below GROUPED_MIN_CHUNK."""
    even = (-(-work // GROUPED_BLOCKS) + 63) // 64 * 64
    return max(even, GROUPED_MIN_CHUNK)


def tile_plan(grp: np.ndarray, counts: np.ndarray, members: dict, qt_max: int = 4):
    """The tiles of one chunk (<= 1024 queries) of a call: ``grp`` [n, k] / ``counts`` [n] are the distinct stage's answer,
    ``members[code]`` the number of live allowed rows of a group.  Returns (rows per list chunk, [(code, pairs in the tile,
    chunks of the list)] in launch order of the host loop): a group's pairs are cut into tiles of <= ``qt_max``."""
    picked = {}
    for i in range(grp.shape[0]):
        for j in range(int(counts[i])):
            picked[int(grp[i, j])] = picked.get(int(grp[i, j]), 0) + 1
    work = sum(-(-n // qt_max) * members[code] for code, n in picked.items())
    rows = chunk_rows(work)
    tiles = []
    for code in sorted(picked):
        nch = max(1, -(-members[code] // rows))
        left = picked[code]
        while left:
            take = min(qt_max, left)
            tiles.append((code, take, nch))
            left -= take
    return rows, tiles
