"""The host side of the similarity join (include/mlvdb_join.h): the answer class of ``Index.join_within``, the regrouping of
a by-ids answer into the caller's order, and the connected components ``Index.duplicate_groups`` makes of a self-join's
pairs."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

METRICS = ("l2", "euclidean", "cosine", "ip")  # the metrics a join takes: the ones ``range_search_many`` post-processes
ORDERS = ("left", "distance")


class PairHits:
    """The pairs of a join, one entry per pair: ``left_ids`` / ``right_ids`` (object arrays of UUIDs), ``scores`` (float64,
    post-processed like ``range_search_many``), the engine's ``left_labels`` / ``right_labels`` (insertion order) and the
    float32 ``distances`` behind the scores; per left row its ``left_row_ids`` and the exact number of partners ``counts``
    (also above ``max_per_row``).  ``complete``: no row had more partners than ``max_per_row``, so every pair is here."""

    __slots__ = ("left_ids", "right_ids", "scores", "counts", "complete", "left_labels", "right_labels", "distances",
                 "left_row_ids")

    def __init__(self, left_ids, right_ids, scores, counts, complete, left_labels, right_labels, distances, left_row_ids):
        self.left_ids, self.right_ids, self.scores = left_ids, right_ids, scores
        self.counts, self.complete = counts, bool(complete)
        self.left_labels, self.right_labels, self.distances = left_labels, right_labels, distances
        self.left_row_ids = left_row_ids

    @classmethod
    def empty(cls, n_left: int = 0, left_row_ids=None) -> "PairHits":
        none = np.zeros(0, dtype=object)
        return cls(none, none.copy(), np.zeros(0, np.float64), np.zeros(n_left, np.int64), True, np.zeros(0, np.int64),
                   np.zeros(0, np.int64), np.zeros(0, np.float32),
                   np.zeros(n_left, dtype=object) if left_row_ids is None else left_row_ids)

    def __len__(self) -> int:
        return int(self.left_labels.size)

    def pairs(self) -> List[tuple]:
        """[(left id, right id, score), ...] in the answer's order."""
        return list(zip(self.left_ids.tolist(), self.right_ids.tolist(), self.scores.tolist()))


def gather_segments(offsets: np.ndarray, order: np.ndarray) -> np.ndarray:
    """Indices into packed arrays laid out by ``offsets`` that list the segments ``order[0], order[1], ...`` one after the
    other (each segment's entries in their own order)."""
    lens = np.diff(offsets)[order]
    starts = offsets[:-1][order]
    ends = np.cumsum(lens)
    return np.repeat(starts - (ends - lens), lens) + np.arange(int(ends[-1]) if ends.size else 0, dtype=np.int64)


def connected_groups(left: Sequence[int], right: Sequence[int]) -> List[List[int]]:
    """The connected components (size >= 2) of the graph with edges ``(left[i], right[i])`` over integer nodes: every group
    ascending, the groups ordered by their first member.  A plain union-find (path halving, the smaller root wins)."""
    parent: dict = {}

    def find(x: int) -> int:
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(left, dtype=np.int64).tolist(), np.asarray(right, dtype=np.int64).tolist()):
        parent.setdefault(a, a)
        parent.setdefault(b, b)
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    groups: dict = {}
    for x in sorted(parent):
        groups.setdefault(find(x), []).append(x)
    return [g for _, g in sorted(groups.items()) if len(g) >= 2]
