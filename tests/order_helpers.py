"""Shared by the ordered-query tests (include/mlvdb_order.h): the NumPy oracle of ``mlvdb_where_ordered`` and an oracle engine
that answers it without a GPU."""
from __future__ import annotations

import numpy as np

from tests.facet_helpers import FacetOracleEngine, present_of

MAX_ROWS = 4096  # MLVDB_ORDER_MAX_ROWS


def ordered_oracle(col: np.ndarray, mask: np.ndarray, descending: bool, offset: int, limit: int):
    """(labels, col[labels], matched, absent): ranks [offset, offset + limit) of the rows of ``mask`` (live and matching)
    that hold a present value, by value -- ``descending`` reverses the values only -- and ties by ascending label."""
    present = present_of(col)
    labels = np.flatnonzero(mask & present)
    values = col[labels]
    if col.dtype == np.float64:
        key = values + 0.0  # folds -0.0 onto 0.0
        key = -key if descending else key
    else:
        key = ~values if descending else values  # (a negation can overflow; the complement reverses the order exactly)
    order = np.lexsort((labels, key))
    picked = labels[order][offset:offset + limit].astype(np.int64)
    return picked, col[picked], int(mask.sum()), int((mask & ~present).sum())


class OrderOracleEngine(FacetOracleEngine):
    """``FacetOracleEngine`` + ``where_ordered`` of ``HipScanEngine``, in NumPy."""

    def where_ordered(self, attr, limit, where=None, descending=False, offset=0):
        assert 0 <= offset and 1 <= limit and offset + limit <= MAX_ROWS
        return ordered_oracle(self._cols[attr], self._mask(where), bool(descending), int(offset), int(limit))
