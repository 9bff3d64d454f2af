"""Shared by the sparse-vector tests (include/mlvdb_sparse.h): a model engine that keeps every row's vector as a Python
dict and scores with NumPy fp64 over a dense [rows, vocabulary] matrix (the terms that occur are renumbered densely, so a
term of 2^31 - 1 costs one column), and seeded generators of sparse corpora and queries.  Nothing here asks the library
for an answer: ``where.SparseColumn`` is used as the plain CSR container the engines exchange."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import where as W
from tests.tags_helpers import TagsOracleEngine

TERM_MAX = 2 ** 31 - 1


def sparse_csr(rows) -> W.SparseColumn:
    """Rows as ``None`` / dicts term -> weight -> the CSR container (terms ascending, weights as float32)."""
    offsets, terms, weights, present = [0], [], [], []
    for row in rows:
        present.append(0 if row is None else 1)
        for t in sorted(row or ()):
            terms.append(t)
            weights.append(row[t])
        offsets.append(len(terms))
    return W.SparseColumn(np.array(offsets, dtype=np.int64), np.array(terms, dtype=np.int32),
                          np.array(weights, dtype=np.float32), np.array(present, dtype=np.uint8))


def sparse_uncsr(col: W.SparseColumn):
    """The CSR container -> rows as ``None`` / dicts term -> float32 weight (as a Python float)."""
    off = col.offsets.tolist()
    terms, weights = col.terms.tolist(), col.weights.astype(np.float32).tolist()
    return [dict(zip(terms[off[i]:off[i + 1]], weights[off[i]:off[i + 1]])) if p else None
            for i, p in enumerate(col.present.tolist())]


def dense_scores(queries, rows):
    """(fp64 scores [nq, n], fp64 sums of |wq * wr| [nq, n]) of dict queries against ``None`` / dict rows: the inner
    product over the shared terms, each product exact in fp64 (two float32 factors), summed by NumPy."""
    vocab = sorted({t for q in queries for t in q} | {t for r in rows if r for t in r})
    at = {t: i for i, t in enumerate(vocab)}
    m = np.zeros((len(rows), max(1, len(vocab))), dtype=np.float64)
    for i, r in enumerate(rows):
        for t, w in (r or {}).items():
            m[i, at[t]] = np.float32(w)
    qm = np.zeros((len(queries), max(1, len(vocab))), dtype=np.float64)
    for i, q in enumerate(queries):
        for t, w in q.items():
            qm[i, at[t]] = np.float32(w)
    return qm @ m.T, np.abs(qm) @ np.abs(m).T


def rank(scores, cand, k):
    """Per query the candidates by (score descending, label ascending): (labels [nq, k] padded -1, scores64 [nq, k] padded
    -inf, counts [nq])."""
    nq = scores.shape[0]
    labels = np.full((nq, k), -1, dtype=np.int64)
    s64 = np.full((nq, k), -np.inf, dtype=np.float64)
    counts = np.zeros(nq, dtype=np.int32)
    idx = np.flatnonzero(cand)
    for q in range(nq):
        order = idx[np.lexsort((idx, -scores[q, idx]))][:k]
        labels[q, :order.size] = order
        s64[q, :order.size] = scores[q, order]
        counts[q] = order.size
    return labels, s64, counts


class SparseOracleEngine(TagsOracleEngine):
    """The oracle engine + sparse columns kept as Python dicts: ``self._lists[attr][row]`` is ``None`` or a dict term ->
    weight (the inherited machinery sees its length: EXISTS, LEN, compaction and the pool counters work on it as they do
    for a list), refused by every list and scalar entry as the library refuses it."""

    def __init__(self, dim: int, space: str) -> None:
        super().__init__(dim, space)
        self._sparse = set()

    def define_attr(self, attr, kind):
        if kind != "sparse":
            return super().define_attr(attr, kind)
        super().define_attr(attr, "int64_list")
        self._sparse.add(attr)

    def _refuse_sparse(self, attr, what):
        if attr in self._sparse:
            raise RuntimeError(f"{what} failed (1): a sparse column")

    def _refuse_list(self, attr, what):
        self._refuse_sparse(attr, what)
        super()._refuse_list(attr, what)

    def set_attr_list(self, attr, first, col):
        self._refuse_sparse(attr, "attr_list_set")
        return super().set_attr_list(attr, first, col)

    def set_attr_list_at(self, attr, labels, col):
        self._refuse_sparse(attr, "attr_list_set_at")
        return super().set_attr_list_at(attr, labels, col)

    def get_attr_list(self, attr, first, n):
        self._refuse_sparse(attr, "attr_list_get")
        return super().get_attr_list(attr, first, n)

    def update_where_list(self, program, attr, values):
        self._refuse_sparse(attr, "attr_list_update_where")
        return super().update_where_list(program, attr, values)

    def facet_list_values(self, attr, max_values, where=None):
        self._refuse_sparse(attr, "facet_list_values")
        return super().facet_list_values(attr, max_values, where)

    def set_attr_sparse(self, attr, first, col):
        assert attr in self._sparse
        rows = sparse_uncsr(col)
        assert first + len(rows) <= self._rows.shape[0]
        for i, r in enumerate(rows):
            self._put(attr, first + i, r)
        self._pool_used[attr] += int(col.terms.size)

    def set_attr_sparse_at(self, attr, labels, col):
        assert attr in self._sparse
        labels = np.asarray(labels, dtype=np.int64).ravel()
        rows = sparse_uncsr(col)
        assert len(rows) == labels.size
        if labels.size and (labels.min() < 0 or labels.max() >= self._rows.shape[0] or np.unique(labels).size != labels.size):
            raise RuntimeError("sparse_set_at failed (1): bad labels")
        wrote = 0
        for lab, r in zip(labels.tolist(), rows):
            if not self._deleted[lab]:
                self._put(attr, lab, r)
                wrote += 1
        self._pool_used[attr] += int(col.terms.size)
        return wrote

    def get_attr_sparse(self, attr, first, n):
        assert attr in self._sparse
        return sparse_csr(self._lists[attr][first:first + n])

    def sparse_rows(self, attr):
        return self._lists[attr]

    def candidates(self, attr, where=None):
        """bool [total]: live, holding a vector (an empty one too), matching."""
        have = np.array([r is not None for r in self._lists[attr]], dtype=bool).reshape(self._rows.shape[0])
        return self._mask(where) & have

    def search_batch_sparse(self, attr, queries, k, where=None):
        assert attr in self._sparse
        qs = sparse_uncsr(W.SparseColumn(queries.offsets, queries.terms, queries.weights,
                                         np.ones(queries.offsets.size - 1, dtype=np.uint8)))
        scores, _ = dense_scores(qs, self._lists[attr])
        labels, s64, counts = rank(scores, self.candidates(attr, where), k)
        with np.errstate(over="ignore"):
            return labels, s64.astype(np.float32), counts, s64


# ---------------------------------------------------------------- seeded corpora and queries
def exact_weight(rng):
    """A nonzero multiple of 1/8 in [-4, 4]: sums of products of such weights are exact in fp64 in any order."""
    w = 0
    while w == 0:
        w = int(rng.integers(-32, 33))
    return w / 8.0


def random_vector(rng, length, vocab, exact, terms=None):
    """A dict of ``length`` distinct terms below ``vocab`` (or drawn from ``terms``) with exact or random fp32 weights."""
    pick = rng.choice(vocab if terms is None else terms, size=length, replace=False)
    return {int(t): (exact_weight(rng) if exact else float(np.float32(rng.standard_normal()) or np.float32(1)))
            for t in np.atleast_1d(pick).tolist()}


def random_corpus(rng, n, vocab, exact, p_absent=0.1):
    """n rows: ``None`` for about ``p_absent`` of them, else vectors of mostly short lengths with 0, 1, 15, 16, 17 and 255
    among them (255 only when the vocabulary allows), the first terms 0 and 2^31 - 1 planted in a few rows."""
    special = [0, 1, 15, 16, 17, min(255, vocab)]
    rows = []
    for i in range(n):
        if rng.random() < p_absent:
            rows.append(None)
            continue
        length = special[i % len(special)] if i % 7 == 0 else int(rng.integers(0, min(40, vocab) + 1))
        rows.append(random_vector(rng, length, vocab, exact))
    for i in range(3, n, 97):  # the ends of the term range, next to ordinary terms
        if rows[i] is not None and len(rows[i]) < 254:
            rows[i].pop(0, None)
            rows[i][0] = exact_weight(rng) if exact else 0.75
            rows[i][TERM_MAX] = exact_weight(rng) if exact else -1.5
    return rows


# ---------------------------------------------------------------- snapshots of indexes without a sparse attribute
def legacy_index(version):
    """A fixed index without a sparse attribute (v1: no attributes, v2: scalar ones, v3: scalar and list ones) on the model
    engine, ids fixed: its snapshot files are hashed against what the code before sparse attributes wrote."""
    import uuid

    from mlvectordb_amd.index import Index
    from mlvectordb_amd.vector import Vector

    rng = np.random.default_rng(33)
    schema = {"v1": {}, "v2": {"genre": "str", "year": "int", "price": "float"},
              "v3": {"genre": "str", "tags": "str[]", "nums": "int[]", "price": "float"}}[version]
    index = Index(space="cosine", engine_factory=lambda dim, sp: TagsOracleEngine(dim, sp), attributes=schema)
    vectors = [Vector(values=rng.standard_normal(5).astype(np.float32).tolist(),
                      metadata={"genre": ["folk", None, "dub"][i % 3], "year": 1990 + i, "price": i / 8 if i % 4 else None,
                                "tags": [["a", "b"], [], None, ["c"]][i % 4], "nums": [i % 5, 7] if i % 6 else None})
               for i in range(50)]
    for i, v in enumerate(vectors):
        v._id = uuid.UUID(int=5000 + i)  # (ids are random by default: fixed here, the files are hashed)
    index.add(vectors[:30], "ns")
    index.add(vectors[30:], "ns")
    index.remove([v.id for v in vectors[::9]], "ns")
    if version == "v3":
        index.update_attributes([vectors[1].id, vectors[2].id], [{"tags": ["z"]}, {"nums": None}], "ns")
    return index
