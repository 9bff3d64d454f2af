"""Shared by the binary-vector tests (include/mlvdb_bits.h): a model engine that keeps every row's code as a tuple of Python
ints (one per 64-bit word) and computes distances from ``np.unpackbits`` sums, and seeded generators of corpora of codes.
Nothing here asks the library for an answer: ``where.BitsColumn`` is used as the plain container the engines exchange."""
from __future__ import annotations

import numpy as np

from mlvectordb_amd import where as W
from tests.sparse_helpers import SparseOracleEngine

METRICS = ("hamming", "jaccard")


def unpack(words) -> np.ndarray:
    """uint64 [n, W] -> uint8 [n, 64 W]: entry b of a row is bit b of its code (bit b & 63 of word b >> 6)."""
    words = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")


def distances(queries, codes, metric, chunk=8192) -> np.ndarray:
    """fp64 [nq, n]: the distance of every query to every code, from sums over the unpacked bits.  The counts are integers
    of at most 16,320, so the fp32 matrix product that sums them (``chunk`` codes at a time) is exact; Jaccard is one fp64
    division of two of them."""
    q = unpack(queries).astype(np.float32)
    pq = q.sum(axis=1, dtype=np.float64)[:, None]
    out = np.empty((q.shape[0], len(codes)), dtype=np.float64)
    for lo in range(0, len(codes), chunk):
        x = unpack(codes[lo:lo + chunk]).astype(np.float32)
        inter = (q @ x.T).astype(np.float64)  # popcount(q & x)
        px = x.sum(axis=1, dtype=np.float64)[None, :]
        if metric == "hamming":
            out[:, lo:lo + chunk] = pq + px - 2.0 * inter  # popcount(q ^ x)
        else:
            assert metric == "jaccard"
            union = pq + px - inter
            with np.errstate(invalid="ignore", divide="ignore"):
                out[:, lo:lo + chunk] = np.where(union == 0, 0.0, (union - inter) / union)  # (both fp64: one division)
    return out


def rank(dist, cand, k):
    """Per query the candidates by (distance ascending, label ascending): (labels [nq, k] padded -1, dist64 [nq, k] padded
    +inf, counts [nq]).  ``dist`` holds one column per entry of ``cand`` that is set, in label order."""
    nq = dist.shape[0]
    labels = np.full((nq, k), -1, dtype=np.int64)
    d64 = np.full((nq, k), np.inf, dtype=np.float64)
    counts = np.zeros(nq, dtype=np.int32)
    idx = np.flatnonzero(cand)
    for q in range(nq):
        order = np.lexsort((idx, dist[q]))[:k]
        labels[q, :order.size] = idx[order]
        d64[q, :order.size] = dist[q, order]
        counts[q] = order.size
    return labels, d64, counts


def bits_column(rows, words) -> W.BitsColumn:
    """Rows as ``None`` / sequences of ``words`` ints -> the container."""
    out = np.zeros((len(rows), words), dtype=np.uint64)
    present = np.zeros(len(rows), dtype=np.uint8)
    for i, r in enumerate(rows):
        if r is not None:
            out[i] = np.array(r, dtype=np.uint64)
            present[i] = 1
    return W.BitsColumn(out, present)


class BitsOracleEngine(SparseOracleEngine):
    """The oracle engine + bits columns: ``self._lists[attr][row]`` is ``None`` or a tuple of the code's words as Python ints
    (the inherited machinery sees its length: EXISTS, compaction and the pool counters work on it as they do for a list),
    refused by every scalar, list and sparse entry as the library refuses it."""

    def __init__(self, dim: int, space: str) -> None:
        super().__init__(dim, space)
        self._bits = set()

    def define_attr(self, attr, kind):
        if kind != "bits":
            return super().define_attr(attr, kind)
        super().define_attr(attr, "int64_list")
        self._bits.add(attr)

    def _refuse_bits(self, attr, what):
        if attr in self._bits:
            raise RuntimeError(f"{what} failed (1): a bits column")

    def _refuse_sparse(self, attr, what):  # (every list entry and, through _refuse_list, every scalar one asks here)
        self._refuse_bits(attr, what)
        super()._refuse_sparse(attr, what)

    def set_attr_sparse(self, attr, first, col):
        self._refuse_bits(attr, "sparse_set")
        return super().set_attr_sparse(attr, first, col)

    def set_attr_sparse_at(self, attr, labels, col):
        self._refuse_bits(attr, "sparse_set_at")
        return super().set_attr_sparse_at(attr, labels, col)

    def get_attr_sparse(self, attr, first, n):
        self._refuse_bits(attr, "sparse_get")
        return super().get_attr_sparse(attr, first, n)

    def search_batch_sparse(self, attr, queries, k, where=None):
        self._refuse_bits(attr, "search_batch_sparse")
        return super().search_batch_sparse(attr, queries, k, where)

    @staticmethod
    def _codes(col):
        words = np.asarray(col.words, dtype=np.uint64)
        assert words.ndim == 2 and words.shape[0] == col.present.size and 1 <= words.shape[1] <= 255
        return [tuple(r) if p else None for r, p in zip(words.tolist(), col.present.tolist())], words.shape[1]

    def bits_set(self, attr, first, col):
        assert attr in self._bits
        rows, words = self._codes(col)
        assert first + len(rows) <= self._rows.shape[0]
        for i, r in enumerate(rows):
            self._put(attr, first + i, r)
        self._pool_used[attr] += words * int(np.count_nonzero(col.present))

    def bits_set_at(self, attr, labels, col):
        assert attr in self._bits
        labels = np.asarray(labels, dtype=np.int64).ravel()
        rows, words = self._codes(col)
        assert len(rows) == labels.size
        if labels.size and (labels.min() < 0 or labels.max() >= self._rows.shape[0] or np.unique(labels).size != labels.size):
            raise RuntimeError("bits_set_at failed (1): bad labels")
        wrote = 0
        for lab, r in zip(labels.tolist(), rows):
            if not self._deleted[lab]:
                self._put(attr, lab, r)
                wrote += 1
        self._pool_used[attr] += words * int(np.count_nonzero(col.present))
        return wrote

    def bits_get(self, attr, first, n):
        assert attr in self._bits
        rows = self._lists[attr][first:first + n]
        widths = np.array([0 if r is None else len(r) for r in rows], dtype=np.int32)
        flat = [w for r in rows if r is not None for w in r]
        return widths, np.array(flat, dtype=np.uint64)

    def bits_rows(self, attr):
        return self._lists[attr]

    def candidates(self, attr, where=None, words=None):
        """bool [total]: live, matching, holding a code (of ``words`` words, when given)."""
        have = np.array([r is not None and (words is None or len(r) == words) for r in self._lists[attr]],
                        dtype=bool).reshape(self._rows.shape[0])
        return self._mask(where) & have

    def search_bits(self, attr, queries, k, metric="hamming", where=None):
        assert attr in self._bits and metric in METRICS
        queries = np.asarray(queries, dtype=np.uint64)
        nq, words = queries.shape
        cand = self.candidates(attr, where, words)
        idx = np.flatnonzero(cand)
        codes = np.array([self._lists[attr][i] for i in idx.tolist()], dtype=np.uint64).reshape(idx.size, words)
        dist = distances(queries, codes, metric) if idx.size and nq else np.zeros((nq, idx.size))
        labels, d64, counts = rank(dist, cand, k)
        return labels, d64.astype(np.float32), counts, d64


# ---------------------------------------------------------------- seeded corpora
def random_codes(rng, n, words, alphabet=12, p_alphabet=0.5):
    """uint64 [n, words]: about ``p_alphabet`` of the rows repeat one of ``alphabet`` distinct codes (so that groups of rows
    at exactly the same distance of any query are large and straddle every rank), the others are uniformly random; a few
    codes of the alphabet are sparse (few bits set) and the all-zero and all-ones codes are among them."""
    base = rng.integers(0, 2 ** 64, size=(alphabet, words), dtype=np.uint64)
    base[0] = 0
    base[1] = np.uint64(2 ** 64 - 1)
    for a in range(2, min(5, alphabet)):  # sparse codes: Jaccard distances away from 1
        base[a] &= rng.integers(0, 2 ** 64, size=words, dtype=np.uint64) & rng.integers(0, 2 ** 64, size=words, dtype=np.uint64)
    codes = rng.integers(0, 2 ** 64, size=(n, words), dtype=np.uint64)
    pick = rng.random(n) < p_alphabet
    codes[pick] = base[rng.integers(0, alphabet, size=int(pick.sum()))]
    return codes, base


def near(rng, code, flips):
    """``code`` with ``flips`` distinct bits flipped."""
    out = np.array(code, dtype=np.uint64).copy()
    for b in rng.choice(64 * out.size, size=flips, replace=False).tolist():
        out[b >> 6] ^= np.uint64(1 << (b & 63))
    return out


# ---------------------------------------------------------------- snapshots of indexes without a bits attribute
def legacy_index(version):
    """A fixed index without a bits attribute on a model engine, ids fixed: v1 - v3 are ``sparse_helpers.legacy_index``'s, v4
    adds a sparse attribute and v5 holds a geo one.  Its snapshot files are hashed against what the code before bits
    attributes wrote."""
    import uuid

    from mlvectordb_amd.index import Index
    from mlvectordb_amd.vector import Vector
    from tests import geo_helpers, sparse_helpers

    if version in ("v1", "v2", "v3"):
        return sparse_helpers.legacy_index(version)
    rng = np.random.default_rng(34)
    schema = {"v4": {"genre": "str", "lexical": "sparse", "tags": "str[]"},
              "v5": {"genre": "str", "loc": "geo", "price": "float"}}[version]
    engine = SparseOracleEngine if version == "v4" else geo_helpers.oracle_engine_class()
    index = Index(space="cosine", engine_factory=lambda dim, sp: engine(dim, sp), attributes=schema)
    vectors = [Vector(values=rng.standard_normal(5).astype(np.float32).tolist(),
                      metadata={"genre": ["folk", None, "dub"][i % 3], "price": i / 8 if i % 4 else None,
                                "tags": [["a", "b"], [], None, ["c"]][i % 4],
                                "lexical": [{1: 0.5, 7: -2.0}, {}, None, {i: 1.25}][i % 4],
                                "loc": None if i % 5 == 0 else (i - 20.0, 3.0 * i - 60.0)})
               for i in range(40)]
    for i, v in enumerate(vectors):
        v._id = uuid.UUID(int=7000 + i)  # (ids are random by default: fixed here, the files are hashed)
    index.add(vectors[:25], "ns")
    index.add(vectors[25:], "ns")
    index.remove([v.id for v in vectors[::9]], "ns")
    if version == "v4":
        index.update_attributes([vectors[1].id, vectors[2].id], [{"lexical": {3: 4.0}}, {"tags": None}], "ns")
    return index
