"""``Index``: MLVectorDB's per-namespace kNN index, backed by an exhaustive MI355X scan.

Drop-in for the reference's ``Index`` (src/mlvectordb/implementations/index.py:17-165): same
constructor, same four Protocol methods (interfaces/index.py:9-13), same ``is_rebuild_required``
and ``_space`` that ``QueryProcessor.delete`` reads (query_processor.py:58-61).  Where the
reference hands rows to an ``hnswlib.Index`` per namespace, this class hands them to a
``ScanEngine`` per namespace -- in production ``HipScanEngine`` (one ``mlvdb_index`` in HBM).
This side owns only what the reference's Python owns: UUID<->label maps, float32 coercion
(index.py:108), top-k clamping (:107), tombstone accounting (:84-89,103-105), and the
``1 - d`` flip (:126-127).

Behaviour kept from the reference: Q1/Q2 the ``metric`` argument of
``search`` never changes the space searched, it only flips the score; Q5 unknown / empty
namespace -> ``[]`` and top_k clamps to the live count; Q7 queries may be lists or float64.
Not kept: Q3 the 10,000-row cap (capacity is HBM-bound).  A query of the wrong
dimensionality returns ``[]`` exactly as the reference does (hnswlib's RuntimeError is
swallowed by index.py:110-119); rows of the wrong dimensionality raise ``RuntimeError``.

Additive (no reference counterpart): ``search_many`` (one scan for a whole query batch),
``range_search`` / ``range_search_many``, ``metric="euclidean"`` as sqrt(l2), ``compact`` and
``save_index`` / ``load_index`` (named in the reference's README.md:240-241 only); metadata filters evaluated on the device
(``attributes=`` / ``where=`` / ``count`` / ``query_by_metadata``: README.md:121,130,252,274 intent, no reference code) and
aggregated there (``facets`` / ``histogram``).
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from collections.abc import Sequence as SequenceABC
from typing import Callable, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple
from uuid import UUID

import numpy as np

from . import _native
from . import cluster as _cluster
from . import join as _join
from . import score as _score
from . import stats as _stats
from . import where as _where
from .engine import FacetOverflow, HipScanEngine, JoinOverflow, ScanEngine, StatsOverflow
from .idtable import IdTable, mint_uuid4_bytes
from .interfaces import VectorDTO, VectorProtocol

_SPACE_ALIASES = {"l2": "l2", "cosine": "cosine", "ip": "ip", "euclidean": "l2"}


@dataclass
class SearchResult:
    vector_id: UUID
    score: float


class _Namespace:
    """Host-side bookkeeping for one namespace (reference index.py:19-29, per key)."""

    __slots__ = ("engine", "dim", "ids", "total", "deleted", "rebuild_required", "strings")

    def __init__(self, engine: ScanEngine, dim: int) -> None:
        self.engine = engine
        self.dim = dim
        self.ids = IdTable()  # label <-> UUID (arrays, not dicts: idtable.py)
        self.total = 0
        self.deleted = 0
        self.rebuild_required = False
        self.strings: Dict[str, Dict[str, int]] = {}  # str attribute -> {value: dictionary code} (codes in order of first use)


class BatchHits(SequenceABC):
    """What ``search_many`` returns: a sequence of ``nq`` hit lists (entry ``i`` is exactly what ``search`` returns for
    query ``i``) whose ``SearchResult`` objects are only built when an entry is read.  The arrays behind it are public,
    so a batched caller (``QueryProcessor.find_similar_many``) never pays a Python object per hit it does not look at:

    ``labels``  int64 [nq, k]   row labels, -1 = padding
    ``scores``  float64 [nq, k] the post-processed score (``1 - d`` for metric "cosine", index.py:125-127)
    ``counts``  int32 [nq]      valid prefix of each row
    ``ids()``   object [nq, k]  ``uuid.UUID`` per hit (``None`` at padding)
    """

    __slots__ = ("labels", "scores", "counts", "_table", "_ids", "_rows")

    def __init__(self, labels: np.ndarray, scores: np.ndarray, counts: np.ndarray, table: Optional[IdTable]) -> None:
        self.labels, self.scores, self.counts = labels, scores, counts
        self._table = table
        self._ids: Optional[np.ndarray] = None
        self._rows: Dict[int, List[SearchResult]] = {}

    @classmethod
    def empty(cls, nq: int) -> "BatchHits":
        return cls(np.full((nq, 0), -1, dtype=np.int64), np.zeros((nq, 0)), np.zeros(nq, dtype=np.int32), None)

    def valid(self) -> np.ndarray:
        """bool [nq, k]: which slots hold a hit."""
        return np.arange(self.labels.shape[1])[None, :] < self.counts[:, None]

    def id_bytes(self) -> np.ndarray:
        """uint8 [nq, k, 16]: the hits' UUID bytes (zeros at padding); no Python object per hit."""
        if self._table is None:
            return np.zeros(self.labels.shape + (16,), dtype=np.uint8)
        v = self.valid()
        out = self._table.raw[np.where(v, self.labels, 0)]
        out[~v] = 0
        return out

    def handles(self) -> np.ndarray:
        """int64 [nq, k]: the caller's per-row payload given to ``add_arrays`` (-1 = none / padding)."""
        if self._table is None:
            return np.full(self.labels.shape, -1, dtype=np.int64)
        v = self.valid()
        return np.where(v, self._table.handles[np.where(v, self.labels, 0)], -1)

    def ids(self) -> np.ndarray:
        if self._ids is None:
            valid = np.arange(self.labels.shape[1])[None, :] < self.counts[:, None]
            lab = np.where(valid, self.labels, -1)
            self._ids = (self._table.uuids_at(lab) if self._table is not None
                         else np.full(self.labels.shape, None, dtype=object))
        return self._ids

    def __len__(self) -> int:
        return int(self.labels.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        row = self._rows.get(i)
        if row is None:
            n = int(self.counts[i])
            row = [SearchResult(vector_id=u, score=s)
                   for u, s in zip(self.ids()[i, :n].tolist(), self.scores[i, :n].tolist()) if u is not None]
            self._rows[i] = row
        return row

    def __eq__(self, other) -> bool:
        if isinstance(other, (list, BatchHits)):
            return len(self) == len(other) and all(a == b for a, b in zip(self, other))
        return NotImplemented


class ScoredBatchHits(BatchHits):
    """What ``search_scored`` returns: ``BatchHits`` whose ``scores`` are the fp64 values of the score formula (lower is
    better, as computed), plus

    ``distances``  float64 [nq, k]  the hits' raw fp64 distances in the index's space (+inf at padding)
    """

    __slots__ = ("distances",)

    def __init__(self, labels, scores, counts, table, distances: np.ndarray) -> None:
        super().__init__(labels, scores, counts, table)
        self.distances = distances

    @classmethod
    def empty(cls, nq: int) -> "ScoredBatchHits":
        return cls(np.full((nq, 0), -1, dtype=np.int64), np.zeros((nq, 0)), np.zeros(nq, dtype=np.int32), None,
                   np.zeros((nq, 0)))


class TieredBatchHits(BatchHits):
    """What ``search_examples`` / ``search_discover`` return: ``BatchHits`` ranked by (tier, value), plus

    ``tiers``   int32 [nq, k]    the hits' tiers (INT32_MAX at padding), lower first
    ``values``  float64 [nq, k]  the hits' values inside their tier, as computed (+inf at padding), lower first

    ``scores`` is ``values``: a distance of the index's space (or a sum of such differences), never ``1 - d``.
    """

    __slots__ = ("tiers", "values")

    def __init__(self, labels, tiers: np.ndarray, values: np.ndarray, counts, table) -> None:
        super().__init__(labels, values, counts, table)
        self.tiers, self.values = tiers, values

    @classmethod
    def empty(cls, nq: int) -> "TieredBatchHits":
        return cls(np.full((nq, 0), -1, dtype=np.int64), np.zeros((nq, 0), dtype=np.int32), np.zeros((nq, 0)),
                   np.zeros(nq, dtype=np.int32), None)


class GroupedBatchHits(BatchHits):
    """What ``search_many(distinct=..., group_size=...)`` returns: ``BatchHits`` whose rows hold, per query, the groups in rank
    order and each group's members in order, compacted (``counts`` is the total, the valid prefix as everywhere), plus what
    splits the flat list again:

    ``group_sizes``   int32 [nq, k]   members returned per group (0 at padding)
    ``group_values``  object [nq, k]  the groups' values decoded (``str`` / ``bool`` / ``int``; ``None`` at padding)
    """

    __slots__ = ("group_sizes", "group_values")

    def __init__(self, labels, scores, counts, table, group_sizes: np.ndarray, group_values: np.ndarray) -> None:
        super().__init__(labels, scores, counts, table)
        self.group_sizes, self.group_values = group_sizes, group_values

    @classmethod
    def empty(cls, nq: int) -> "GroupedBatchHits":
        return cls(np.full((nq, 0), -1, dtype=np.int64), np.zeros((nq, 0)), np.zeros(nq, dtype=np.int32), None,
                   np.zeros((nq, 0), dtype=np.int32), np.full((nq, 0), None, dtype=object))


class HybridBatchHits(BatchHits):
    """What ``search_hybrid(components=True)`` returns: ``BatchHits`` whose ``scores`` is the fused score, plus what it was
    fused from:

    ``dense``        float64 [nq, k]  the hit's distance to the dense query (+inf at padding)
    ``sparse``       float64 [nq, k]  its sparse score (-inf at padding)
    ``rank_dense``   int32 [nq, k]    its position among the dense candidates, -1: only the sparse leg found it
    ``rank_sparse``  int32 [nq, k]    its position among the sparse candidates, -1: only the dense leg found it
    """

    __slots__ = ("dense", "sparse", "rank_dense", "rank_sparse")

    def __init__(self, labels, scores, counts, table, dense, sparse, rank_dense, rank_sparse) -> None:
        super().__init__(labels, scores, counts, table)
        self.dense, self.sparse, self.rank_dense, self.rank_sparse = dense, sparse, rank_dense, rank_sparse

    @classmethod
    def empty(cls, nq: int) -> "HybridBatchHits":
        return cls(np.full((nq, 0), -1, dtype=np.int64), np.zeros((nq, 0)), np.zeros(nq, dtype=np.int32), None,
                   np.zeros((nq, 0)), np.zeros((nq, 0)), np.zeros((nq, 0), dtype=np.int32), np.zeros((nq, 0), dtype=np.int32))


@dataclass
class DocumentResult:
    value: object  # the document: the decoded value of the ``by`` attribute (``str`` / ``bool`` / ``int``)
    score: float
    matches: Optional[List[SearchResult]] = None  # with ``matches=True``: the document's best row per query token, in token order


class LateBatchHits(SequenceABC):
    """What ``search_late`` returns: a sequence of ``nq`` document lists in rank order whose ``DocumentResult`` objects are
    only built when an entry is read.  The arrays behind it are public:

    ``values``        object [nq, k]   the documents' values decoded (``None`` at padding)
    ``scores``        float64 [nq, k]  the summed score (sum of cosines for metric "cosine", else the summed distance)
    ``counts``        int32 [nq]       valid prefix of each row
    ``offsets``       int64 [nq + 1]   query ``i`` owns token rows ``offsets[i] .. offsets[i + 1]`` of the two below
    ``match_labels``  int64 [tokens, k]   with ``matches=True``: the label of the best row of the query's ``j``-th document for
                                          the token (-1 = padding); else ``None``
    ``match_scores``  float64 [tokens, k] that pair's score (``1 - d`` for metric "cosine"); else ``None``
    """

    __slots__ = ("values", "scores", "counts", "offsets", "match_labels", "match_scores", "_table", "_rows")

    def __init__(self, values, scores, counts, offsets, table: Optional[IdTable], match_labels=None, match_scores=None) -> None:
        self.values, self.scores, self.counts, self.offsets = values, scores, counts, offsets
        self.match_labels, self.match_scores = match_labels, match_scores
        self._table = table
        self._rows: Dict[int, List[DocumentResult]] = {}

    @classmethod
    def empty(cls, lengths: Sequence[int], k: int = 0, matches: bool = False) -> "LateBatchHits":
        nq = len(lengths)
        offsets = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)
        ntok = int(offsets[-1])
        return cls(np.full((nq, k), None, dtype=object), np.full((nq, k), np.inf), np.zeros(nq, dtype=np.int32), offsets, None,
                   np.full((ntok, k), -1, dtype=np.int64) if matches else None, np.full((ntok, k), np.inf) if matches else None)

    def match_ids(self, i: int) -> Optional[np.ndarray]:
        """object [T_i, counts[i]]: the UUIDs of query ``i``'s matched rows (``None`` without ``matches=True``)."""
        if self.match_labels is None:
            return None
        lab = self.match_labels[int(self.offsets[i]):int(self.offsets[i + 1]), :int(self.counts[i])]
        return self._table.uuids_at(lab) if self._table is not None else np.full(lab.shape, None, dtype=object)

    def __len__(self) -> int:
        return int(self.counts.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        row = self._rows.get(i)
        if row is None:
            n = int(self.counts[i])
            ids = self.match_ids(i)
            t0, t1 = int(self.offsets[i]), int(self.offsets[i + 1])
            row = []
            for j, (v, sc) in enumerate(zip(self.values[i, :n].tolist(), self.scores[i, :n].tolist())):
                found = None if ids is None else [SearchResult(vector_id=u, score=float(ms)) for u, ms in
                                                  zip(ids[:, j].tolist(), self.match_scores[t0:t1, j].tolist())]
                row.append(DocumentResult(value=v, score=sc, matches=found))
            self._rows[i] = row
        return row


EngineFactory = Callable[[int, str], ScanEngine]


class Index:
    def __init__(self, space: str = "l2", ef_construction: int = 200, M: int = 16,
                 rebuild_threshold: float = 0.2, *, device: int = 0, devices: Optional[Sequence[int]] = None,
                 strategy: str = "auto", capacity_hint: int = 0,
                 engine_factory: Optional[EngineFactory] = None, attributes: Optional[Mapping[str, str]] = None) -> None:
        # ef_construction / M are HNSW build knobs (index.py:18,37); an exhaustive scan has none.
        self._space = space
        self._ef_construction = ef_construction
        self._M = M
        self._rebuild_threshold = float(rebuild_threshold)
        self._device = device
        # devices=[0, 1, ...]: every namespace is row-sharded over these GPUs inside this one process (SURVEY 8e,
        # multi_device.py); a device may be listed more than once (logical shards on one GPU)
        self._devices = None if devices is None else [int(x) for x in devices]
        self._strategy = strategy
        self._capacity_hint = int(capacity_hint)  # rows to reserve per namespace (and shard) up front: no regrowth copies
        self._engine_factory = engine_factory
        self._ns: Dict[str, _Namespace] = {}
        # attributes={"genre": "str", "year": "int", ...}: per-row metadata columns in HBM, filtered on the device (where.py);
        # attribute i (declaration order) is the engine's column i
        self._attributes: Dict[str, str] = self._check_schema(attributes or {})
        if self._attributes:
            self._refuse_sharded("attributes=")

    @staticmethod
    def _check_schema(attributes: Mapping[str, str]) -> Dict[str, str]:
        attributes = dict(attributes)
        if len(attributes) > _where.MAX_ATTRS:
            raise ValueError(f"at most {_where.MAX_ATTRS} attributes per index (got {len(attributes)})")
        for name, kind in attributes.items():
            if not isinstance(name, str) or name.startswith("$"):
                raise ValueError(f"attribute name {name!r}: a string not starting with '$'")
            known = _where.ATTR_TYPES + _where.LIST_TYPES + _where.SPARSE_TYPES + _where.GEO_TYPES
            if kind not in known and not _where.is_bits(kind):
                raise ValueError(f"attribute {name!r}: type {kind!r} is not one of {known + _where.BITS_TYPES} "
                                 f"(N a multiple of 64 in [64, {64 * _where.BITS_MAX_WORDS}])")
        return attributes

    @property
    def attributes(self) -> Dict[str, str]:
        return dict(self._attributes)

    # ------------------------------------------------------------------ internals
    def _new_engine(self, dim: int, space: str) -> ScanEngine:
        native_space = _SPACE_ALIASES.get(space)
        if native_space is None:
            raise RuntimeError(f"Space name must be one of l2, ip, cosine or euclidean (got {space!r})")
        if self._devices is not None and len(self._devices) > 1:
            from .multi_device import MultiDeviceEngine

            factory = self._engine_factory
            per_shard = -(-self._capacity_hint // len(self._devices))
            return MultiDeviceEngine(dim, native_space, self._devices, strategy=self._strategy, capacity_hint=per_shard,
                                     shard_factory=None if factory is None else (lambda dev: factory(dim, native_space)))
        if self._engine_factory is not None:
            return self._engine_factory(dim, native_space)
        device = self._devices[0] if self._devices else self._device
        return HipScanEngine(dim, native_space, device=device, strategy=self._strategy,
                             capacity_hint=self._capacity_hint)

    def _get_or_create(self, namespace: str, dim: int, space: str) -> _Namespace:
        ns = self._ns.get(namespace)
        if ns is None:
            ns = _Namespace(self._new_engine(dim, space), dim)
            for i, kind in enumerate(self._attributes.values()):
                ns.engine.define_attr(i, _where.column_kind(kind))
            self._ns[namespace] = ns
        return ns

    # ------------------------------------------------------------------ attributes
    def _stage_attrs(self, namespace: str, columns: Mapping[str, Sequence], n: int):
        """Encode a batch's attribute values (``columns``: name -> n values, ``None`` = absent) -> (column index -> array,
        the namespace's string dictionaries with the batch's new strings).  Raises ``ValueError`` before anything is mutated."""
        if not self._attributes:
            if columns:
                raise ValueError(f"this index declares no attributes (got {sorted(columns)})")
            return {}, None
        for name in columns:
            self._declared(name)
        ns = self._ns.get(namespace)
        strings = {name: dict(codes) for name, codes in (ns.strings if ns is not None else {}).items()}
        out = {}
        for i, (name, kind) in enumerate(self._attributes.items()):
            values = columns.get(name)
            if values is None:
                continue
            if len(values) != n:
                raise ValueError(f"attribute {name!r}: {len(values)} values for {n} rows")
            if _where.is_list(kind):
                col = _where.encode_list_column(name, kind, values, strings.setdefault(name, {}) if kind == "str[]" else {})
                if col.present.any():
                    out[i] = col
                continue
            if _where.is_sparse(kind):
                col = _where.encode_sparse_column(name, values)
                if col.present.any():
                    out[i] = col
                continue
            if _where.is_bits(kind):
                col = _where.encode_bits_column(name, kind, values)
                if col.present.any():
                    out[i] = col
                continue
            col = _where.encode_column(name, kind, values, strings.setdefault(name, {}) if kind == "str" else {})
            present = ~np.isnan(col) if col.dtype == np.float64 else col != _where.INT64_ABSENT
            if present.any():
                out[i] = col
        return out, strings

    # ------------------------------------------------------------------ what the entry families share
    # Each refusal takes ``what``, the words its message starts with; the entries call them in the order they refuse in.
    def _refuse_sharded(self, what: str) -> None:
        if self._devices is not None and len(self._devices) > 1:
            raise ValueError(f"{what} is not supported on a row-sharded index (devices=[...] with more than one entry)")

    def _declared(self, name, what: str = "") -> str:
        """The type of the declared attribute ``name``."""
        if not isinstance(name, str) or name not in self._attributes:
            raise ValueError(f"{what}{name!r} is not a declared attribute of this index (declared: {sorted(self._attributes)})")
        return self._attributes[name]

    def _column(self, name: str) -> int:
        """The engine's column of the declared attribute ``name``."""
        return list(self._attributes).index(name)

    @staticmethod
    def _engine_entry(ns: _Namespace, method: str, subject: str, named: Optional[str] = None):
        """The engine's ``method``; ``subject`` is who asks ("top_by needs", "list attributes need")."""
        fn = getattr(ns.engine, method, None)
        if fn is None:
            raise ValueError(f"{subject} an engine with {named or method} (a single-device namespace)")
        return fn

    @staticmethod
    def _one_filter(what: str, where) -> None:
        if where is not None and not isinstance(where, Mapping):
            raise ValueError(f"{what}: where must be one dict filter or None (got {type(where).__name__})")

    @staticmethod
    def _no_where_list(what: str, where, allowed_ids=None) -> None:
        """The older families' form of ``_one_filter``: they name what they refuse and leave other types to ``_compile``."""
        if isinstance(where, (list, tuple)):
            raise ValueError(f"{what}: a per-query where list is not supported, give one dict filter")
        if allowed_ids is not None:
            raise ValueError(f"{what}: allowed_ids is not supported, give a dict where filter")

    def _program(self, namespace: str, where) -> Optional["_where.Program"]:
        return None if where is None else self._compile(namespace, where)

    @staticmethod
    def _nothing_to_search(ns: Optional[_Namespace], top_k=1, nq: int = 1, dim: Optional[int] = None) -> bool:
        """The empty answer is due: no live row, no neighbour asked for, no query, or queries of another dimensionality."""
        return ns is None or ns.total - ns.deleted <= 0 or top_k <= 0 or nq == 0 or (dim is not None and dim != ns.dim)

    @staticmethod
    def _no_rows(ns: Optional[_Namespace]) -> bool:
        """Nothing for a metadata query to read (tombstoned rows still count: the engine holds their columns)."""
        return ns is None or ns.total == 0

    @staticmethod
    def _int_in(value, lo: int, hi: Optional[int] = None) -> bool:
        """``value`` is an int, not a bool, in [lo, hi]."""
        return (not isinstance(value, bool) and isinstance(value, (int, np.integer)) and lo <= value
                and (hi is None or value <= hi))

    def _check_window(self, what: str, limit, offset) -> None:
        if not self._int_in(limit, 1):
            raise ValueError(f"{what}: limit must be an int >= 1 (got {limit!r})")
        if not self._int_in(offset, 0):
            raise ValueError(f"{what}: offset must be an int >= 0 (got {offset!r})")
        if int(offset) + int(limit) > self._MAX_ORDER_ROWS:
            raise ValueError(f"{what}: offset + limit must be <= {self._MAX_ORDER_ROWS} (got {int(offset) + int(limit)})")

    @staticmethod
    def _group_bound(ns: _Namespace, name: str, kind: str, other: int) -> int:
        """What the host knows about the number of values of attribute ``name``: the dictionary's size, two booleans,
        ``other`` for integers."""
        return len(ns.strings.get(name, {})) if kind in ("str", "str[]") else 2 if kind == "bool" else other

    @staticmethod
    def _decode_codes(ns: _Namespace, name: str, kind: str, codes: list) -> list:
        """Column values of attribute ``name`` decoded: the strings of its dictionary, ``True`` / ``False``, ints."""
        if kind in ("str", "str[]"):
            known = ns.strings.get(name, {})
            strings = sorted(known, key=known.get)  # code order
            return [strings[c] for c in codes]
        return [bool(c) for c in codes] if kind == "bool" else codes

    @staticmethod
    def _sparse_queries(queries: list, what: str) -> "_where.SparseColumn":
        """Sparse query vectors as one column; query ``i`` is refused as ``{what} i``."""
        offsets = np.zeros(len(queries) + 1, dtype=np.int64)
        terms: List[int] = []
        weights: List[float] = []
        for i, q in enumerate(queries):
            t, w = _where.encode_sparse_vector(q, f"{what} {i}", _where.SPARSE_MAX_QUERY_TERMS)
            terms.extend(t)
            weights.extend(w)
            offsets[i + 1] = len(terms)
        return _where.SparseColumn(offsets, np.array(terms, dtype=np.int32), np.array(weights, dtype=np.float32),
                                   np.ones(len(queries), dtype=np.uint8))

    def _check_sparse(self, what: str, name: str) -> None:
        if _where.is_sparse(self._attributes[name]):
            raise ValueError(f"{what}: attribute {name!r} is a sparse column; it needs a scalar attribute "
                             f"(a sparse vector is searched with search_sparse)")
        if _where.is_geo(self._attributes[name]):
            raise ValueError(f"{what}: attribute {name!r} is a geo column; it needs a scalar attribute (a location is "
                             f"filtered with $geo_radius / $geo_box and ranked with nearest)")
        if _where.is_bits(self._attributes[name]):
            raise ValueError(f"{what}: attribute {name!r} is a {self._attributes[name]} column; it needs a scalar attribute "
                             f"(a bit code is searched with search_bits)")

    def _check_scalar(self, what: str, name: str) -> None:
        self._check_sparse(what, name)
        if _where.is_list(self._attributes[name]):
            raise ValueError(f"{what}: attribute {name!r} is a {self._attributes[name]} column; it needs a scalar attribute "
                             f"(a list has no one value to rank, bin or group by)")

    def _metadata_columns(self, metadata: Sequence[Optional[Mapping]]) -> Dict[str, list]:
        """The declared attributes' values out of per-row metadata dicts (missing key / no metadata = absent)."""
        return {name: [None if m is None else m.get(name) for m in metadata] for name in self._attributes}

    def extract_attributes(self, metadata: Sequence[Optional[Mapping]]) -> Dict[str, list]:
        """Columnar ``attributes=`` for ``add_arrays`` out of per-row metadata dicts (``QueryProcessor.upsert_arrays``)."""
        return self._metadata_columns(metadata)

    @staticmethod
    def _commit_attrs(ns: _Namespace, first: int, staged) -> None:
        cols, strings = staged
        for i, col in cols.items():
            if isinstance(col, _where.ListColumn):
                Index._engine_entry(ns, "set_attr_list", "list attributes need")(i, first, col)
            elif isinstance(col, _where.SparseColumn):
                Index._engine_entry(ns, "set_attr_sparse", "sparse attributes need")(i, first, col)
            elif isinstance(col, _where.BitsColumn):
                Index._engine_entry(ns, "bits_set", "bits attributes need")(i, first, col)
            else:
                ns.engine.set_attr(i, first, col)
        if strings is not None:
            ns.strings = strings

    def _compile(self, namespace: str, where) -> "_where.Program":
        if not isinstance(where, Mapping):
            raise ValueError(f"where must be a dict filter (where.py), got {type(where).__name__}")
        ns = self._ns.get(namespace)
        return _where.compile_where(where, self._attributes, ns.strings if ns is not None else {})

    @staticmethod
    def _stack_rows(vectors: Sequence[VectorProtocol], dim: int) -> np.ndarray:
        try:  # one C-level pass when every row has the right shape (the only case that succeeds)
            rows = np.asarray([v.values for v in vectors], dtype=np.float32)
            if rows.shape == (len(vectors), dim):
                return rows
        except ValueError:
            pass
        for i, v in enumerate(vectors):
            vals = np.asarray(v.values, dtype=np.float32)
            if vals.shape != (dim,):
                raise RuntimeError(f"Wrong dimensionality of the vectors: row {i} has shape {vals.shape}, index dim {dim}")
        raise RuntimeError(f"Wrong dimensionality of the vectors: expected [{len(vectors)}, {dim}]")

    @staticmethod
    def _check_finite(rows: np.ndarray) -> None:
        # A non-finite row would get a NaN norm, which the scan kernels read as "tombstoned": the row would vanish from
        # every search without being counted as deleted.  hnswlib accepts such rows and returns garbage; this index
        # refuses them.
        if not np.isfinite(rows).all():
            bad = int(np.flatnonzero(~np.isfinite(rows).all(axis=1))[0])
            raise RuntimeError(f"row {bad} of the batch holds a non-finite value (NaN / inf): not indexable")

    @staticmethod
    def _check_ids(vectors: Sequence[VectorProtocol]) -> List[UUID]:
        # the id table stores 16 bytes per row: anything else (SimpleVector("abc", ...)) is refused BEFORE the rows
        # reach the engine, so a bad batch leaves the namespace exactly as it was
        ids = [v.id for v in vectors]
        for i, u in enumerate(ids):
            if not isinstance(u, UUID):
                raise RuntimeError(f"row {i} of the batch has id {u!r}: this index keys rows by uuid.UUID")
        return ids

    def _stage(self, vectors: Sequence[VectorProtocol], dim: int):
        """Everything that can refuse a batch, before anything is mutated: (rows float32 [n, dim], ids)."""
        for i, v in enumerate(vectors):
            if getattr(v, "values", None) is None:
                raise RuntimeError(f"row {i} of the batch carries no values (a storage row whose values live in HBM only)")
        rows = self._stack_rows(vectors, dim)
        self._check_finite(rows)
        return rows, self._check_ids(vectors)

    def _append(self, ns: _Namespace, vectors: Sequence[VectorProtocol], staged=None) -> None:
        rows, ids = staged if staged is not None else self._stage(vectors, ns.dim)
        first = ns.engine.append(rows)
        if first != ns.total or ns.ids.append_uuids(ids) != first:
            raise RuntimeError(f"engine label base {first} != host row count {ns.total}")
        ns.total += len(ids)

    # ------------------------------------------------------------------ IndexProtocol
    def add(self, vectors: Iterable[VectorProtocol], namespace: str) -> None:
        """Append rows; labels continue from the namespace's row count (index.py:50-67)."""
        vectors = list(vectors)
        if not vectors:
            return
        known = self._ns.get(namespace)
        dim = known.dim if known is not None else int(np.asarray(vectors[0].values).shape[0])
        staged = self._stage(vectors, dim)  # a refused batch creates no namespace and appends nothing
        attrs = self._stage_attrs(namespace, self._metadata_columns([getattr(v, "metadata", None) for v in vectors]),
                                  len(vectors)) if self._attributes else None
        ns = self._get_or_create(namespace, dim, self._space)
        first = ns.total
        self._append(ns, vectors, staged)
        if attrs is not None:
            self._commit_attrs(ns, first, attrs)

    def validate_arrays(self, rows: np.ndarray, namespace: str, handles: Optional[np.ndarray] = None,
                        attributes: Optional[Mapping[str, Sequence]] = None) -> None:
        """Raises what ``add_arrays`` would raise for this batch, without touching the index: a caller that writes to a
        second store first (``QueryProcessor.upsert_arrays``) checks here before it writes anything."""
        if rows.ndim != 2:
            raise RuntimeError(f"Wrong dimensionality of the vectors: expected a matrix, got shape {rows.shape}")
        ns = self._ns.get(namespace)
        if ns is not None and rows.shape[0] and rows.shape[1] != ns.dim:
            raise RuntimeError(f"Wrong dimensionality of the vectors: got {rows.shape}, index dim {ns.dim}")
        if handles is not None and np.asarray(handles).shape != (rows.shape[0],):
            raise RuntimeError(f"{rows.shape[0]} rows but handles of shape {np.asarray(handles).shape}")
        self._check_finite(rows)
        if attributes is not None:
            self._stage_attrs(namespace, attributes, rows.shape[0])

    def add_arrays(self, rows: np.ndarray, namespace: str, ids: Optional[np.ndarray] = None,
                   handles: Optional[np.ndarray] = None, attributes: Optional[Mapping[str, Sequence]] = None) -> np.ndarray:
        """Additive bulk form of ``add``: ``rows`` is a float ``[n, dim]`` matrix, ``ids`` an optional ``[n, 16] uint8``
        table of UUID bytes (minted as uuid4 when omitted), ``handles`` an optional int64 payload per row that comes
        back with every hit (``BatchHits.handles``: a storage row number), ``attributes`` optional columnar values of the
        declared attributes (name -> n values: an array, or a list with ``None`` for absent).  No Python object per row
        is created; returns the id table.  Same label rule as ``add`` (index.py:56-63)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2:
            raise RuntimeError(f"Wrong dimensionality of the vectors: expected a matrix, got shape {rows.shape}")
        n = rows.shape[0]
        ids = mint_uuid4_bytes(n) if ids is None else np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 16)
        if ids.shape[0] != n:
            raise RuntimeError(f"{n} rows but {ids.shape[0]} ids")
        if n == 0:
            return ids
        self.validate_arrays(rows, namespace, handles)  # every refusal happens before the engine is touched
        attrs = self._stage_attrs(namespace, attributes or {}, n) if (attributes or self._attributes) else None
        ns = self._get_or_create(namespace, rows.shape[1], self._space)
        first = ns.engine.append(rows)
        if first != ns.total or ns.ids.append_raw(ids, handles) != first:
            raise RuntimeError(f"engine label base {first} != host row count {ns.total}")
        ns.total += n
        if attrs is not None:
            self._commit_attrs(ns, first, attrs)
        return ids

    def remove(self, ids: Sequence[UUID], namespace: str) -> None:
        """Tombstone rows; raise the rebuild flag at deleted/total >= threshold (index.py:69-89)."""
        ns = self._ns.get(namespace)
        if ns is None:
            return
        labels = ns.ids.lookup(ids)
        labels = np.unique(labels[labels >= 0])
        if labels.size:
            ns.engine.tombstone(labels)
            ns.ids.kill(labels)
        ns.deleted += int(labels.size)
        if ns.deleted / max(1, ns.total) >= self._rebuild_threshold:
            ns.rebuild_required = True

    def search(self, query: VectorDTO, top_k: int, namespace: str, metric: str) -> List[SearchResult]:
        """Single-query kNN (index.py:91-129); one-row case of ``search_many``."""
        values = np.asarray(query.values, dtype=np.float32)
        if values.ndim != 1:
            return []
        return self.search_many(values[None, :], top_k, namespace, metric)[0]

    def rebuild(self, source: Mapping[str, Iterable[VectorProtocol]], metric: str) -> None:
        """Replace *every* namespace by ``source``, searching ``metric`` as the space (index.py:131-162).

        The whole source is staged and validated on the host first (values present, one dimensionality per namespace,
        finite, UUID ids, a known space): a source that cannot be indexed raises and leaves the index as it was --
        closing the engines first would have destroyed the only copy of rows that live in HBM only."""
        if _SPACE_ALIASES.get(metric) is None:
            raise RuntimeError(f"Space name must be one of l2, ip, cosine or euclidean (got {metric!r})")
        staged = []
        for namespace, vectors in source.items():
            vectors = list(vectors)
            if not vectors:
                continue
            if getattr(vectors[0], "values", None) is None:
                raise RuntimeError(f"namespace {namespace!r}: the source rows carry no values")
            dim = int(np.asarray(vectors[0].values).shape[0])
            attrs = None
            if self._attributes:  # (dictionaries start afresh: the namespace is rebuilt from nothing)
                cols = self._metadata_columns([getattr(v, "metadata", None) for v in vectors])
                saved, self._ns = self._ns, {}
                try:
                    attrs = self._stage_attrs(namespace, cols, len(vectors))
                finally:
                    self._ns = saved
            staged.append((namespace, dim, vectors, self._stage(vectors, dim), attrs))
        for ns in self._ns.values():
            ns.engine.close()
        self._ns.clear()
        for namespace, dim, vectors, st, attrs in staged:
            ns = self._get_or_create(namespace, dim, metric)
            self._append(ns, vectors, st)
            if attrs is not None:
                self._commit_attrs(ns, 0, attrs)

    def is_rebuild_required(self, namespace: str) -> bool:
        ns = self._ns.get(namespace)
        return bool(ns and ns.rebuild_required)

    def compact(self, namespace: str) -> bool:
        """Additive: what ``rebuild`` from this namespace's surviving vectors (in insertion order) leaves
        behind -- labels renumbered from 0, tombstones gone, flag cleared (index.py:145-162) -- computed on
        the device from the rows the index already owns, touching no other namespace (quirk Q4) and moving
        nothing over PCIe.  Returns False when the namespace is unknown."""
        ns = self._ns.get(namespace)
        if ns is None:
            return False
        old = ns.engine.compact()  # old[new label] = old label
        ns.ids = ns.ids.take(old)
        ns.total = ns.ids.n
        ns.deleted = 0
        ns.rebuild_required = False
        return True

    # ------------------------------------------------------------------ additive: batches and ranges
    @staticmethod
    def _scores(dist: np.ndarray, metric: str) -> np.ndarray:
        """``Index.search``'s score rule (index.py:125-127) on a whole array: the float32 distance as a Python float
        (= float64), ``1 - d`` for metric "cosine"; additive: the square root for "euclidean"."""
        score = dist.astype(np.float64)
        if metric == "cosine":
            score = 1 - score
        elif metric == "euclidean":
            score = np.sqrt(np.maximum(score, 0.0))
        return score

    def search_many(self, queries, top_k: int, namespace: str, metric: str,
                    allowed_ids: Optional[Iterable[UUID]] = None, where: Optional[Mapping] = None,
                    distinct: Optional[str] = None, mmr_lambda: Optional[float] = None,
                    fetch_k: Optional[int] = None, group_size: Optional[int] = None) -> BatchHits:
        """kNN for a batch of queries in one corpus scan.

        ``queries`` is an ``[nq, dim]`` array or a sequence of ``VectorDTO``.  Each entry of
        the result is what ``search`` would return for that query (``BatchHits``: a lazy sequence over the result
        arrays).  ``allowed_ids`` (additive: the row mask of a metadata-filtered search, README.md:121,130 intent)
        restricts the search to those vectors; the answer is the exact top-k among them.  ``where`` (additive: a dict
        filter over the declared attributes, where.py) does the same with the row mask evaluated on the device; a list or
        tuple of ``nq`` entries, each a dict filter or ``None`` (unfiltered), gives every query its own filter (one batched
        call, include/mlvdb_where_each.h): each query's answer is what a single-dict call for it alone returns.
        ``distinct`` (additive: the name of a declared ``int`` / ``str`` / ``bool`` attribute) returns one hit per value of
        that attribute -- the nearest row of each of the ``top_k`` (<= 64) nearest groups, rows without a value left out
        (include/mlvdb_distinct.h); an optional single dict ``where`` restricts the rows first.
        ``mmr_lambda`` (additive: a number in [0, 1]) diversifies the answer by maximal marginal relevance on the device
        (include/mlvdb_mmr.h): among the ``fetch_k`` nearest vectors (default ``min(1024, max(4 * top_k, 20))``, at most
        1024) the nearest is picked first, then ``top_k`` (<= 64) in all, each minimising ``mmr_lambda * d(query, i) -
        (1 - mmr_lambda) * min over the picks s of d(s, i)`` in the index's distance; 1 is the plain search, 0 pure
        diversity.  Hits come back in pick order with the usual scores; an optional single dict ``where`` restricts the
        rows first.
        ``group_size`` (additive, with ``distinct``: an int in [1, 64]) returns the ``group_size`` nearest rows of each of
        those groups instead of one (include/mlvdb_grouped.h) as a ``GroupedBatchHits``: per query the groups in rank
        order, each group's members in order, ``group_sizes`` / ``group_values`` to split the flat list.
        """
        if group_size is not None and distinct is None:
            raise ValueError("search_many: group_size is the member count of distinct=, give both or neither")
        if mmr_lambda is not None:
            return self._search_many_mmr(queries, top_k, namespace, metric, allowed_ids, where, distinct, mmr_lambda, fetch_k)
        if fetch_k is not None:
            raise ValueError("search_many: fetch_k is the candidate count of mmr_lambda=, give both or neither")
        if distinct is not None:
            return self._search_many_distinct(queries, top_k, namespace, metric, allowed_ids, where, distinct, group_size)
        if where is not None and allowed_ids is not None:
            raise ValueError("search_many: give allowed_ids or where, not both")
        if isinstance(where, (list, tuple)):
            return self._search_many_each(queries, top_k, namespace, metric, where)
        program = self._program(namespace, where)
        q = self._coerce_queries(queries)
        nq = q.shape[0]
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, top_k, nq, q.shape[1]):
            return BatchHits.empty(nq)  # (another dimensionality: the reference swallows the RuntimeError, index.py:110-119)
        active = ns.total - ns.deleted
        mask = None
        if allowed_ids is not None:
            picked = ns.ids.lookup(allowed_ids)
            picked = picked[picked >= 0]
            if not picked.size:
                return BatchHits.empty(nq)
            mask = np.zeros(ns.total, dtype=np.uint8)
            mask[picked] = 1
            active = int(mask.sum())
        k = min(int(top_k), active, self._MAX_TOP_K)  # the reference clamps to the live count (index.py:107)
        if program is not None:  # (counts = min(k, matching rows): the padding says how many matched)
            labels, dist, counts = ns.engine.search(q, k, where=program)
        else:
            labels, dist, counts = self._search_engine(ns, q, k, mask)
        return BatchHits(labels, self._scores(dist, metric), counts, ns.ids)

    _MAX_TOP_K = 16384  # MLVDB_MAX_TOPK_PAGED: the most neighbours one call returns per query

    _MAX_TOP_K_DISTINCT = 64  # MLVDB_MAX_TOPK: one selection list of a wavefront

    _MAX_GROUP_SIZE = 64  # MLVDB_GROUPED_MAX_SIZE: one selection list of a wavefront

    def _search_many_distinct(self, queries, top_k: int, namespace: str, metric: str, allowed_ids, where,
                              distinct: str, group_size: Optional[int] = None) -> BatchHits:
        """``search_many`` with ``distinct=``: every refusal happens before the engine is touched."""
        if group_size is not None and not self._int_in(group_size, 1, self._MAX_GROUP_SIZE):
            raise ValueError(f"group_size must be an int in [1, {self._MAX_GROUP_SIZE}] (got {group_size!r})")
        self._refuse_sharded("distinct=")
        kind = self._declared(distinct, "distinct: ")
        self._check_scalar("distinct", distinct)
        if kind == "float":
            raise ValueError(f"distinct: attribute {distinct!r} is a float column; groups need an int, str or bool attribute")
        if top_k > self._MAX_TOP_K_DISTINCT:
            raise ValueError(f"distinct: top_k must be <= {self._MAX_TOP_K_DISTINCT} (got {top_k})")
        self._no_where_list("distinct", where, allowed_ids)
        program = self._program(namespace, where)
        q = self._coerce_queries(queries)
        nq = q.shape[0]
        ns = self._ns.get(namespace)
        if group_size is not None:
            return self._search_many_grouped(q, top_k, ns, metric, program, distinct, kind, int(group_size))
        if self._nothing_to_search(ns, top_k, nq, q.shape[1]):
            return BatchHits.empty(nq)
        search_distinct = self._engine_entry(ns, "search_distinct", "distinct= needs")
        k = min(int(top_k), ns.total - ns.deleted)
        max_groups = self._group_bound(ns, distinct, kind, 0)  # (nothing is known about integers)
        if kind == "str" and max_groups == 0:
            return BatchHits(np.full((nq, k), -1, np.int64), self._scores(np.full((nq, k), np.inf, np.float32), metric),
                             np.zeros(nq, np.int32), ns.ids)  # no string was ever stored: every row is absent
        labels, dist, counts, _ = search_distinct(q, k, self._column(distinct), max_groups=max_groups, where=program)
        return BatchHits(labels, self._scores(dist, metric), counts, ns.ids)

    def _search_many_grouped(self, q: np.ndarray, top_k: int, ns, metric: str, program, distinct: str, kind: str,
                             g: int) -> "GroupedBatchHits":
        """The validated ``distinct=`` call with ``group_size=``: the engine's [nq, k, g] answer compacted on the host."""
        nq = q.shape[0]
        if self._nothing_to_search(ns, top_k, nq, q.shape[1]):
            return GroupedBatchHits.empty(nq)
        search_grouped = self._engine_entry(ns, "search_grouped", "group_size= needs")
        k = min(int(top_k), ns.total - ns.deleted)
        max_groups = self._group_bound(ns, distinct, kind, 0)
        if kind == "str" and max_groups == 0:  # no string was ever stored: every row is absent
            return GroupedBatchHits(np.full((nq, k * g), -1, np.int64),
                                    self._scores(np.full((nq, k * g), np.inf, np.float32), metric), np.zeros(nq, np.int32),
                                    ns.ids, np.zeros((nq, k), np.int32), np.full((nq, k), None, dtype=object))
        labels, dist, ngroups, sizes, codes = search_grouped(q, k, g, self._column(distinct), max_groups=max_groups,
                                                             where=program)
        # compaction: the valid slots of a query first, in their order (groups by rank, members in order), padding behind
        valid = (np.arange(g)[None, None, :] < sizes[:, :, None]).reshape(nq, k * g)
        order = np.argsort(~valid, axis=1, kind="stable")
        valid = np.take_along_axis(valid, order, axis=1)
        labels = np.where(valid, np.take_along_axis(labels.reshape(nq, k * g), order, axis=1), -1)
        dist = np.where(valid, np.take_along_axis(dist.reshape(nq, k * g), order, axis=1), np.float32(np.inf))
        values = self._decode_groups(ns, distinct, kind, codes, ngroups)
        return GroupedBatchHits(labels, self._scores(dist, metric), sizes.sum(axis=1).astype(np.int32), ns.ids,
                                sizes.astype(np.int32), values)

    @staticmethod
    def _decode_groups(ns, name: str, kind: str, codes: np.ndarray, ngroups: np.ndarray) -> np.ndarray:
        """object [nq, k]: the group codes of attribute ``name`` decoded (``str`` / ``bool`` / ``int``), ``None`` at padding."""
        nq, k = codes.shape
        values = np.full((nq, k), None, dtype=object)
        have = np.arange(k)[None, :] < ngroups[:, None]
        values[have] = Index._decode_codes(ns, name, kind, codes[have].tolist())
        return values

    _MAX_TOP_K_LATE = 64    # MLVDB_MAX_TOPK: one selection list of a wavefront
    _MAX_LATE_TOKENS = 128  # MLVDB_MAXSIM_MAX_TOKENS

    @staticmethod
    def _late_queries(queries) -> List[np.ndarray]:
        """``queries`` of ``search_late`` as one float32 ``[T_i, dim]`` array per query."""
        if isinstance(queries, np.ndarray) and queries.ndim == 3:
            queries = list(queries)
        if isinstance(queries, np.ndarray) or not isinstance(queries, (SequenceABC, np.ndarray)):
            raise ValueError("search_late: queries must be a sequence of [T_i, dim] arrays or one [nq, T, dim] array")
        out = []
        for i, q in enumerate(queries):
            a = np.asarray(q, dtype=np.float32)
            if a.ndim != 2:
                raise ValueError(f"search_late: query {i} must be a [T, dim] array of token vectors (got shape {a.shape})")
            out.append(np.ascontiguousarray(a))
        return out

    def search_late(self, queries, top_k: int, namespace: str, metric: str, by: str, *, where: Optional[Mapping] = None,
                    matches: bool = False, allowed_ids: Optional[Iterable[UUID]] = None) -> LateBatchHits:
        """Additive: late-interaction (MaxSim) search on the device (include/mlvdb_maxsim.h).  A query is a bag of token
        vectors -- ``queries`` is a sequence of ``[T_i, dim]`` arrays (1..128 tokens each) or one ``[nq, T, dim]`` array --
        and a document is one value of the declared ``int`` / ``str`` / ``bool`` attribute ``by`` (rows without a value are
        in no document).  A document's distance is the sum, over the query's tokens in order, of the token's distance to
        the document's nearest live row; the ``top_k`` (<= 64) documents with the smallest sum come back per query, exact,
        ties to the smaller value code.  Scores, from the fp64 sum: the sum of cosines for metric "cosine" (``T_i`` minus
        the summed distance), the summed distance itself for "l2" / "ip"; "euclidean" is refused (a root does not
        distribute over the sum).  ``where`` (one dict filter) restricts the rows first; ``matches=True`` adds, per document
        and token, the matched row and its score.  Every refusal happens before the engine is touched."""
        self._refuse_sharded("search_late")
        if metric == "euclidean":
            raise ValueError('search_late: metric "euclidean" is not supported (a root does not distribute over the sum), use "l2"')
        kind = self._declared(by, "search_late: ")
        self._check_scalar("search_late", by)
        if kind == "float":
            raise ValueError(f"search_late: attribute {by!r} is a float column; documents need an int, str or bool attribute")
        if top_k > self._MAX_TOP_K_LATE:
            raise ValueError(f"search_late: top_k must be <= {self._MAX_TOP_K_LATE} (got {top_k})")
        self._no_where_list("search_late", where, allowed_ids)
        qs = self._late_queries(queries)
        lengths = [int(q.shape[0]) for q in qs]
        ns = self._ns.get(namespace)
        for i, q in enumerate(qs):
            if not 1 <= q.shape[0] <= self._MAX_LATE_TOKENS:
                raise ValueError(f"search_late: query {i} holds {q.shape[0]} tokens, 1 to {self._MAX_LATE_TOKENS} are supported")
            if q.shape[1] != (ns.dim if ns is not None else qs[0].shape[1]):
                raise ValueError(f"search_late: query {i} has token vectors of dim {q.shape[1]}, "
                                 f"expected {ns.dim if ns is not None else qs[0].shape[1]}")
        program = self._program(namespace, where)
        if self._nothing_to_search(ns, top_k, len(qs)):
            return LateBatchHits.empty(lengths, 0, matches)
        search_maxsim = self._engine_entry(ns, "search_maxsim", "search_late needs")
        k = min(int(top_k), ns.total - ns.deleted)
        if kind == "str" and not ns.strings.get(by):  # no string was ever stored: every row is absent
            return LateBatchHits.empty(lengths, k, matches)
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        codes, _, counts, s64, m_lab, m_d64 = search_maxsim(np.concatenate(qs, axis=0), offsets, k, self._column(by),
                                                            where=program, want_matches=bool(matches))
        # the score rule, in fp64 from the fp64 sum: T_i - s is the sum of the tokens' cosines
        scores = np.asarray(lengths, np.float64)[:, None] - s64 if metric == "cosine" else s64.copy()
        scores[np.arange(k)[None, :] >= counts[:, None]] = np.inf
        if m_d64 is not None:
            m_d64 = np.where(m_lab >= 0, 1 - m_d64, np.inf) if metric == "cosine" else m_d64
        return LateBatchHits(self._decode_groups(ns, by, kind, codes, counts), scores, counts, offsets, ns.ids, m_lab, m_d64)

    _MAX_TOP_K_SCORED = 64  # MLVDB_MAX_TOPK: one selection list of a wavefront

    def search_scored(self, queries, top_k: int, namespace: str, metric: str, score, *, where: Optional[Mapping] = None,
                      allowed_ids: Optional[Iterable[UUID]] = None) -> "ScoredBatchHits":
        """Additive: scored kNN on the device (include/mlvdb_score.h) -- the ``top_k`` rows with the smallest value of the
        formula ``score`` (score.py: an expression over ``"$distance"``, ``{"$attr": ..}``, ``{"$match": {..}}`` and
        ``$add $sub $mul $div $min $max $neg $abs``), evaluated in fp64 for every live row -- of those ``where`` (one dict
        filter) matches -- so the answer is exact, with no candidate window.  Rows whose score is NaN (an absent attribute
        without a ``$default``, ``0/0``) are dropped; ties go to the earlier row.  ``scores`` are the formula's values,
        lower is better, returned as computed; ``distances`` the hits' raw fp64 distances.  ``$distance`` is the index's
        distance -- the squared distance for "l2", ``1 - cosine`` for "cosine" -- so metric "euclidean" is refused: use
        "l2".  ``top_k`` is clamped to the live row count and to 64.  Recipes:

            bonus               {"$sub": ["$distance", {"$mul": [0.2, {"$match": {"tier": "gold"}}]}]}
            popularity          {"$div": ["$distance", {"$add": [1, {"$attr": "likes", "$default": 0}]}]}
            linear age penalty  {"$add": ["$distance", {"$mul": [0.3, {"$min": [1, {"$div": [{"$abs": {"$sub": [
                                    {"$attr": "year"}, 2024]}}, 10]}]}]}]}

        Every refusal happens before the engine is touched."""
        self._refuse_sharded("search_scored")
        if metric == "euclidean":
            raise ValueError('search_scored: metric "euclidean" is not supported ($distance is the squared distance), use "l2"')
        self._no_where_list("search_scored", where, allowed_ids)
        ns = self._ns.get(namespace)
        program = _score.compile_score(score, self._attributes, ns.strings if ns is not None else {})
        where_program = self._program(namespace, where)
        q = self._coerce_queries(queries)
        nq = q.shape[0]
        if self._nothing_to_search(ns, top_k, nq, q.shape[1]):
            return ScoredBatchHits.empty(nq)
        search = self._engine_entry(ns, "search_scored", "search_scored needs")
        k = min(int(top_k), ns.total - ns.deleted, self._MAX_TOP_K_SCORED)
        labels, scores, counts, d64 = search(q, k, program, where=where_program, want64=True)
        return ScoredBatchHits(labels, scores, counts, ns.ids, d64)

    _MAX_TOP_K_SPARSE = 64  # MLVDB_MAX_TOPK: one selection list of a wavefront

    def search_sparse(self, queries, top_k: int, namespace: str, by: str, *, where: Optional[Mapping] = None) -> BatchHits:
        """Additive: exact lexical kNN over the declared ``sparse`` attribute ``by`` on the device
        (include/mlvdb_sparse.h).  ``queries`` is a sequence of sparse vectors -- each a mapping ``{term: weight}`` or a pair
        ``(indices, values)``, at most 1024 nonzeros, typed as at ingest -- and every live row that holds a vector (an empty
        one included) is a candidate; ``where`` (one dict filter) restricts the rows first.  Per query the ``top_k`` rows
        with the largest inner product come back, ties to the earlier row; ``scores`` is the fp64 dot product.  ``top_k`` is
        clamped to the live row count and to 64.  Every refusal happens before the engine is touched."""
        self._refuse_sharded("search_sparse")
        if not _where.is_sparse(self._declared(by, "search_sparse: ")):
            raise ValueError(f"search_sparse: attribute {by!r} is a {self._attributes[by]} column; it needs a sparse attribute")
        self._one_filter("search_sparse", where)
        if isinstance(queries, Mapping) or isinstance(queries, (str, bytes)):
            raise ValueError("search_sparse: queries is a sequence of sparse vectors (got one mapping: wrap it in a list)")
        col = self._sparse_queries(list(queries), "search_sparse: query")
        program = self._program(namespace, where)
        nq = col.present.size
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, top_k, nq):
            return BatchHits.empty(nq)
        search = self._engine_entry(ns, "search_batch_sparse", "sparse attributes need")
        k = min(int(top_k), ns.total - ns.deleted, self._MAX_TOP_K_SPARSE)
        labels, _, counts, s64 = search(self._column(by), col, k, where=program)
        return BatchHits(labels, s64, counts, ns.ids)

    _BITS_METRICS = ("hamming", "jaccard")  # MLVDB_BITS_*

    @staticmethod
    def _bits_queries(queries, nbits: int, entry: str) -> np.ndarray:
        """Bit-code queries as uint64 [nq, nbits / 64]; query ``i`` is refused as ``{entry}: query i``."""
        if isinstance(queries, (str, bytes, bytearray, memoryview, Mapping)) or \
                (isinstance(queries, np.ndarray) and queries.ndim != 2):
            raise ValueError(f"{entry}: queries is a sequence of bit codes or a 2-d array with one code per row "
                             f"(got one code: wrap it in a list)")
        rows = list(queries)
        out = np.zeros((len(rows), nbits // 64), dtype=np.uint64)
        for i, q in enumerate(rows):
            out[i] = _where.encode_bits_code(q, nbits, f"{entry}: query {i}")
        return out

    def search_bits(self, queries, top_k: int, namespace: str, by: str, *, metric: str = "hamming",
                    where: Optional[Mapping] = None) -> BatchHits:
        """Additive: exact kNN over the declared ``bits<N>`` attribute ``by`` on the device (include/mlvdb_bits.h).
        ``queries`` is a sequence of ``N``-bit codes -- each ``bytes`` of ``N / 8`` bytes, a ``uint8`` array of ``N / 8``
        entries or a bool / 0-1 array of ``N`` entries, typed as at ingest -- or a ``uint8`` array ``[nq, N / 8]``; every live
        row that holds a code is a candidate, and ``where`` (one dict filter) restricts the rows first.  ``metric`` is
        ``"hamming"`` (the number of differing bits) or ``"jaccard"`` (``1 - |q & x| / |q | x|``, 0 for two all-zero codes).
        Per query the ``top_k`` rows with the smallest distance come back, ties to the earlier row; ``scores`` is the fp64
        distance.  ``top_k`` is clamped to the live row count and to 64.  Every refusal happens before the engine is
        touched."""
        self._refuse_sharded("search_bits")
        if not _where.is_bits(self._declared(by, "search_bits: ")):
            raise ValueError(f"search_bits: attribute {by!r} is a {self._attributes[by]} column; it needs a bits attribute")
        if metric not in self._BITS_METRICS:
            raise ValueError(f"search_bits: metric must be one of {self._BITS_METRICS} (got {metric!r})")
        self._one_filter("search_bits", where)
        q = self._bits_queries(queries, _where.bits_width(self._attributes[by]), "search_bits")
        program = self._program(namespace, where)
        nq = q.shape[0]
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, top_k, nq):
            return BatchHits.empty(nq)
        search = self._engine_entry(ns, "search_bits", "bits attributes need")
        k = min(int(top_k), ns.total - ns.deleted, self._MAX_TOP_K_SPARSE)
        labels, _, counts, d64 = search(self._column(by), q, k, metric=metric, where=program)
        return BatchHits(labels, d64, counts, ns.ids)

    _FUSIONS = ("rrf", "linear", "relative")  # MLVDB_FUSE_*
    _MAX_FETCH_K_HYBRID = 1024                # MLVDB_HYBRID_MAX_FETCH_DENSE

    @classmethod
    def _default_fetch_k_sparse(cls, top_k: int) -> int:
        return min(cls._MAX_TOP_K_SPARSE, max(int(top_k), 20))

    def search_hybrid(self, queries, sparse_queries, top_k: int, namespace: str, metric: str, by: str, *,
                      fusion: str = "rrf", weights=(1.0, 1.0), rrf_k: float = 60.0, fetch_k: Optional[int] = None,
                      fetch_k_sparse: Optional[int] = None, where: Optional[Mapping] = None,
                      components: bool = False) -> BatchHits:
        """Additive: hybrid retrieval in one device call (include/mlvdb_hybrid.h).  Query ``i`` is the dense vector
        ``queries[i]`` and the sparse vector ``sparse_queries[i]`` (typed as for ``search_sparse``) over the declared
        ``sparse`` attribute ``by``.  The ``fetch_k`` nearest rows (default ``min(1024, max(4 * top_k, 20))``, at most 1024)
        and the ``fetch_k_sparse`` best lexical matches (default ``min(64, max(top_k, 20))``, at most 64) are joined, every
        row of the union gets both its distance and its sparse score, and the ``top_k`` (<= 64) rows with the largest fused
        score come back, ties to the earlier row.  ``fusion``:

        ``"rrf"``       ``w_dense / (rrf_k + rank_dense + 1) + w_sparse / (rrf_k + rank_sparse + 1)``, a term being 0 for a
                        row its list does not hold (ranks are 0-based)
        ``"linear"``    ``w_sparse * sparse_score - w_dense * distance``
        ``"relative"``  ``w_dense * nd + w_sparse * ns``, the components min-max normalised over the union (the nearest row
                        has ``nd`` 1, the best match ``ns`` 1)

        with ``weights = (w_dense, w_sparse)``, finite and >= 0, and the distance the index's own (whatever ``metric``).
        ``where`` (one dict filter) is evaluated once and restricts both legs.  ``scores`` is the fused score;
        ``components=True`` returns a ``HybridBatchHits`` that adds ``dense`` (the distance), ``sparse`` (the score),
        ``rank_dense`` and ``rank_sparse`` (-1: the hit is not in that list).  An empty sparse query is no special case: its
        sparse list is the first ``fetch_k_sparse`` rows by label with score 0 -- a caller without a sparse query wants
        ``search_many``.  The fetch sizes are clamped to the live row count.  Every refusal happens before the engine is
        touched."""
        self._refuse_sharded("search_hybrid")
        if not _where.is_sparse(self._declared(by, "search_hybrid: ")):
            raise ValueError(f"search_hybrid: attribute {by!r} is a {self._attributes[by]} column; it needs a sparse attribute")
        if fusion not in self._FUSIONS:
            raise ValueError(f"search_hybrid: fusion must be one of {self._FUSIONS} (got {fusion!r})")
        try:
            w_dense, w_sparse = (float(w) for w in weights)
            c = float(rrf_k)
        except (TypeError, ValueError):
            raise ValueError(f"search_hybrid: weights is a pair of numbers and rrf_k a number (got {weights!r}, {rrf_k!r})") from None
        if not (np.isfinite(w_dense) and w_dense >= 0 and np.isfinite(w_sparse) and w_sparse >= 0):
            raise ValueError(f"search_hybrid: weights must be finite and >= 0 (got {weights!r})")
        if not (np.isfinite(c) and c >= 0):
            raise ValueError(f"search_hybrid: rrf_k must be finite and >= 0 (got {rrf_k!r})")
        self._one_filter("search_hybrid", where)
        if top_k > self._MAX_TOP_K_SPARSE:
            raise ValueError(f"search_hybrid: top_k must be <= {self._MAX_TOP_K_SPARSE} (got {top_k})")
        fetch_k = self._default_fetch_k(max(int(top_k), 0)) if fetch_k is None else int(fetch_k)
        fetch_k_sparse = self._default_fetch_k_sparse(max(int(top_k), 0)) if fetch_k_sparse is None else int(fetch_k_sparse)
        if not 1 <= fetch_k <= self._MAX_FETCH_K_HYBRID:
            raise ValueError(f"search_hybrid: fetch_k must lie in [1, {self._MAX_FETCH_K_HYBRID}] (got {fetch_k})")
        if not 1 <= fetch_k_sparse <= self._MAX_TOP_K_SPARSE:
            raise ValueError(f"search_hybrid: fetch_k_sparse must lie in [1, {self._MAX_TOP_K_SPARSE}] (got {fetch_k_sparse})")
        if top_k > fetch_k + fetch_k_sparse:
            raise ValueError(f"search_hybrid: top_k must be <= fetch_k + fetch_k_sparse (got {top_k} > {fetch_k} + {fetch_k_sparse})")
        if isinstance(sparse_queries, Mapping) or isinstance(sparse_queries, (str, bytes)):
            raise ValueError("search_hybrid: sparse_queries is a sequence of sparse vectors (got one mapping: wrap it in a list)")
        sparse_queries = list(sparse_queries)
        q = self._coerce_queries(queries)
        nq = q.shape[0]
        if len(sparse_queries) != nq:
            raise ValueError(f"search_hybrid: {nq} dense queries but {len(sparse_queries)} sparse queries")
        if not np.isfinite(q).all():
            raise ValueError("search_hybrid: a dense query holds a non-finite value (NaN / inf)")
        col = self._sparse_queries(sparse_queries, "search_hybrid: sparse query")
        program = self._program(namespace, where)
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, top_k, nq, q.shape[1]):
            return HybridBatchHits.empty(nq) if components else BatchHits.empty(nq)
        search = self._engine_entry(ns, "search_hybrid", "search_hybrid needs")
        active = ns.total - ns.deleted
        k = min(int(top_k), active)
        out = search(q, self._column(by), col, k, min(fetch_k, active), min(fetch_k_sparse, active),
                     method=fusion, weights=(w_dense, w_sparse), rrf_k=c, where=program, components=components)
        if not components:
            return BatchHits(out[0], out[1], out[2], ns.ids)
        return HybridBatchHits(out[0], out[1], out[2], ns.ids, *out[3:7])

    _MAX_TOP_K_MMR = 64      # MLVDB_MAX_TOPK
    _MAX_FETCH_K_MMR = 1024  # MLVDB_MMR_MAX_FETCH: the longest candidate list the selection walks

    @classmethod
    def _default_fetch_k(cls, top_k: int) -> int:
        return min(cls._MAX_FETCH_K_MMR, max(4 * int(top_k), 20))

    def _search_many_mmr(self, queries, top_k: int, namespace: str, metric: str, allowed_ids, where, distinct,
                         mmr_lambda, fetch_k) -> BatchHits:
        """``search_many`` with ``mmr_lambda=``: every refusal happens before the engine is touched."""
        self._refuse_sharded("mmr_lambda=")
        if distinct is not None:
            raise ValueError("mmr_lambda: distinct= cannot be combined with it, give one of the two")
        lam = float(mmr_lambda)
        if not 0.0 <= lam <= 1.0:  # (NaN fails both comparisons)
            raise ValueError(f"mmr_lambda must lie in [0, 1] (got {mmr_lambda})")
        if top_k > self._MAX_TOP_K_MMR:
            raise ValueError(f"mmr_lambda: top_k must be <= {self._MAX_TOP_K_MMR} (got {top_k})")
        if fetch_k is None:
            fetch_k = self._default_fetch_k(max(int(top_k), 0))
        fetch_k = int(fetch_k)
        if fetch_k > self._MAX_FETCH_K_MMR:
            raise ValueError(f"mmr_lambda: fetch_k must be <= {self._MAX_FETCH_K_MMR} (got {fetch_k})")
        if fetch_k < top_k:
            raise ValueError(f"mmr_lambda: fetch_k must be >= top_k (got fetch_k={fetch_k}, top_k={top_k})")
        self._no_where_list("mmr_lambda", where, allowed_ids)
        program = self._program(namespace, where)
        q = self._coerce_queries(queries)
        nq = q.shape[0]
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, top_k, nq, q.shape[1]):
            return BatchHits.empty(nq)
        search_mmr = self._engine_entry(ns, "search_mmr", "mmr_lambda= needs")
        active = ns.total - ns.deleted
        k = min(int(top_k), active)  # as search_many clamps top_k (the reference clamps to the live count)
        fetch = min(fetch_k, active)  # (>= k: fetch_k >= top_k)
        labels, dist, counts = search_mmr(q, k, fetch, lam, where=program)[:3]
        return BatchHits(labels, self._scores(dist, metric), counts, ns.ids)

    _MAX_LIKE_EXAMPLES = 64  # MLVDB_LIKE_MAX_EXAMPLES: one example per lane of the strip's wavefront
    _MAX_LIKE_FETCH = 1024   # MLVDB_LIKE_MAX_FETCH: top_k + the most examples of one query

    @staticmethod
    def _like_groups(groups, what: str) -> List[list]:
        """``positive`` / ``negative`` / ``weights`` as one list per query; a flat sequence (of UUIDs, of numbers) is one query."""
        if isinstance(groups, (UUID, str, bytes)) or not isinstance(groups, (SequenceABC, np.ndarray)):
            raise ValueError(f"search_like: {what} must be a sequence with one sequence per query (or one flat sequence)")
        rows = list(groups)
        if rows and not any(isinstance(r, (SequenceABC, np.ndarray)) and not isinstance(r, (str, bytes)) for r in rows):
            return [rows]
        for r in rows:
            if isinstance(r, (UUID, str, bytes)) or not isinstance(r, (SequenceABC, np.ndarray)):
                raise ValueError(f"search_like: {what} mixes per-query sequences with single entries")
        return [list(r) for r in rows]

    @staticmethod
    def like_weights(n_positive: int, n_negative: int) -> Tuple[float, float]:
        """The default "average vector" rule, in Python floats: (weight of each positive, weight of each negative) --
        ``1/|P|`` without negatives, else ``2/|P|`` and ``-1/|N|``: ``mean(P) + (mean(P) - mean(N))``."""
        if n_negative == 0:
            return (1.0 / n_positive if n_positive else 0.0), 0.0
        return (2.0 / n_positive if n_positive else 0.0), -1.0 / n_negative

    def search_like(self, positive, top_k: int, namespace: str, metric: str, *, negative=None, queries=None, weights=None,
                    exclude_examples: bool = True, where: Optional[Mapping] = None) -> BatchHits:
        """Additive: "more like this" -- kNN around stored vectors named by id, built and searched on the device
        (include/mlvdb_like.h): the rows never leave HBM.

        ``positive`` (and the optional ``negative``) hold ``nq`` entries, each a sequence of UUIDs of stored vectors; a
        flat sequence of UUIDs means one query.  Query ``i`` is the weighted sum of its examples -- of their unit vectors
        in a cosine namespace -- positives first, then negatives, each summed as often as it is named: every positive
        weighs ``1/|P|`` without negatives, ``2/|P|`` with them and every negative ``-1/|N|`` (``mean(P) + (mean(P) -
        mean(N))``).  ``weights=`` (the shape of ``positive``) gives explicit per-example numbers instead and cannot be
        combined with ``negative``.  ``queries=`` (``[nq, dim]`` or a sequence of ``VectorDTO``) is an optional base batch
        the examples are added to, e.g. the embedding of a text query.  With ``exclude_examples`` (the default) a query's
        examples never come back among its hits; at most 64 examples per query and ``top_k`` + examples <= 1024.  ``where``
        (one dict filter) restricts the rows searched, not the examples.  Every refusal happens before the engine is
        touched; hits and scores are otherwise those of ``search_many`` for the same query vectors."""
        self._refuse_sharded("search_like")
        self._no_where_list("search_like", where)
        if weights is not None and negative is not None:
            raise ValueError("search_like: weights= gives every example its own number and cannot be combined with negative=")
        pos = self._like_groups(positive, "positive")
        nq = len(pos)
        neg = [[] for _ in range(nq)] if negative is None else self._like_groups(negative, "negative")
        if len(neg) != nq:
            raise ValueError(f"search_like: {nq} positive entries, {len(neg)} negative entries")
        if weights is not None:
            given = self._like_groups(weights, "weights")
            if [len(g) for g in given] != [len(p) for p in pos]:
                raise ValueError("search_like: weights must hold one number per positive id")
            per_example = [float(x) for g in given for x in g]
            if not all(math.isfinite(x) for x in per_example):
                raise ValueError("search_like: weights must be finite")
        else:
            per_example = []
            for p, n in zip(pos, neg):
                wp, wn = self.like_weights(len(p), len(n))
                per_example += [wp] * len(p) + [wn] * len(n)
        examples = [p + n for p, n in zip(pos, neg)]
        for i, e in enumerate(examples):
            if len(e) > self._MAX_LIKE_EXAMPLES:
                raise ValueError(f"search_like: query {i} names {len(e)} examples, at most {self._MAX_LIKE_EXAMPLES} are supported")
            if not e and queries is None:
                raise ValueError(f"search_like: query {i} has no example and there is no queries= batch to start from")
        most = max((len(set(e)) for e in examples), default=0)
        if top_k + most > self._MAX_LIKE_FETCH:
            raise ValueError(f"search_like: top_k + examples must be <= {self._MAX_LIKE_FETCH} (got {top_k} + {most})")
        program = self._program(namespace, where)
        base = None if queries is None else self._coerce_queries(queries)
        if base is not None and base.shape[0] != nq:
            raise ValueError(f"search_like: {nq} positive entries, {base.shape[0]} queries")
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, top_k, nq, None if base is None else base.shape[1]):
            return BatchHits.empty(nq)
        flat = [u for e in examples for u in e]
        labels = ns.ids.lookup(flat) if flat else np.zeros(0, np.int64)
        if (labels < 0).any():
            raise ValueError(f"search_like: id {flat[int(np.argmax(labels < 0))]} is unknown or removed in namespace {namespace!r}")
        search_like = self._engine_entry(ns, "search_like", "search_like needs")
        offsets = np.concatenate([[0], np.cumsum([len(e) for e in examples])]).astype(np.int64)
        k = min(int(top_k), ns.total - ns.deleted)  # as search_many clamps top_k (the reference clamps to the live count)
        out_labels, dist, counts = search_like(labels, np.asarray(per_example, np.float64), offsets, k, base=base,
                                               exclude=bool(exclude_examples), where=program)[:3]
        return BatchHits(out_labels, self._scores(dist, metric), counts, ns.ids)

    _MAX_EXAMPLES = 64        # MLVDB_EXAMPLES_MAX
    _MAX_TOP_K_EXAMPLES = 64  # MLVDB_MAX_TOPK: one selection list of a wavefront

    @staticmethod
    def _is_example_vector(e) -> bool:
        """``e`` is one vector: a ``VectorDTO``-like object, a 1-D array, or a sequence of plain numbers."""
        if hasattr(e, "values") and not isinstance(e, (dict, np.ndarray)):
            return True
        if isinstance(e, np.ndarray):
            return e.ndim == 1
        return (isinstance(e, SequenceABC) and not isinstance(e, (str, bytes)) and len(e) > 0
                and all(isinstance(x, (int, float, np.number)) and not isinstance(x, bool) for x in e))

    def _example_bags(self, what: str, bags, name: str) -> List[list]:
        """``positive`` / ``negative`` / ``context`` as one list per query; a flat sequence of ids is one query."""
        if isinstance(bags, (UUID, str, bytes)) or not isinstance(bags, (SequenceABC, np.ndarray)):
            raise ValueError(f"{what}: {name} must hold one sequence of examples per query")
        rows = list(bags)
        if rows and all(isinstance(r, UUID) for r in rows):
            return [rows]
        for i, r in enumerate(rows):
            if isinstance(r, (UUID, str, bytes)) or not isinstance(r, (SequenceABC, np.ndarray)):
                raise ValueError(f"{what}: {name} mixes per-query sequences with single entries")
            if self._is_example_vector(r):
                raise ValueError(f"{what}: {name}[{i}] is one vector where the examples of query {i} are expected; "
                                 "wrap it in a list")
        return [list(r) for r in rows]

    def _search_bags(self, what: str, mode: int, bags, top_k: int, namespace: str, metric: str, where, allowed_ids,
                     exclude_examples: bool) -> "TieredBatchHits":
        """The tail the two entries share.  ``bags``: per query a list of (example, role); every refusal before the engine."""
        if metric == "euclidean":
            raise ValueError(f'{what}: metric "euclidean" is not supported (tiers and sums are defined on the squared '
                             'distance), use "l2"')
        self._no_where_list(what, where, allowed_ids)
        if callable(where):
            raise ValueError(f"{what}: where must be one dict filter (a predicate has no device form)")
        for i, bag in enumerate(bags):
            if len(bag) > self._MAX_EXAMPLES:
                raise ValueError(f"{what}: query {i} holds {len(bag)} examples, at most {self._MAX_EXAMPLES} are supported")
        program = self._program(namespace, where)
        ns = self._ns.get(namespace)
        nq = len(bags)
        flat = [e for bag in bags for e, _ in bag]
        stored = [i for i, e in enumerate(flat) if not self._is_example_vector(e)]
        for i in stored:
            if not isinstance(flat[i], UUID):
                raise ValueError(f"{what}: example {i} is neither the UUID of a stored vector nor a vector (a 1-D array, a "
                                 f"sequence of numbers or a VectorDTO): {flat[i]!r}")
        labels = np.full(len(flat), -1, np.int64)
        if stored:
            ids = [flat[i] for i in stored]
            found = ns.ids.lookup(ids) if ns is not None else np.full(len(ids), -1, np.int64)
            if (found < 0).any():
                raise ValueError(f"{what}: id {ids[int(np.argmax(found < 0))]} is unknown or removed in namespace {namespace!r}")
            labels[stored] = found
        vectors = None
        if len(stored) < len(flat):
            dim = ns.dim if ns is not None else None
            for i, e in enumerate(flat):
                if labels[i] >= 0:
                    continue
                v = np.asarray(getattr(e, "values", e), dtype=np.float32)
                if v.ndim != 1 or (dim is not None and v.size != dim) or not np.isfinite(v).all():
                    raise ValueError(f"{what}: example {i} is no finite vector of the namespace's dimensionality")
                if vectors is None:
                    dim = v.size
                    vectors = np.zeros((len(flat), dim), np.float32)
                vectors[i] = v
        if self._nothing_to_search(ns, top_k, nq):
            return TieredBatchHits.empty(nq)
        search = self._engine_entry(ns, "search_examples", f"{what} needs")
        roles = np.asarray([r for bag in bags for _, r in bag], np.int32)
        offsets = np.concatenate([[0], np.cumsum([len(bag) for bag in bags])]).astype(np.int64)
        k = min(int(top_k), ns.total - ns.deleted, self._MAX_TOP_K_EXAMPLES)
        out_labels, tiers, values, counts = search(mode, labels, vectors, roles, offsets, k, exclude=bool(exclude_examples),
                                                   where=program)
        return TieredBatchHits(out_labels, tiers, values, counts, ns.ids)

    def search_examples(self, positive, top_k: int, namespace: str, metric: str, *, negative=None,
                        where: Optional[Mapping] = None, exclude_examples: bool = True,
                        allowed_ids: Optional[Iterable[UUID]] = None) -> "TieredBatchHits":
        """Additive: "recommend", best score (include/mlvdb_examples.h) -- every row judged against each example on its own
        instead of against their average (``search_like``).  ``positive`` (and the optional ``negative``) hold one sequence
        per query; an example is the UUID of a stored vector (read on the device, never sent) or a vector (an array, a
        sequence of numbers, a ``VectorDTO``); a flat sequence of UUIDs means one query.  Rows nearer to some liked example
        than to any disliked one come first (tier 0), ranked by the distance to their nearest liked example; the others
        follow (tier 1), the farthest from its nearest disliked example first (value: minus that distance).  The answer is
        the exact top ``top_k`` (clamped to the live count and to 64) over all live rows -- of those ``where`` (one dict
        filter) matches; with ``exclude_examples`` a query's stored examples never come back.  Values are distances of the
        index's space -- the squared distance for "l2", ``1 - cosine`` for "cosine" -- so metric "euclidean" is refused.
        At most 64 examples per query, at least one.  Every refusal happens before the engine is touched."""
        what = "search_examples"
        self._refuse_sharded(what)
        pos = self._example_bags(what, positive, "positive")
        neg = [[] for _ in pos] if negative is None else self._example_bags(what, negative, "negative")
        if len(neg) != len(pos):
            raise ValueError(f"{what}: {len(pos)} positive entries, {len(neg)} negative entries")
        bags = [[(e, _native.EXAMPLE_POS) for e in p] + [(e, _native.EXAMPLE_NEG) for e in n] for p, n in zip(pos, neg)]
        for i, bag in enumerate(bags):
            if not bag:
                raise ValueError(f"{what}: query {i} has no example")
        return self._search_bags(what, _native.EXAMPLES_BEST, bags, top_k, namespace, metric, where, allowed_ids,
                                 exclude_examples)

    def search_discover(self, top_k: int, namespace: str, metric: str, *, target=None, context,
                        where: Optional[Mapping] = None, exclude_examples: bool = True,
                        allowed_ids: Optional[Iterable[UUID]] = None) -> "TieredBatchHits":
        """Additive: "discover" / "context" search (include/mlvdb_examples.h).  ``context`` holds per query a sequence of
        (positive, negative) pairs of examples (ids or vectors, as in ``search_examples``); each pair cuts the space into
        the half nearer to its positive.  With ``target`` (one example per query) the rows are ranked by the number of
        pairs they miss (tier), then by their distance to the target (value): the target is searched inside as many of
        the half-spaces as possible, and without pairs this is the plain exact search.  ``target=None`` selects context
        mode (at least one pair per query): tier 0 for every row, value the sum over the pairs of how much nearer the row
        is to the negative than to the positive, 0.0 inside every half-space.  Limits and refusals as ``search_examples``:
        at most 64 examples per query, the target included."""
        what = "search_discover"
        self._refuse_sharded(what)
        if isinstance(context, (UUID, str, bytes)) or not isinstance(context, (SequenceABC, np.ndarray)):
            raise ValueError(f"{what}: context must hold one sequence of (positive, negative) pairs per query")
        per_query = [list(c) for c in context]
        if target is None:
            targets = [None] * len(per_query)
        else:
            # one example (an id, or one vector in any of its forms) is the target of one query; else one per query
            targets = [target] if isinstance(target, UUID) or self._is_example_vector(target) else list(target)
            if len(targets) != len(per_query):
                raise ValueError(f"{what}: {len(targets)} targets, {len(per_query)} context entries")
        bags = []
        for i, (t, pairs) in enumerate(zip(targets, per_query)):
            bag = [] if target is None else [(t, _native.EXAMPLE_TARGET)]
            for pair in pairs:
                if isinstance(pair, (UUID, str, bytes)) or not isinstance(pair, (SequenceABC, np.ndarray)) or len(pair) != 2:
                    raise ValueError(f"{what}: query {i}: every context entry must be a (positive, negative) pair")
                bag += [(pair[0], _native.EXAMPLE_POS), (pair[1], _native.EXAMPLE_NEG)]
            if target is None and not pairs:
                raise ValueError(f"{what}: query {i} has neither a target nor a context pair")
            bags.append(bag)
        mode = _native.EXAMPLES_CONTEXT if target is None else _native.EXAMPLES_DISCOVER
        return self._search_bags(what, mode, bags, top_k, namespace, metric, where, allowed_ids, exclude_examples)

    def _compile_each(self, namespace: str, wheres) -> Tuple[list, np.ndarray]:
        for w in wheres:
            if w is not None and not isinstance(w, Mapping):
                raise ValueError(f"per-query where entries must be dict filters or None (where.py), got {type(w).__name__}")
        ns = self._ns.get(namespace)
        return _where.compile_each(list(wheres), self._attributes, ns.strings if ns is not None else {})

    def _search_many_each(self, queries, top_k: int, namespace: str, metric: str, wheres) -> BatchHits:
        """``search_many`` with ``where`` = one dict filter (or ``None``) per query."""
        q = self._coerce_queries(queries)
        nq = q.shape[0]
        if len(wheres) != nq:
            raise ValueError(f"search_many: {len(wheres)} per-query filters for {nq} queries")
        programs, of = self._compile_each(namespace, wheres)
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, top_k, nq, q.shape[1]):
            return BatchHits.empty(nq)
        k = min(int(top_k), ns.total - ns.deleted, self._MAX_TOP_K)  # as a single-dict call clamps it
        if not programs:
            labels, dist, counts = self._search_engine(ns, q, k)
        else:
            labels, dist, counts = self._engine_entry(ns, "search_each", "per-query filters need")(q, k, programs, of)
        return BatchHits(labels, self._scores(dist, metric), counts, ns.ids)

    def search_stream(self, batches, top_k: int, namespace: str, metric: str):
        """Additive: ``search_many`` over an iterable of query batches, pipelined -- yields one ``BatchHits`` per batch, in
        order, while the next batch is already being scanned.  On a row-sharded namespace (``Index(devices=[...])``) the
        shard scans of wave i+1 are queued before wave i's per-shard candidates are merged
        (``MultiDeviceEngine.search_stream``); on a single engine a worker thread runs the next ``search_many`` (the ctypes
        call holds no GIL) while the caller consumes the current one.  The namespace must not be mutated meanwhile."""
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, top_k):
            for q in batches:
                yield BatchHits.empty(self._coerce_queries(q).shape[0])
            return
        k = min(int(top_k), ns.total - ns.deleted, self._MAX_TOP_K)
        stream = getattr(ns.engine, "search_stream", None)
        if stream is not None:
            ok = []  # per batch: the query count if it could not be scanned (wrong dimensionality), else None

            def feed():
                for q in batches:
                    q = self._coerce_queries(q)
                    if q.shape[1] != ns.dim or q.shape[0] == 0:
                        ok.append(q.shape[0])
                        continue
                    ok.append(None)
                    yield q

            results = stream(feed(), k)
            done = 0
            for labels, dist, counts, _ in results:
                while done < len(ok) and ok[done] is not None:  # batches skipped before this one
                    yield BatchHits.empty(ok[done])
                    done += 1
                done += 1
                yield BatchHits(labels, self._scores(dist, metric), counts, ns.ids)
            while done < len(ok):
                if ok[done] is not None:
                    yield BatchHits.empty(ok[done])
                done += 1
            return
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=1) as pool:
            pending = None
            for q in batches:
                nxt = pool.submit(self.search_many, q, top_k, namespace, metric)
                if pending is not None:
                    yield pending.result()
                pending = nxt
            if pending is not None:
                yield pending.result()

    def range_search(self, query: VectorDTO, radius: float, namespace: str, metric: str,
                     max_results: int = 1024, where: Optional[Mapping] = None) -> List[SearchResult]:
        values = np.asarray(query.values, dtype=np.float32)
        if values.ndim != 1:
            return []
        return self.range_search_many(values[None, :], radius, namespace, metric, max_results, where=where)[0]

    # ------------------------------------------------------------------ additive: metadata queries on the device
    def count(self, namespace: str, where: Mapping) -> int:
        """Live rows of ``namespace`` whose attributes satisfy the dict filter ``where`` (where.py); 0 for an unknown
        namespace."""
        program = self._compile(namespace, where)
        ns = self._ns.get(namespace)
        return 0 if self._no_rows(ns) else ns.engine.where_count(program)

    def count_many(self, namespace: str, wheres: Sequence[Mapping]) -> List[int]:
        """``count`` of each dict filter of ``wheres``, all evaluated in one pass over the columns per native call."""
        wheres = list(wheres)
        if any(w is None for w in wheres):
            raise ValueError("count_many: every entry must be a dict filter")
        programs, of = self._compile_each(namespace, wheres)
        ns = self._ns.get(namespace)
        if self._no_rows(ns) or not programs:
            return [0] * len(wheres)
        counts = np.asarray(ns.engine.count_each(programs), dtype=np.int64)
        return [int(counts[j]) for j in of]

    def query_by_metadata(self, namespace: str, where: Mapping, *, order_by: Optional[str] = None, descending: bool = False,
                          limit: Optional[int] = None, offset: int = 0) -> List[UUID]:
        """UUIDs of the live rows satisfying ``where``, in insertion order (README.md:252,274: ``query_by_metadata``).  With
        ``order_by`` (and a ``limit``): ``top_by(namespace, order_by, limit, where, ...)["ids"]`` -- the rows that hold a value
        of that attribute, ranked on the device."""
        self.check_order_keywords(order_by, descending, limit, offset)
        if order_by is not None:
            return self.top_by(namespace, order_by, limit, where, descending=descending, offset=offset)["ids"]
        program = self._compile(namespace, where)
        ns = self._ns.get(namespace)
        if self._no_rows(ns):
            return []
        return ns.ids.uuids_at(ns.engine.where_labels(program)).tolist()

    # ------------------------------------------------------------------ additive: updates and deletes on the device
    def check_attribute_patches(self, n_ids: int, values) -> List[Mapping]:
        """The refusals of ``update_attributes`` that need no namespace -> one patch per id (``values`` is one mapping for
        every id, or a sequence with one mapping per id; the keys are declared attributes)."""
        if isinstance(values, Mapping):
            patches = [values] * n_ids
            distinct = [values]
        else:
            patches = distinct = list(values)
            if len(patches) != n_ids:
                raise ValueError(f"update_attributes: {n_ids} ids but {len(patches)} value mappings")
        for p in distinct:
            if not isinstance(p, Mapping):
                raise ValueError(f"update_attributes: values must be mappings, got {type(p).__name__}")
            for name in p:
                self._declared(name)
        return patches

    def _stage_patches(self, namespace: str, patches: Sequence[Mapping]):
        """Encode per-id patches -> ({column index: (positions in the id list, encoded values)}, the namespace's string
        dictionaries with the new strings).  Raises ``ValueError`` before anything is mutated."""
        ns = self._ns.get(namespace)
        strings = {name: dict(codes) for name, codes in (ns.strings if ns is not None else {}).items()}
        out = {}
        for i, (name, kind) in enumerate(self._attributes.items()):
            pos = [j for j, p in enumerate(patches) if name in p]
            if not pos:
                continue
            if _where.is_list(kind):
                col = _where.encode_list_column(name, kind, [patches[j][name] for j in pos],
                                                strings.setdefault(name, {}) if kind == "str[]" else {})
            elif _where.is_sparse(kind):
                col = _where.encode_sparse_column(name, [patches[j][name] for j in pos])
            elif _where.is_bits(kind):
                col = _where.encode_bits_column(name, kind, [patches[j][name] for j in pos])
            else:
                col = _where.encode_column(name, kind, [patches[j][name] for j in pos],
                                           strings.setdefault(name, {}) if kind == "str" else {})
            out[i] = (np.asarray(pos, dtype=np.int64), col)
        return out, strings

    def validate_attribute_update(self, n_ids: int, values, namespace: str) -> None:
        """Raises what ``update_attributes`` would raise for these values, without touching the index."""
        self._stage_patches(namespace, self.check_attribute_patches(n_ids, values))

    def update_attributes(self, ids: Sequence[UUID], values, namespace: str) -> int:
        """Set attribute values of the rows ``ids`` in place (no new label, no tombstone): ``values`` is one mapping applied to
        every id, or a sequence with one mapping per id.  Keys are declared attributes, values are typed as at ingest, ``None``
        clears a value, a key that is missing leaves that attribute alone.  Unknown or removed ids are skipped, as ``remove``
        skips them; for an id listed twice the entries apply in order, so the last one that names a key wins.  Returns the
        number of rows that were given a value.  New strings reach the namespace's dictionary only when every engine call
        succeeded."""
        ids = list(ids)
        staged, strings = self._stage_patches(namespace, self.check_attribute_patches(len(ids), values))
        ns = self._ns.get(namespace)
        if self._no_rows(ns) or not ids or not staged:
            return 0
        set_at = self._engine_entry(ns, "set_attr_at", "update_attributes needs")
        labels = ns.ids.lookup(ids)
        touched = []
        for i, (pos, col) in staged.items():
            lab = labels[pos]
            keep = lab >= 0
            lab = lab[keep]
            rows, last = np.unique(lab[::-1], return_index=True)  # the last entry of each row
            if not rows.size:
                continue
            if isinstance(col, _where.ListColumn):
                set_list_at = self._engine_entry(ns, "set_attr_list_at", "list attributes need")
                set_list_at(i, rows, col.take(np.flatnonzero(keep)[lab.size - 1 - last]))
            elif isinstance(col, _where.SparseColumn):
                set_sparse_at = self._engine_entry(ns, "set_attr_sparse_at", "sparse attributes need")
                set_sparse_at(i, rows, col.take(np.flatnonzero(keep)[lab.size - 1 - last]))
            elif isinstance(col, _where.BitsColumn):
                set_bits_at = self._engine_entry(ns, "bits_set_at", "bits attributes need")
                set_bits_at(i, rows, col.take(np.flatnonzero(keep)[lab.size - 1 - last]))
            else:
                set_at(i, rows, col[keep][lab.size - 1 - last])
            touched.append(rows)
        ns.strings = strings
        return int(np.unique(np.concatenate(touched)).size) if touched else 0

    def stage_assignments(self, namespace: str, values: Mapping):
        """The refusals of ``update_where``'s ``values`` -> ([(column, op, a), ...] as the engine takes them, the namespace's
        string dictionaries with the new strings).  A value is a literal (typed as at ingest), ``None`` (clear) or
        ``{"$inc": x}`` on an ``int`` (``x`` an int) or ``float`` (``x`` an int or float, not NaN) attribute."""
        if not isinstance(values, Mapping) or not values:
            raise ValueError("update_where: values must be a non-empty mapping of declared attributes")
        for name in values:
            self._declared(name)
        ns = self._ns.get(namespace)
        strings = {name: dict(codes) for name, codes in (ns.strings if ns is not None else {}).items()}
        out = []
        for i, (name, kind) in enumerate(self._attributes.items()):
            if name not in values:
                continue
            v = values[name]
            if _where.is_sparse(kind):
                raise ValueError(f"update_where: {name!r} is a sparse attribute: one vector for every matching row is not "
                                 f"supported, use update_attributes with ids")
            if _where.is_bits(kind):
                raise ValueError(f"update_where: {name!r} is a {kind} attribute: one code for every matching row is not "
                                 f"supported, use update_attributes with ids")
            if _where.is_geo(kind) and isinstance(v, Mapping) and "$inc" in v:
                raise ValueError(f"update_where: {name!r} is a geo attribute: it takes a point or None, $inc adds to numbers")
            if _where.is_list(kind):  # one list for every matching row, or None: (column, "list", sorted codes or None)
                if isinstance(v, Mapping):
                    raise ValueError(f"update_where: {name!r} is a {kind} attribute: it takes a list or None, no operator "
                                     f"($inc adds to numbers; per-row $push / $pull are not supported)")
                col = _where.encode_list_column(name, kind, [v], strings.setdefault(name, {}) if kind == "str[]" else {})
                out.append((i, "list", col.row(0)))
                continue
            if isinstance(v, Mapping) and not _where.is_geo(kind):  # (a geo literal may be {"lat": .., "lon": ..})
                if list(v) != ["$inc"]:
                    raise ValueError(f"update_where: {name!r}: the only operator is $inc (got {sorted(map(str, v))})")
                x = v["$inc"]
                if kind == "int" and isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)):
                    if not -(2 ** 63) < int(x) < 2 ** 63:
                        raise ValueError(f"update_where: {name!r}: $inc {x!r} is outside int64")
                    out.append((i, _native.SET_ADD, int(x)))
                elif kind == "float" and isinstance(x, (int, float, np.integer, np.floating)) and \
                        not isinstance(x, (bool, np.bool_)) and not np.isnan(float(x)):
                    out.append((i, _native.SET_ADD, _where.float_bits(float(x))))
                else:
                    raise ValueError(f"update_where: {name!r} ({kind}): $inc takes an int on an int attribute, an int or a "
                                     f"float that is not NaN on a float attribute (got {x!r})")
                continue
            col = _where.encode_column(name, kind, [v], strings.setdefault(name, {}) if kind == "str" else {})
            out.append((i, _native.SET_ASSIGN, int(col.view(np.int64)[0])))
        return out, strings

    def update_where(self, namespace: str, where: Mapping, values: Mapping) -> int:
        """Set attribute values of every live row the dict filter ``where`` matches, in one pass on the device
        (include/mlvdb_mutate.h): ``values`` maps a declared attribute to a literal, to ``None`` (clear) or to ``{"$inc": x}``
        (rows without a value keep none).  The filter sees the values from before the call.  Returns the matched count.  All
        or nothing: when an increment would overflow on some row, ``ValueError`` says on how many and nothing has changed.
        A list attribute takes a list (every matching row shares it) or ``None``.  The scalar assignments are one device pass
        and each list attribute is one more; a call that needs several passes must not assign an attribute its own filter
        reads (``ValueError``: split it), since a later pass would see the earlier one's values."""
        program = self._compile(namespace, where)
        assigns, strings = self.stage_assignments(namespace, values)
        scalars = [a for a in assigns if a[1] != "list"]
        lists = [a for a in assigns if a[1] == "list"]
        if len(lists) + bool(scalars) > 1:
            ops = program.ops
            read = set(ops["attr"][~np.isin(ops["op"], (_where.TRUE, _where.AND, _where.OR, _where.NOT))].tolist())
            clash = sorted(name for i, name in enumerate(self._attributes) if i in read and any(a[0] == i for a in assigns))
            if clash:
                raise ValueError(f"update_where: the filter reads {clash}, which this call assigns together with other "
                                 f"attributes in several passes; assign them in a call of their own")
        ns = self._ns.get(namespace)
        if self._no_rows(ns):
            return 0
        matched = None
        if scalars:  # first: the only pass that can refuse
            matched, refused = self._engine_entry(ns, "update_where", "update_where needs")(program, scalars)
            if refused:
                raise ValueError(f"update_where: $inc would overflow on {refused} of the {matched} matching rows; nothing was changed")
        for i, _, codes in lists:
            matched = self._engine_entry(ns, "update_where_list", "list attributes need")(program, i, codes)
        ns.strings = strings
        return matched

    def remove_where(self, namespace: str, where: Mapping, *, return_ids: bool = False):
        """``remove`` of every live row the dict filter ``where`` matches, tombstoned on the device without listing them on
        the host first.  Returns their count, or their UUIDs (insertion order) with ``return_ids=True``."""
        program = self._compile(namespace, where)
        ns = self._ns.get(namespace)
        if self._no_rows(ns):
            return [] if return_ids else 0
        labels = self._engine_entry(ns, "tombstone_where", "remove_where needs")(program)
        ids = ns.ids.uuids_at(labels).tolist() if return_ids else None
        if labels.size:
            ns.ids.kill(labels)
        ns.deleted += int(labels.size)
        if ns.deleted / max(1, ns.total) >= self._rebuild_threshold:
            ns.rebuild_required = True
        return ids if return_ids else int(labels.size)

    # ------------------------------------------------------------------ additive: ordered metadata queries on the device
    _MAX_ORDER_ROWS = 4096  # MLVDB_ORDER_MAX_ROWS

    @staticmethod
    def check_order_keywords(order_by, descending, limit, offset) -> None:
        """The refusals of ``query_by_metadata``'s ordering keywords: they come with ``order_by`` (and a ``limit``) or not at all."""
        if order_by is None:
            if descending is not False or limit is not None or not (offset == 0 and not isinstance(offset, bool)):
                raise ValueError("query_by_metadata: descending, limit and offset need order_by")
        elif limit is None:
            raise ValueError("query_by_metadata: order_by needs a limit (at most 4096 rows are ranked per call)")

    def check_top_by_args(self, by, limit, descending=False, offset=0) -> str:
        """The refusals of ``top_by`` that need no namespace -> the column kind of ``by`` ("int", "float" or "bool")."""
        kind = self._declared(by, "top_by: ")
        self._check_scalar("top_by", by)
        if kind == "str":
            raise ValueError(f"top_by: attribute {by!r} is a str column; its codes are in order of first use, not in lexical "
                             f"order, so ranking needs an int, float or bool attribute")
        self._check_window("top_by", limit, offset)
        if not isinstance(descending, (bool, np.bool_)):
            raise ValueError(f"top_by: descending must be a bool (got {descending!r})")
        return kind

    @staticmethod
    def decode_order_values(kind: str, values) -> list:
        """Column values as ``top_by`` returns them: ``True`` / ``False`` for a bool attribute, Python ints or floats."""
        values = values.tolist() if isinstance(values, np.ndarray) else list(values)
        return [bool(v) for v in values] if kind == "bool" else values

    def top_by(self, namespace: str, by: str, limit: int, where: Optional[Mapping] = None, *, descending: bool = False,
               offset: int = 0):
        """Ranks ``[offset, offset + limit)`` of the live rows of ``namespace`` (those the dict filter ``where`` matches,
        when one is given) that hold a value of the declared ``int`` / ``float`` / ``bool`` attribute ``by``, ranked on the
        device (include/mlvdb_order.h) by that value -- ascending, or ``descending`` -- and rows of equal value in insertion
        order: ``{"ids": [UUID, ...], "values": [...], "matched": live matching rows, "absent": those of them without a
        value}``, the values decoded (``True`` / ``False``, ints, floats; ``-0.0`` and ``0.0`` tie).  ``offset + limit`` is at
        most 4096.  An unknown or empty namespace gives no rows and zeros."""
        kind = self.check_top_by_args(by, limit, descending, offset)
        self._one_filter("top_by", where)
        program = self._program(namespace, where)
        ns = self._ns.get(namespace)
        if self._no_rows(ns):
            return {"ids": [], "values": [], "matched": 0, "absent": 0}
        where_ordered = self._engine_entry(ns, "where_ordered", "top_by needs")
        labels, values, matched, absent = where_ordered(self._column(by), int(limit), where=program,
                                                        descending=bool(descending), offset=int(offset))
        return {"ids": ns.ids.uuids_at(labels).tolist(), "values": self.decode_order_values(kind, values), "matched": matched,
                "absent": absent}

    # ------------------------------------------------------------------ additive: nearest by distance on a geo attribute
    def check_nearest_args(self, by, point, limit, offset=0) -> int:
        """The refusals of ``nearest`` that need no namespace -> the packed centre."""
        if not _where.is_geo(self._declared(by, "nearest: ")):
            raise ValueError(f"nearest: attribute {by!r} is a {self._attributes[by]} column; it needs a geo attribute")
        self._check_window("nearest", limit, offset)
        return _where.geo_pack(point, "nearest: point")

    def nearest(self, namespace: str, by: str, point, limit: int, where: Optional[Mapping] = None, *, offset: int = 0):
        """Ranks ``[offset, offset + limit)`` of the live rows of ``namespace`` (those the dict filter ``where`` matches,
        when one is given) that hold a location in the declared ``geo`` attribute ``by``, ranked on the device
        (include/mlvdb_geo.h) by great-circle distance from ``point`` and rows at equal distance in insertion order:
        ``{"ids": [UUID, ...], "points": [(lat, lon), ...], "distances": [metres, ...], "matched": live matching rows,
        "absent": those of them without a location}``.  ``point`` is quantised as stored points are; a maximum distance is a
        ``$geo_radius`` in ``where``.  ``offset + limit`` is at most 4096.  An unknown or empty namespace gives no rows."""
        center = self.check_nearest_args(by, point, limit, offset)
        self._one_filter("nearest", where)
        program = self._program(namespace, where)
        ns = self._ns.get(namespace)
        if self._no_rows(ns):
            return {"ids": [], "points": [], "distances": [], "matched": 0, "absent": 0}
        geo_nearest = self._engine_entry(ns, "geo_nearest", "nearest needs")
        labels, points, dist, matched, absent = geo_nearest(self._column(by), center, int(limit), where=program,
                                                            offset=int(offset))
        return {"ids": ns.ids.uuids_at(labels).tolist(), "points": [_where.geo_degrees(p) for p in points.tolist()],
                "distances": dist.tolist(), "matched": matched, "absent": absent}

    # ------------------------------------------------------------------ additive: facet counts and histograms on the device
    _MAX_FACET_VALUES = 1 << 20  # MLVDB_FACET_MAX_VALUES
    _MAX_FACET_EDGES = 4096      # MLVDB_FACET_MAX_EDGES

    def check_facet_args(self, by, order: str = "count", limit: Optional[int] = None, max_values: int = 65536) -> List[str]:
        """The refusals of ``facets`` that need no namespace -> the attributes to facet (``by`` as a list)."""
        names = list(by) if isinstance(by, (list, tuple)) else [by]
        for name in names:
            kind = self._declared(name, "facets: ")
            self._check_sparse("facets", name)
            if kind == "float":
                raise ValueError(f"facets: attribute {name!r} is a float column; value facets need an int, str or bool "
                                 f"attribute (histogram() bins floats)")
        if order not in ("count", "value"):
            raise ValueError(f'facets: order must be "count" or "value" (got {order!r})')
        if limit is not None and not self._int_in(limit, 1):
            raise ValueError(f"facets: limit must be None or an int >= 1 (got {limit!r})")
        if not self._int_in(max_values, 1, self._MAX_FACET_VALUES):
            raise ValueError(f"facets: max_values must be in 1..{self._MAX_FACET_VALUES} (got {max_values!r})")
        return names

    @staticmethod
    def order_facets(pairs: List[tuple], order: str, limit: Optional[int]) -> List[tuple]:
        """(decoded value, count) pairs in the order ``facets`` returns them: by count descending with ties by value
        ascending, or by value ascending; cut to ``limit``."""
        pairs = sorted(pairs, key=(lambda p: (-p[1], p[0])) if order == "count" else (lambda p: p[0]))
        return pairs if limit is None else pairs[:int(limit)]

    def facets(self, namespace: str, by, where: Optional[Mapping] = None, *, limit: Optional[int] = None,
               order: str = "count", max_values: int = 65536):
        """Group-by counts of a declared ``str`` / ``int`` / ``bool`` attribute over the live rows of ``namespace`` (those the
        dict filter ``where`` matches, when one is given), aggregated on the device (include/mlvdb_facet.h):
        ``{"values": [(value, count), ...], "matched": live matching rows, "absent": those of them without a value}``,
        the values decoded (strings, ``True`` / ``False``).  ``order="count"``: by count descending, ties by value
        ascending; ``order="value"``: by value ascending; ``limit`` cuts after ordering.  ``max_values`` bounds the distinct
        values of an ``int`` attribute (more: ``ValueError``); a ``str`` attribute is bounded by its dictionary, a ``bool``
        by two.  ``by`` as a list of attributes returns a dict keyed by attribute (one device pass each).  An unknown or
        empty namespace gives no values and zeros.  A list attribute (``str[]`` / ``int[]``) counts a row under every
        element of its list -- the counts then do not add up to ``matched - absent`` -- and ``absent`` counts the rows with no
        list or an empty one."""
        names = self.check_facet_args(by, order, limit, max_values)
        self._one_filter("facets", where)
        program = self._program(namespace, where)
        ns = self._ns.get(namespace)
        out = {}
        for name in names:
            if self._no_rows(ns):
                out[name] = {"values": [], "matched": 0, "absent": 0}
                continue
            kind = self._attributes[name]
            facet_values = self._engine_entry(ns, "facet_list_values" if _where.is_list(kind) else "facet_values", "facets needs",
                                              named="facet_values")
            bound = max(1, self._group_bound(ns, name, kind, int(max_values)))
            try:
                values, counts, matched, absent = facet_values(self._column(name), bound, where=program)
            except FacetOverflow as e:
                raise ValueError(f"facets: attribute {name!r} holds more than max_values={bound} distinct values among the "
                                 f"{e.matched} matching rows; raise max_values (at most {self._MAX_FACET_VALUES})") from e
            values = self._decode_codes(ns, name, kind, values.tolist())
            out[name] = {"values": self.order_facets(list(zip(values, counts.tolist())), order, limit), "matched": matched,
                         "absent": absent}
        return out if isinstance(by, (list, tuple)) else out[names[0]]

    def check_histogram_args(self, by: str, edges) -> np.ndarray:
        """The refusals of ``histogram`` -> the edges as the column's own type (int64 / float64)."""
        kind = self._declared(by, "histogram: ")
        self._check_scalar("histogram", by)
        if kind not in ("int", "float"):
            raise ValueError(f"histogram: attribute {by!r} is a {kind} column; bins need an int or float attribute")
        edges = edges.tolist() if isinstance(edges, np.ndarray) else list(edges)
        if not 1 <= len(edges) <= self._MAX_FACET_EDGES:
            raise ValueError(f"histogram: 1..{self._MAX_FACET_EDGES} edges (got {len(edges)})")
        for e in edges:  # where.py's literal rules: an int attribute refuses floats, a float one takes ints and floats
            if kind == "int":
                if not isinstance(e, (int, np.integer)):  # (bool is an int)
                    raise ValueError(f"histogram: {by!r} is an int attribute: edge {e!r} is not an int")
                if not -(2 ** 63) < int(e) < 2 ** 63:
                    raise ValueError(f"histogram: edge {e!r} is outside int64 (INT64_MIN marks absent)")
            elif isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, float, np.integer, np.floating)):
                raise ValueError(f"histogram: {by!r} is a float attribute: edge {e!r} is not an int or float")
        out = np.array([int(e) for e in edges], dtype=np.int64) if kind == "int" else \
            np.array([float(e) for e in edges], dtype=np.float64)
        if kind == "float" and np.isnan(out).any():
            raise ValueError("histogram: an edge is NaN")
        if not (out[1:] > out[:-1]).all():
            raise ValueError("histogram: edges must be strictly ascending (unsorted or duplicate edges)")
        return out

    def histogram(self, namespace: str, by: str, edges, where: Optional[Mapping] = None):
        """Bin counts of a declared ``int`` / ``float`` attribute over the live rows of ``namespace`` (those the dict filter
        ``where`` matches, when one is given), on the device: ``{"counts": int64 array [len(edges) + 1], "matched",
        "absent"}`` with ``counts[i]`` = rows whose value has ``i`` edges at or below it (``np.searchsorted(edges, v,
        side="right")``: slot 0 below the first edge, the last slot at or above the last).  ``edges``: 1..4096 strictly
        ascending literals, ints for an ``int`` attribute, ints or floats (not NaN) for a ``float`` one."""
        e = self.check_histogram_args(by, edges)
        self._one_filter("histogram", where)
        program = self._program(namespace, where)
        ns = self._ns.get(namespace)
        if self._no_rows(ns):
            return {"counts": np.zeros(e.size + 1, dtype=np.int64), "matched": 0, "absent": 0}
        counts, matched, absent = self._engine_entry(ns, "facet_bins", "histogram needs")(self._column(by), e, where=program)
        return {"counts": counts, "matched": matched, "absent": absent}

    # ------------------------------------------------------------------ additive: attribute statistics on the device
    def check_stats_args(self, attr, by: Optional[str] = None, max_groups: int = 65536) -> List[str]:
        """The refusals of ``stats`` that need no namespace -> the attributes to summarise (``attr`` as a list)."""
        self._refuse_sharded("stats")
        names = list(attr) if isinstance(attr, (list, tuple)) else [attr]
        for name in names + ([] if by is None else [by]):
            self._declared(name, "stats: ")
            self._check_scalar("stats", name)
        for name in names:
            if self._attributes[name] not in ("int", "float", "bool"):
                raise ValueError(f"stats: attribute {name!r} is a {self._attributes[name]} column; min, max and sum need an "
                                 f"int, float or bool attribute")
        if by is not None and self._attributes[by] == "float":
            raise ValueError(f"stats: by={by!r} is a float column; groups need an int, str or bool attribute")
        if not self._int_in(max_groups, 1, self._MAX_FACET_VALUES):
            raise ValueError(f"stats: max_groups must be in 1..{self._MAX_FACET_VALUES} (got {max_groups!r})")
        return names

    def stats(self, namespace: str, attr, where: Optional[Mapping] = None, by: Optional[str] = None,
              max_groups: int = 65536):
        """Count, min, max, sum and mean of a declared ``int`` / ``float`` / ``bool`` attribute over the live rows of
        ``namespace`` (those the dict filter ``where`` matches, when one is given), aggregated on the device
        (include/mlvdb_stats.h).  Ungrouped: ``{"matched": live matching rows, "count": those with a value, "absent": those
        without, "min", "max", "sum", "mean"}``.  ``by=`` a declared ``int`` / ``str`` / ``bool`` attribute: ``{"groups":
        [(value, {"rows", "count", "min", "max", "sum", "mean"}), ...], "matched", "by_absent"}``, the groups ascending by
        decoded value, ``rows`` the group's matching rows and ``by_absent`` the matching rows without a value of ``by``.
        An ``int`` sum is an exact Python int, a ``bool`` counts as 0 / 1 (``mean`` = the share of true), a ``float`` sum
        is the fixed-point sum of the header -- the same bits whatever the order of the rows, the correctly rounded sum
        when the values lie within a factor 2**9 of the largest; ``mean`` is ``sum / count``.  No value at all: ``min``,
        ``max`` and ``mean`` are ``None``, ``sum`` is 0.  ``max_groups`` bounds the groups of an ``int`` ``by`` (more:
        ``ValueError``); a ``str`` one is bounded by its dictionary, a ``bool`` by two.  ``attr`` as a list of attributes
        returns a dict keyed by attribute (one device call each)."""
        names = self.check_stats_args(attr, by, max_groups)
        self._one_filter("stats", where)
        program = self._program(namespace, where)
        ns = self._ns.get(namespace)
        out = {}
        for name in names:
            kind = self._attributes[name]
            if self._no_rows(ns):
                out[name] = self.shape_stats(kind, by, [], [], 0, 0) if by is not None else \
                    self.shape_stats(kind, None, [None], [(0, 0, None, None, 0)], 0, 0)
                continue
            attr_stats = self._engine_entry(ns, "attr_stats", "stats needs")
            by_kind = None if by is None else self._attributes[by]
            bound = 1 if by is None else max(1, self._group_bound(ns, by, by_kind, int(max_groups)))
            try:
                keys, rows, count, lo, hi, sum_hi, sum_lo, matched, by_absent = attr_stats(
                    self._column(name), None if by is None else self._column(by), bound, where=program)
            except StatsOverflow as e:
                raise ValueError(f"stats: by={by!r} holds more than max_groups={bound} distinct values among the {e.matched} "
                                 f"matching rows; raise max_groups (at most {self._MAX_FACET_VALUES})") from e
            values = self._decode_codes(ns, by, by_kind, keys.tolist())
            groups = [(r, c, a, b, _stats.int128(h, l)) for r, c, a, b, h, l in
                      zip(rows.tolist(), count.tolist(), lo.tolist(), hi.tolist(), sum_hi.tolist(), sum_lo.tolist())]
            out[name] = self.shape_stats(kind, by, values, groups, matched, by_absent)
        return out if isinstance(attr, (list, tuple)) else out[names[0]]

    @staticmethod
    def shape_stats(kind: str, by: Optional[str], values: list, groups: List[tuple], matched: int, by_absent: int) -> dict:
        """The answer of ``stats`` from decoded group values and (rows, count, min, max, exact or fixed-point sum) per
        group; ungrouped (``by is None``): the one group."""
        if by is None:
            rows, count, lo, hi, total = groups[0]
            return {"matched": matched, "absent": matched - count, **_stats.summary(kind, count, lo, hi, total)}
        pairs = [(v, {"rows": g[0], **_stats.summary(kind, *g[1:])}) for v, g in zip(values, groups)]
        return {"groups": sorted(pairs, key=lambda p: p[0]), "matched": matched, "by_absent": by_absent}

    def range_search_many(self, queries, radius: float, namespace: str, metric: str,
                          max_results: int = 1024, where=None) -> List[List[SearchResult]]:
        """The live rows within ``radius`` of each query, nearest first (ties by insertion order), at most
        ``max_results`` per query (the nearest ones; ``None`` = all, up to the engine's 16384 per query).

        ``radius`` is a distance in the namespace's space (squared for l2; plain for
        ``metric="euclidean"``); scores are post-processed exactly like ``search``.
        No reference implementation exists for range queries (README prose only).  ``where``: a dict filter over the
        declared attributes (where.py), evaluated on the device; a list or tuple of ``nq`` entries, each a dict filter or
        ``None`` (unfiltered), gives every query its own filter (one batched call, include/mlvdb_where_each_range.h): each
        query's answer is what a single-dict call for it alone returns.
        """
        programs = of = program = None
        q = self._coerce_queries(queries)
        nq = q.shape[0]
        if isinstance(where, (list, tuple)):
            if len(where) != nq:
                raise ValueError(f"range_search_many: {len(where)} per-query filters for {nq} queries")
            programs, of = self._compile_each(namespace, where)
        elif where is not None:
            program = self._compile(namespace, where)
        ns = self._ns.get(namespace)
        if self._nothing_to_search(ns, nq=nq, dim=q.shape[1]):
            return [[] for _ in range(nq)]
        native_radius = float(radius) ** 2 if metric == "euclidean" else float(radius)
        cap = self._MAX_TOP_K if max_results is None else max(1, int(max_results))
        if programs:
            per_query = self._engine_entry(ns, "range_each", "per-query filters need")(q, native_radius, cap, programs, of,
                                                                                       truncate=True)
        elif program is None:
            per_query = ns.engine.range(q, native_radius, cap, truncate=True)
        else:
            per_query = ns.engine.range(q, native_radius, cap, truncate=True, where=program)
        out: List[List[SearchResult]] = []
        for labels, dist in per_query:
            uids = ns.ids.uuids_at(labels).tolist()
            scores = self._scores(dist, metric).tolist()
            out.append([SearchResult(vector_id=u, score=s) for u, s in zip(uids, scores) if u is not None])
        return out

    # ------------------------------------------------------------------ additive: similarity join
    _MAX_JOIN_PER_ROW = _native.JOIN_MAX_CAPACITY  # MLVDB_JOIN_MAX_CAPACITY: the most partners one row returns

    def check_join_args(self, what: str, metric, radius, where=None, ids=None, max_per_row=1024, order: str = "left") -> float:
        """The refusals of ``join_within`` / ``duplicate_groups`` that need no namespace, in their order; returns the radius
        in the space's own distance (squared for ``metric="euclidean"``)."""
        self._refuse_sharded(what)
        if callable(where) and not isinstance(where, Mapping):
            raise ValueError(f"{what}: where must be one dict filter (a predicate has no device form)")
        self._one_filter(what, where)
        if metric not in _join.METRICS:
            raise ValueError(f"{what}: metric must be one of {_join.METRICS} (got {metric!r})")
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or math.isnan(radius):
            raise ValueError(f"{what}: radius must be a number (got {radius!r})")
        if radius < 0 and metric != "ip":  # (an ip distance is 1 - <a, b>: similar rows lie below zero)
            raise ValueError(f"{what}: radius must be >= 0 for metric {metric!r} (got {radius!r})")
        if not self._int_in(max_per_row, 1, self._MAX_JOIN_PER_ROW):
            raise ValueError(f"{what}: max_per_row must be an int in [1, {self._MAX_JOIN_PER_ROW}] (got {max_per_row!r})")
        if order not in _join.ORDERS:
            raise ValueError(f"{what}: order must be one of {_join.ORDERS} (got {order!r})")
        if ids is not None:
            ids = list(ids)
            if len(set(ids)) != len(ids):
                raise ValueError(f"{what}: ids must not repeat")
        return float(radius) ** 2 if metric == "euclidean" else float(radius)

    def join_within(self, namespace: str, metric: str, radius: float, *, where: Optional[Mapping] = None,
                    ids: Optional[Sequence[UUID]] = None, max_per_row: int = 1024, order: str = "left") -> "_join.PairHits":
        """Additive: which stored rows lie within ``radius`` of each other, answered on the device from the rows in HBM
        (include/mlvdb_join.h) -- near-duplicate detection, record linkage, the neighbourhood graph of a cluster view.

        ``ids=None`` is the self-join: the left rows are the live rows ``where`` matches (all live rows without one), and
        every unordered pair of them within ``radius`` appears once, the earlier-inserted row on the left.  ``ids=[...]``
        asks "what is stored near these stored vectors": per id, every other live row ``where`` matches within ``radius``
        (the ids themselves need not match it), answered in the caller's order; repeated ids are refused.  ``radius`` and
        the scores follow ``range_search_many`` (squared for l2, plain for ``metric="euclidean"``).  At most
        ``max_per_row`` partners per left row come back, the nearest; ``counts`` holds the exact numbers and ``complete``
        says whether any was cut.  ``order="left"``: grouped by left row, nearest first; ``"distance"``: nearest pair
        first over the whole answer (ties by left, then right insertion order).  Every refusal happens before the engine
        is touched.  Returns a ``PairHits``."""
        native_radius = self.check_join_args("join_within", metric, radius, where, ids, max_per_row, order)
        program = self._program(namespace, where)
        ns = self._ns.get(namespace)
        asked = None if ids is None else list(ids)
        labels = None
        if asked is not None and ns is not None:
            labels = ns.ids.lookup(asked) if asked else np.zeros(0, np.int64)
            if (labels < 0).any():
                raise ValueError(f"join_within: id {asked[int(np.argmax(labels < 0))]} is unknown or removed in namespace "
                                 f"{namespace!r}")
        elif asked:
            raise ValueError(f"join_within: id {asked[0]} is unknown or removed in namespace {namespace!r}")
        if self._nothing_to_search(ns):
            return _join.PairHits.empty()
        join = self._engine_entry(ns, "join_within", "join_within needs")
        if labels is None:  # the self-join: every unordered pair once
            left = ns.engine.where_labels(program if program is not None else self._compile(namespace, {}))
            back = np.arange(left.size)
            mode = _native.JOIN_LATER
        else:
            back = np.argsort(labels, kind="stable")  # the engine takes ascending labels; the answer keeps the caller's order
            left = labels[back]
            mode = _native.JOIN_OTHERS
        hits, counts = join(left, mode, native_radius, int(max_per_row), where=program, truncate=True)
        if labels is not None:
            inverse = np.empty_like(back)
            inverse[back] = np.arange(back.size)
            pick = _join.gather_segments(hits.offsets, inverse)
            lens = np.diff(hits.offsets)[inverse]
            right, dist, counts, left = hits.labels[pick], hits.dist[pick], counts[inverse], labels
        else:
            lens = np.diff(hits.offsets)
            right, dist = hits.labels[:int(hits.offsets[-1])], hits.dist[:int(hits.offsets[-1])]
        left_of_pair = np.repeat(left, lens)
        if order == "distance":
            by = np.lexsort((right, left_of_pair, dist))
            left_of_pair, right, dist = left_of_pair[by], right[by], dist[by]
        return _join.PairHits(ns.ids.uuids_at(left_of_pair), ns.ids.uuids_at(right), self._scores(dist, metric), counts,
                              bool((counts <= int(max_per_row)).all()), left_of_pair, right, dist, ns.ids.uuids_at(left))

    def duplicate_groups(self, namespace: str, metric: str, radius: float, *, where: Optional[Mapping] = None,
                         max_per_row: int = 1024) -> List[List[UUID]]:
        """Additive: the groups of near-duplicates -- the connected components (two rows or more) of the self-join's pairs
        (``join_within`` with ``ids=None``), each in insertion order, the groups ordered by their first member.  Raises
        ``JoinOverflow`` when a row has more than ``max_per_row`` partners: a truncated pair list does not determine the
        components."""
        self.check_join_args("duplicate_groups", metric, radius, where, None, max_per_row)
        pairs = self.join_within(namespace, metric, radius, where=where, max_per_row=max_per_row)
        if not pairs.complete:
            raise JoinOverflow(int(max_per_row), int(pairs.counts.max()))
        ns = self._ns.get(namespace)
        return [ns.ids.uuids_at(np.asarray(g, dtype=np.int64)).tolist()
                for g in _join.connected_groups(pairs.left_labels, pairs.right_labels)]

    # ------------------------------------------------------------------ additive: clustering
    _MAX_CLUSTERS = _native.CLUSTER_MAX  # MLVDB_CLUSTER_MAX
    _MAX_CLUSTER_ITERATIONS = _native.CLUSTER_MAX_ITERATIONS

    def _check_cluster_args(self, what: str, metric, metrics, where, assign_to) -> int:
        """The refusals the two clustering entries share that need no namespace, in their order; returns the engine's
        column of ``assign_to`` (-1 without one)."""
        self._refuse_sharded(what)
        if callable(where) and not isinstance(where, Mapping):
            raise ValueError(f"{what}: where must be one dict filter (a predicate has no device form)")
        self._one_filter(what, where)
        if metric not in metrics:
            raise ValueError(f"{what}: metric must be one of {metrics} (got {metric!r})"
                             + (": no mean minimises the inner product; assign_clusters serves it" if metric == "ip" else ""))
        if assign_to is None:
            return -1
        if self._declared(assign_to, f"{what}: assign_to ") != "int":
            raise ValueError(f"{what}: assign_to {assign_to!r} is a {self._attributes[assign_to]} attribute; a cluster id "
                             f"needs an int attribute")
        return self._column(assign_to)

    def _cluster_namespace(self, what: str, namespace: str, metric: str) -> Optional[_Namespace]:
        ns = self._ns.get(namespace)
        space = getattr(ns.engine, "space", metric) if ns is not None else metric
        if space != metric:
            raise ValueError(f"{what}: namespace {namespace!r} is indexed in space {space!r}, not {metric!r}")
        return ns

    def _centroid_array(self, what: str, centroids, ns: Optional[_Namespace]) -> np.ndarray:
        try:
            c = np.ascontiguousarray(centroids, dtype=np.float32)
        except (TypeError, ValueError):
            c = None
        if c is None or c.ndim != 2 or (ns is not None and c.shape[1] != ns.dim) or not np.isfinite(c).all():
            raise ValueError(f"{what}: the centroids must be a finite [k, dim] array of the namespace's dimensionality")
        if not 1 <= c.shape[0] <= self._MAX_CLUSTERS:
            raise ValueError(f"{what}: between 1 and {self._MAX_CLUSTERS} centroids are supported (got {c.shape[0]})")
        return c

    def cluster(self, namespace: str, metric: str, k: int, *, where: Optional[Mapping] = None, init="random", seed: int = 0,
                max_iterations: int = 25, assign_to: Optional[str] = None) -> "_cluster.ClusterResult":
        """Additive: k-means over the stored rows, on the device from the rows in HBM (include/mlvdb_cluster.h) -- "which
        themes does this corpus hold", and a cluster id per row to filter, facet and diversify by.

        The candidates are the live rows ``where`` (one dict filter) matches.  Lloyd's algorithm runs from ``init``:
        ``"random"`` draws ``k`` distinct candidates with ``np.random.default_rng(seed)`` (passed as labels: no vector
        crosses the bus); a sequence of ``k`` UUIDs names stored vectors; a ``[k, dim]`` array gives the centroids
        themselves.  Every iteration assigns each candidate to its nearest centroid (the lowest one on a tie) and moves
        every centroid to the mean of its members -- of its normalised members for "cosine"; a cluster without members
        keeps its centroid.  It stops after the first iteration >= 2 that moves no row, or after ``max_iterations``.
        ``assign_to`` names a declared ``int`` attribute that receives the cluster id of every candidate (no other row is
        touched; the filter is evaluated before anything is written, so it may read ``assign_to`` itself).  Metric "ip" is
        refused: no mean minimises it.  The answer depends on the stored rows and the arguments only.  Every refusal
        happens before the engine is touched.  Returns a ``ClusterResult``."""
        what = "cluster"
        column = self._check_cluster_args(what, metric, _cluster.METRICS, where, assign_to)
        if not self._int_in(k, 1, self._MAX_CLUSTERS):
            raise ValueError(f"{what}: k must be an int in [1, {self._MAX_CLUSTERS}] (got {k!r})")
        if not self._int_in(max_iterations, 1, self._MAX_CLUSTER_ITERATIONS):
            raise ValueError(f"{what}: max_iterations must be an int in [1, {self._MAX_CLUSTER_ITERATIONS}] (got {max_iterations!r})")
        k = int(k)
        program = self._program(namespace, where)
        ns = self._cluster_namespace(what, namespace, metric)
        labels = vectors = None
        if isinstance(init, str):
            if init != "random":
                raise ValueError(f'{what}: init must be "random", a sequence of ids or a [k, dim] array (got {init!r})')
            if not self._int_in(seed, 0):
                raise ValueError(f"{what}: seed must be an int >= 0 (got {seed!r})")
            live = 0 if ns is None else ns.total - ns.deleted
            pool = None
            if live >= k and program is not None:  # (only a filter can leave fewer candidates than live rows)
                pool = ns.engine.where_labels(program)
                live = int(pool.size)
            if live < k:
                raise ValueError(f"{what}: k = {k} centroids but only {live} candidate rows in namespace {namespace!r}")
            if pool is None:
                pool = ns.engine.where_labels(self._compile(namespace, {}))
            labels = np.sort(np.random.default_rng(int(seed)).choice(pool, k, replace=False)).astype(np.int64)
        elif isinstance(init, (bytes, UUID)) or not isinstance(init, (SequenceABC, np.ndarray)):
            raise ValueError(f'{what}: init must be "random", a sequence of ids or a [k, dim] array (got {init!r})')
        elif len(init) > 0 and all(isinstance(e, UUID) for e in init):
            ids = list(init)
            if len(ids) != k:
                raise ValueError(f"{what}: k = {k} but init names {len(ids)} ids")
            labels = ns.ids.lookup(ids) if ns is not None else np.full(len(ids), -1, np.int64)
            if (labels < 0).any():
                raise ValueError(f"{what}: id {ids[int(np.argmax(labels < 0))]} is unknown or removed in namespace {namespace!r}")
        else:
            vectors = self._centroid_array(what, init, ns)
            if vectors.shape[0] != k:
                raise ValueError(f"{what}: k = {k} but init holds {vectors.shape[0]} centroids")
        if self._no_rows(ns):
            return _cluster.ClusterResult.of(vectors, np.zeros(k, np.int64), np.zeros(k), min(2, int(max_iterations)),
                                             max_iterations >= 2)
        kmeans = self._engine_entry(ns, "kmeans", f"{what} needs")
        centroids, sizes, costs, iterations, converged, _ = kmeans(labels, vectors, max_iterations=int(max_iterations),
                                                                    where=program, assign_attr=column)
        return _cluster.ClusterResult.of(centroids, sizes, costs, iterations, converged)

    def assign_clusters(self, namespace: str, metric: str, centroids, assign_to: Optional[str] = None,
                        where: Optional[Mapping] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Additive: every live row ``where`` matches to the nearest of the given ``[k, dim]`` centroids (the lowest one on
        a tie), on the device -- "assign the rows I just appended to the centroids I already have".  ``assign_to`` (a
        declared ``int`` attribute) receives the cluster ids as in ``cluster``.  Works for "l2", "cosine" and "ip".
        Returns (sizes int64 [k], costs float64 [k]) as ``ClusterResult`` holds them."""
        what = "assign_clusters"
        column = self._check_cluster_args(what, metric, _cluster.ASSIGN_METRICS, where, assign_to)
        program = self._program(namespace, where)
        ns = self._cluster_namespace(what, namespace, metric)
        vectors = self._centroid_array(what, centroids, ns)
        if self._no_rows(ns):
            return np.zeros(vectors.shape[0], np.int64), np.zeros(vectors.shape[0])
        assign = self._engine_entry(ns, "assign_nearest", f"{what} needs")
        sizes, costs, _ = assign(None, vectors, where=program, assign_attr=column)
        return sizes, costs

    def _int_attribute_of(self, namespace: str, name: str, ids: Sequence[UUID]) -> List[Optional[int]]:
        """The value of the declared ``int`` attribute ``name`` of every stored vector in ``ids`` (``None``: no value, or an
        unknown or removed id).  For ``QueryProcessor``'s clustering entries, which copy a freshly written cluster column
        into the stored metadata of (usually) every row: the whole column comes down in one read, 8 B per row."""
        if self._declared(name) != "int":
            raise ValueError(f"_int_attribute_of: {name!r} is a {self._attributes[name]} attribute")
        ids = list(ids)
        ns = self._ns.get(namespace)
        if self._no_rows(ns) or not ids:
            return [None] * len(ids)
        labels = ns.ids.lookup(ids)
        column = ns.engine.get_attr(self._column(name), 0, ns.total)
        values = np.where(labels >= 0, column[np.maximum(labels, 0)], _where.INT64_ABSENT)
        return [None if v == _where.INT64_ABSENT else int(v) for v in values.tolist()]

    # ------------------------------------------------------------------ helpers
    @staticmethod
    def _coerce_queries(queries) -> np.ndarray:
        if isinstance(queries, np.ndarray):
            q = queries.astype(np.float32, copy=False)
        else:
            q = np.array([np.asarray(getattr(v, "values", v), dtype=np.float32) for v in queries], dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :] if q.size else q.reshape(0, 0)
        return np.ascontiguousarray(q)

    @staticmethod
    def _search_engine(ns: _Namespace, q: np.ndarray, k: int, mask=None):
        """Engines select at most ``max_topk`` per scan; larger k is served in rank-ordered pages."""
        return ns.engine.search(q, k) if mask is None else ns.engine.search(q, k, mask)

    def namespace_counts(self, namespace: str):
        ns = self._ns.get(namespace)
        return (0, 0) if ns is None else (ns.total, ns.deleted)

    def fetch_values(self, namespace: str, labels: np.ndarray) -> np.ndarray:
        """Additive: the stored float32 rows of ``labels`` read back from the index's own copy in HBM (bit-exact), so a
        caller that keeps no second copy of the corpus on the host can still enrich hits with ``values``."""
        ns = self._ns[namespace]
        return ns.engine.get_rows_at(np.asarray(labels, dtype=np.int64))

    def distances(self, queries, ids, namespace: str, metric: str) -> np.ndarray:
        """Additive (SURVEY 8a row a8': the vector-level ``distance()`` / ``similarity()`` of reference README.md:30-41,
        178-181, on the device): the score ``search`` reports for each pair (queries[q], stored vector ids[q][j]) --
        float64 array ``[nq, m]`` of the float32-rounded distance in the namespace's space, post-processed like
        ``search`` (``1 - d`` for metric "cosine", sqrt for "euclidean").  ``ids`` is ``[nq][m]`` UUIDs or an int64 label
        array; unknown / removed ids give NaN.  Computed by the kernels' own fp64 summation over the rows in HBM, so
        ``distances(q, [hit.vector_id])`` equals that hit's score exactly."""
        q = self._coerce_queries(queries)
        ns = self._ns.get(namespace)
        if ns is None or q.shape[1] != ns.dim:
            raise RuntimeError(f"namespace {namespace!r} is unknown or its dimensionality differs from the queries'")
        if isinstance(ids, np.ndarray) and ids.dtype.kind in "iu":
            labels = np.asarray(ids, dtype=np.int64).reshape(q.shape[0], -1).copy()
            inside = (labels >= 0) & (labels < ns.ids.n)
            dead = np.zeros(labels.shape, dtype=bool)
            dead[inside] = ~ns.ids.live[labels[inside]]
            labels[dead | ~inside] = -1  # removed or unknown labels read as NaN, like removed ids (the engine itself would score them)
        else:
            rows = [list(r) for r in ids]
            m = len(rows[0]) if rows else 0
            if any(len(r) != m for r in rows) or len(rows) != q.shape[0]:
                raise RuntimeError("ids must hold the same number of ids for every query")
            labels = ns.ids.lookup([u for r in rows for u in r]).reshape(q.shape[0], m)
        known = labels >= 0
        _, d32 = ns.engine.pair_distances(q, np.where(known, labels, -1))
        out = self._scores(d32, metric)
        out[~known] = np.nan
        return out

    def fetch_values_by_id(self, namespace: str, ids: Sequence[UUID]) -> np.ndarray:
        """``fetch_values`` addressed by id (every id must be live in the namespace)."""
        ns = self._ns[namespace]
        labels = ns.ids.lookup(ids)
        if (labels < 0).any():
            raise RuntimeError("fetch_values_by_id: unknown or removed id")
        return ns.engine.get_rows_at(labels)

    # ------------------------------------------------------------------ additive: persistence
    # Directory layout ("mlvdb-index-v1"): index.json + per namespace i
    #   ns<i>.rows.f32     raw row-major float32 [total, dim], every label incl. tombstoned ones (labels stay stable)
    #   ns<i>.ids.u8       [total, 16] UUID bytes, all-zero for tombstoned labels
    # The fp32 rows are the ones the device holds (bit-exact round trip); norms, bf16 shadow and panel layout are
    # rebuilt by the ingest kernels at load.  No reference behaviour (README.md:240-241 names the two methods only).
    # An index with attributes writes "mlvdb-index-v2": v1 + per namespace i and attribute j
    #   ns<i>.attr<j>.i64 / .f64   the raw device column [total] (int64, INT64_MIN = absent / float64, NaN = absent)
    # and in index.json "attributes" (name -> type, in column order) and per namespace "strings" (str attribute -> its
    # dictionary, code order).  An index without attributes writes exactly v1.
    _FORMAT = "mlvdb-index-v1"
    _FORMAT_V2 = "mlvdb-index-v2"
    _FORMAT_V3 = "mlvdb-index-v3"  # v2 + per list attribute the live rows' lists in CSR form (offsets.i64, values.i64)
    # v3 + per sparse attribute the live rows' vectors in CSR form (offsets.i64, terms.i32, weights.f32); written only by
    # an index that declares a sparse attribute
    _FORMAT_V4 = "mlvdb-index-v4"
    # the layout the index would otherwise write (v2, v3 or v4) with a "geo" attribute in the schema, whose column file is
    # the raw int64 column (packed points, INT64_MIN = absent); written only by an index that declares a geo attribute
    _FORMAT_V5 = "mlvdb-index-v5"
    # v5's layout with a "bits<N>" attribute in the schema, whose column file holds 1 / 0 (INT64_MIN) presence and whose
    # .bits.u64 holds the present live rows' codes, dense, in row order; written only by an index that declares one
    _FORMAT_V6 = "mlvdb-index-v6"
    _CHUNK_BYTES = 256 << 20

    def save_index(self, path: str) -> bool:
        """Write every namespace to directory ``path`` (created if missing); streams the rows off the device in
        chunks, so host memory stays bounded."""
        os.makedirs(path, exist_ok=True)
        has_lists = any(_where.is_list(kind) for kind in self._attributes.values())
        has_sparse = any(_where.is_sparse(kind) for kind in self._attributes.values())
        has_geo = any(_where.is_geo(kind) for kind in self._attributes.values())
        has_bits = any(_where.is_bits(kind) for kind in self._attributes.values())
        fmt = self._FORMAT_V6 if has_bits else self._FORMAT_V5 if has_geo else self._FORMAT_V4 if has_sparse else self._FORMAT_V3 if has_lists else self._FORMAT_V2 if self._attributes else \
            self._FORMAT
        meta = {"format": fmt, "space": self._space,
                "rebuild_threshold": self._rebuild_threshold, "namespaces": []}
        if self._attributes:
            meta["attributes"] = dict(self._attributes)
        for i, (name, ns) in enumerate(self._ns.items()):
            chunk = max(1, self._CHUNK_BYTES // (4 * ns.dim))
            with open(os.path.join(path, f"ns{i}.rows.f32"), "wb") as f:
                for first in range(0, ns.total, chunk):
                    f.write(ns.engine.get_rows(first, min(chunk, ns.total - first)).tobytes())
            dead = ns.ids.dead_labels()
            ids = ns.ids.raw[:ns.total].copy()
            ids[dead] = 0
            ids.tofile(os.path.join(path, f"ns{i}.ids.u8"))
            dead.tofile(os.path.join(path, f"ns{i}.deleted.i64"))
            entry = {"name": name, "dim": ns.dim, "space": ns.engine.space, "total": ns.total,
                     "deleted": ns.deleted, "rebuild_required": ns.rebuild_required}
            if self._attributes:
                for j, kind in enumerate(self._attributes.values()):
                    col = self._attr_file(path, i, j, kind)
                    if _where.is_list(kind):
                        self._save_list(ns, j, col, dead)
                        continue
                    if _where.is_sparse(kind):
                        self._save_sparse(ns, j, col, dead)
                        continue
                    if _where.is_bits(kind):
                        self._save_bits(ns, j, col, dead, _where.bits_width(kind) // 64)
                        continue
                    dtype = np.float64 if kind == "float" else np.int64
                    (ns.engine.get_attr(j, 0, ns.total, dtype) if ns.total else np.zeros(0, dtype)).tofile(col)
                entry["strings"] = {a: sorted(codes, key=codes.get) for a, codes in ns.strings.items()}
            meta["namespaces"].append(entry)
        tmp = os.path.join(path, "index.json.tmp")
        with open(tmp, "w") as f:
            json.dump(meta, f, indent=1)
        os.replace(tmp, os.path.join(path, "index.json"))  # the manifest appears last and atomically
        return True

    @classmethod
    def _save_list(cls, ns: _Namespace, j: int, col_file: str, dead: np.ndarray) -> None:
        """A list attribute of a v3 snapshot: the column file holds each row's length (INT64_MIN: no list), and next to it
        ``.offsets.i64`` / ``.values.i64`` hold the lists of the live rows in CSR form -- what the rows hold now, not the
        device pool with its overwritten lists; a tombstoned row is written without a list."""
        lens = np.full(ns.total, _where.INT64_ABSENT, dtype=np.int64)
        offsets = np.zeros(ns.total + 1, dtype=np.int64)
        parts = []
        chunk = 1 << 20
        for first in range(0, ns.total, chunk):
            n = min(chunk, ns.total - first)
            got = cls._engine_entry(ns, "get_attr_list", "list attributes need")(j, first, n)
            live = got.present.astype(bool)
            live[dead[(dead >= first) & (dead < first + n)] - first] = False
            rows = np.flatnonzero(live)
            kept = got.take(rows)
            n_each = np.zeros(n, dtype=np.int64)
            n_each[rows] = kept.offsets[1:] - kept.offsets[:-1]
            lens[first:first + n][live] = n_each[live]
            offsets[first + 1:first + n + 1] = offsets[first] + np.cumsum(n_each)
            parts.append(kept.values)
        lens.tofile(col_file)
        offsets.tofile(col_file[:-len("i64")] + "offsets.i64")
        (np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)).astype(np.int64).tofile(
            col_file[:-len("i64")] + "values.i64")

    @classmethod
    def _save_sparse(cls, ns: _Namespace, j: int, col_file: str, dead: np.ndarray) -> None:
        """A sparse attribute of a v4 snapshot: the column file holds each row's number of nonzeros (INT64_MIN: no vector),
        and next to it ``.offsets.i64`` / ``.terms.i32`` / ``.weights.f32`` hold the vectors of the live rows in CSR form;
        a tombstoned row is written without a vector."""
        lens = np.full(ns.total, _where.INT64_ABSENT, dtype=np.int64)
        offsets = np.zeros(ns.total + 1, dtype=np.int64)
        terms, weights = [], []
        chunk = 1 << 20
        for first in range(0, ns.total, chunk):
            n = min(chunk, ns.total - first)
            got = cls._engine_entry(ns, "get_attr_sparse", "sparse attributes need")(j, first, n)
            live = got.present.astype(bool)
            live[dead[(dead >= first) & (dead < first + n)] - first] = False
            rows = np.flatnonzero(live)
            kept = got.take(rows)
            n_each = np.zeros(n, dtype=np.int64)
            n_each[rows] = kept.offsets[1:] - kept.offsets[:-1]
            lens[first:first + n][live] = n_each[live]
            offsets[first + 1:first + n + 1] = offsets[first] + np.cumsum(n_each)
            terms.append(kept.terms)
            weights.append(kept.weights)
        base = col_file[:-len("i64")]
        lens.tofile(col_file)
        offsets.tofile(base + "offsets.i64")
        (np.concatenate(terms) if terms else np.zeros(0, np.int32)).astype(np.int32).tofile(base + "terms.i32")
        (np.concatenate(weights) if weights else np.zeros(0, np.float32)).astype(np.float32).tofile(base + "weights.f32")

    @classmethod
    def _save_bits(cls, ns: _Namespace, j: int, col_file: str, dead: np.ndarray, words: int) -> None:
        """A bits attribute of a v6 snapshot: the column file holds 1 for a live row with a code (INT64_MIN: none), and next
        to it ``.bits.u64`` holds those rows' codes, ``words`` words each, in row order; a tombstoned row is written without a
        code, and so is a row whose code has another width (only the raw C entries can write one)."""
        has = np.full(ns.total, _where.INT64_ABSENT, dtype=np.int64)
        parts = []
        chunk = 1 << 20
        for first in range(0, ns.total, chunk):
            n = min(chunk, ns.total - first)
            widths, codes = cls._engine_entry(ns, "bits_get", "bits attributes need")(j, first, n)
            starts = np.concatenate([[0], np.cumsum(widths, dtype=np.int64)])[:-1]
            live = widths == words
            live[dead[(dead >= first) & (dead < first + n)] - first] = False
            rows = np.flatnonzero(live)
            has[first + rows] = 1
            parts.append(codes[(starts[rows][:, None] + np.arange(words)[None, :]).ravel()] if rows.size
                         else np.zeros(0, dtype=np.uint64))
        has.tofile(col_file)
        (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)).astype("<u8").tofile(
            col_file[:-len("i64")] + "bits.u64")

    @staticmethod
    def _attr_file(path: str, i: int, j: int, kind: str) -> str:
        return os.path.join(path, f"ns{i}.attr{j}.{'f64' if kind == 'float' else 'i64'}")

    def load_index(self, path: str) -> bool:
        """Replace the contents of this index by the directory written by ``save_index``.  Returns False (index
        untouched) when ``path`` holds no manifest; raises ``RuntimeError`` on a manifest it cannot honour."""
        manifest = os.path.join(path, "index.json")
        if not os.path.isfile(manifest):
            return False
        with open(manifest) as f:
            meta = json.load(f)
        if meta.get("format") not in (self._FORMAT, self._FORMAT_V2, self._FORMAT_V3, self._FORMAT_V4, self._FORMAT_V5,
                                      self._FORMAT_V6):
            raise RuntimeError(f"unknown index format {meta.get('format')!r}")
        # (v3: v2 with list attributes, v4: v3 with sparse attributes, v5: any of them with geo attributes, v6: any of them
        # with bits attributes)
        v2 = meta["format"] in (self._FORMAT_V2, self._FORMAT_V3, self._FORMAT_V4, self._FORMAT_V5, self._FORMAT_V6)
        v5 = meta["format"] in (self._FORMAT_V5, self._FORMAT_V6)
        if v2 and not v5 and any(_where.is_geo(k) for k in meta.get("attributes", {}).values()):
            raise RuntimeError(f"a geo attribute in a {meta['format']} snapshot: only {self._FORMAT_V5} and later hold them")
        if v2 and meta["format"] != self._FORMAT_V6 and any(_where.is_bits(k) for k in meta.get("attributes", {}).values()):
            raise RuntimeError(f"a bits attribute in a {meta['format']} snapshot: only {self._FORMAT_V6} holds them")
        # v2: the snapshot's attributes replace the declared ones; v1: the declared ones stay, every value absent
        attributes = self._check_schema(meta.get("attributes", {})) if v2 else self._attributes
        if v2 and attributes:
            self._refuse_sharded("attributes=")
        for i, m in enumerate(meta["namespaces"]):  # validate sizes before touching anything
            total, dim = int(m["total"]), int(m["dim"])
            if os.path.getsize(os.path.join(path, f"ns{i}.rows.f32")) != total * dim * 4 or \
                    os.path.getsize(os.path.join(path, f"ns{i}.ids.u8")) != total * 16:
                raise RuntimeError(f"namespace {m['name']!r}: file sizes do not match the manifest")
            if v2 and any(os.path.getsize(self._attr_file(path, i, j, kind)) != total * 8
                          for j, kind in enumerate(attributes.values())):
                raise RuntimeError(f"namespace {m['name']!r}: attribute file sizes do not match the manifest")
            for j, kind in enumerate(attributes.values()):
                if v2 and _where.is_list(kind):
                    base = self._attr_file(path, i, j, kind)[:-len("i64")]
                    if meta["format"] not in (self._FORMAT_V3, self._FORMAT_V4, self._FORMAT_V5, self._FORMAT_V6) or \
                            not os.path.isfile(base + "values.i64") or \
                            not os.path.isfile(base + "offsets.i64") or \
                            os.path.getsize(base + "offsets.i64") != (total + 1) * 8:
                        raise RuntimeError(f"namespace {m['name']!r}: list attribute files do not match the manifest")
                if v2 and _where.is_sparse(kind):
                    base = self._attr_file(path, i, j, kind)[:-len("i64")]
                    if meta["format"] not in (self._FORMAT_V4, self._FORMAT_V5, self._FORMAT_V6) or \
                            not os.path.isfile(base + "terms.i32") or \
                            not os.path.isfile(base + "weights.f32") or not os.path.isfile(base + "offsets.i64") or \
                            os.path.getsize(base + "offsets.i64") != (total + 1) * 8 or \
                            os.path.getsize(base + "terms.i32") != os.path.getsize(base + "weights.f32"):
                        raise RuntimeError(f"namespace {m['name']!r}: sparse attribute files do not match the manifest")
                if v2 and _where.is_bits(kind):
                    base = self._attr_file(path, i, j, kind)[:-len("i64")]
                    held = int((np.fromfile(base + "i64", dtype=np.int64) != _where.INT64_ABSENT).sum())
                    if not os.path.isfile(base + "bits.u64") or \
                            os.path.getsize(base + "bits.u64") != held * (_where.bits_width(kind) // 8):
                        raise RuntimeError(f"namespace {m['name']!r}: bits attribute files do not match the manifest")
        self.close()
        self._attributes = attributes
        self._space = meta["space"]
        self._rebuild_threshold = float(meta["rebuild_threshold"])
        for i, m in enumerate(meta["namespaces"]):
            total, dim = int(m["total"]), int(m["dim"])
            ns = self._get_or_create(m["name"], dim, m["space"])
            if total:
                rows = np.memmap(os.path.join(path, f"ns{i}.rows.f32"), dtype=np.float32, mode="r", shape=(total, dim))
                chunk = max(1, self._CHUNK_BYTES // (4 * dim))
                for first in range(0, total, chunk):
                    if ns.engine.append(np.ascontiguousarray(rows[first:first + chunk])) != first:
                        raise RuntimeError("engine label base does not match the file offset")
                del rows
            deleted = np.fromfile(os.path.join(path, f"ns{i}.deleted.i64"), dtype=np.int64)
            if deleted.size:
                ns.engine.tombstone(deleted)
            ns.ids.append_raw(np.fromfile(os.path.join(path, f"ns{i}.ids.u8"), dtype=np.uint8).reshape(total, 16))
            ns.ids.kill(deleted)
            if v2:
                for j, kind in enumerate(attributes.values()):
                    col = np.fromfile(self._attr_file(path, i, j, kind), dtype=np.float64 if kind == "float" else np.int64)
                    if col.size and _where.is_list(kind):
                        base = self._attr_file(path, i, j, kind)[:-len("i64")]
                        lists = _where.ListColumn(np.fromfile(base + "offsets.i64", dtype=np.int64),
                                                  np.fromfile(base + "values.i64", dtype=np.int64),
                                                  (col != _where.INT64_ABSENT).astype(np.uint8))
                        self._engine_entry(ns, "set_attr_list", "list attributes need")(j, 0, lists)
                    elif col.size and _where.is_sparse(kind):
                        base = self._attr_file(path, i, j, kind)[:-len("i64")]
                        vectors = _where.SparseColumn(np.fromfile(base + "offsets.i64", dtype=np.int64),
                                                      np.fromfile(base + "terms.i32", dtype=np.int32),
                                                      np.fromfile(base + "weights.f32", dtype=np.float32),
                                                      (col != _where.INT64_ABSENT).astype(np.uint8))
                        self._engine_entry(ns, "set_attr_sparse", "sparse attributes need")(j, 0, vectors)
                    elif col.size and _where.is_bits(kind):
                        present = (col != _where.INT64_ABSENT).astype(np.uint8)
                        words = _where.bits_width(kind) // 64
                        dense = np.fromfile(self._attr_file(path, i, j, kind)[:-len("i64")] + "bits.u64", dtype="<u8")
                        codes = np.zeros((total, words), dtype=np.uint64)
                        codes[present.astype(bool)] = dense.reshape(-1, words)
                        self._engine_entry(ns, "bits_set", "bits attributes need")(j, 0, _where.BitsColumn(codes, present))
                    elif col.size:
                        ns.engine.set_attr(j, 0, col)
                ns.strings = {a: {s: c for c, s in enumerate(values)} for a, values in m.get("strings", {}).items()}
            ns.total = total
            ns.deleted = int(m["deleted"])
            ns.rebuild_required = bool(m["rebuild_required"])
        return True

    def close(self) -> None:
        for ns in self._ns.values():
            ns.engine.close()
        self._ns.clear()
