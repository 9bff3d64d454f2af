"""``QueryProcessor``: storage + index orchestration around the search hot path.

Counterpart of the reference's ``QueryProcessor``
(src/mlvectordb/implementations/query_processor.py:11-82).  ``find_similar`` is the
dispatch the north star names: ``Index.search`` then enrichment of each hit with the stored
values/metadata, in index order, silently dropping ids the storage no longer has
(query_processor.py:33-49).  ``find_similar_many`` is the additive batched sibling: one
corpus scan for the whole query batch.

Deliberate divergence: the reference's ``delete`` rebuilds the index
from *only* the affected namespace (query_processor.py:60), and ``Index.rebuild`` clears
every namespace first (index.py:136-143), so other namespaces silently vanish from the
index.  Here the rebuild source is the whole storage map; pass ``rebuild_scope="namespace"``
to reproduce the reference byte for byte.
"""
from __future__ import annotations

import numpy as np
from collections.abc import Mapping
from typing import Any, Dict, Iterable, List, Optional, Sequence
from uuid import UUID

from . import stats as _stats
from .interfaces import IndexProtocol, VectorDTO
from .vector import Vector


class QueryProcessor:
    def __init__(self, storage_engine, index: IndexProtocol, *, rebuild_scope: str = "all") -> None:
        if rebuild_scope not in ("all", "namespace"):
            raise ValueError("rebuild_scope must be 'all' or 'namespace'")
        self._storage = storage_engine
        self._index = index
        self._rebuild_scope = rebuild_scope

    # ---- writes (query_processor.py:16-24): every call mints new ids; update_metadata / update_where change metadata in place
    def insert(self, vector: VectorDTO, namespace: str = "default") -> None:
        row = Vector(values=vector.values, metadata=vector.metadata)
        self._storage.write(row, namespace)
        self._index.add([row], namespace)

    def upsert_many(self, vectors: Iterable[VectorDTO], namespace: str = "default") -> None:
        rows = [Vector(values=v.values, metadata=v.metadata) for v in vectors]
        self._storage.write_vectors(rows, namespace)
        self._index.add(rows, namespace)

    # ---- the hot path
    def _enrich(self, hits, namespace: str) -> List[dict]:
        if not hits:
            return []
        stored = {v.id: v for v in self._storage.read_vectors([h.vector_id for h in hits], namespace) if v}
        out = []
        for h in hits:
            v = stored.get(h.vector_id)
            if v:
                out.append({"id": v.id, "values": v.values, "metadata": v.metadata, "score": h.score})
        return out

    def find_similar(self, query: VectorDTO, top_k: int, namespace: str = "default",
                     metric: str = "cosine") -> List[dict]:
        if hasattr(self._storage, "read_rows_raw") and hasattr(self._index, "search_many"):
            values = np.asarray(query.values, dtype=np.float32)  # array-backed storage: the one-row case of the batch path
            if values.ndim != 1:
                return []
            return self._enrich_many(self._index.search_many(values[None, :], top_k, namespace, metric), namespace)[0]
        hits = self._index.search(query, top_k=top_k, namespace=namespace, metric=metric)
        return self._enrich(hits, namespace)

    def find_similar_many(self, queries, top_k: int, namespace: str = "default",
                          metric: str = "cosine", where=None, distinct=None, mmr_lambda=None,
                          fetch_k=None, group_size=None) -> List[List[dict]]:
        """Batched ``find_similar``: ``queries`` is an [nq, dim] array or a sequence of VectorDTO.

        ``where`` (additive; README.md:121,130,252,274 intent, no reference code) restricts the search to the matching
        vectors -- the exact top-k among them, not a post-filter of an unrestricted top-k:
          - a dict filter over the index's declared attributes (``Index(attributes=...)``, where.py): compiled once and
            evaluated on the device into the row mask; nothing per row happens on the host;
          - a predicate over a stored vector's metadata dict: evaluated once over the namespace's stored vectors and
            handed to the index as a row mask;
          - a list of ``nq`` entries, each a dict filter or ``None``: every query its own filter, all evaluated on the
            device in one batched call (``Index.search_many``); a predicate inside the list is a ``ValueError``.
        ``distinct`` (additive: a declared ``int`` / ``str`` / ``bool`` attribute of the index) returns one hit per value of
        that attribute: the nearest vector of each of the ``top_k`` (<= 64) nearest groups (``Index.search_many``).  With
        it ``where`` is ``None`` or one dict filter.  ``group_size`` (additive, with ``distinct``: an int in [1, 64]) returns
        the ``group_size`` nearest vectors of each of those groups instead of one: per query the groups in rank order, each
        group's members in order, the usual dict per hit.
        ``mmr_lambda`` (additive: a number in [0, 1]; ``fetch_k``: its candidate count) diversifies the hits by maximal
        marginal relevance among the ``fetch_k`` nearest vectors, selected on the device (``Index.search_many``); hits
        come back in pick order.  With it ``where`` is ``None`` or one dict filter, and ``distinct`` is not allowed."""
        if group_size is not None:
            if distinct is None:
                raise ValueError("find_similar_many: group_size is the member count of distinct=, give both or neither")
            if where is not None and not isinstance(where, Mapping):
                raise ValueError("distinct: where must be one dict filter (or None)")
            hits = self._index.search_many(queries, top_k=top_k, namespace=namespace, metric=metric, where=where,
                                           distinct=distinct, mmr_lambda=mmr_lambda, fetch_k=fetch_k, group_size=group_size)
            return self._enrich_many(hits, namespace)
        if mmr_lambda is not None or fetch_k is not None:
            if where is not None and not isinstance(where, (Mapping, list, tuple)):
                raise ValueError("mmr_lambda: a predicate where (allowed_ids) is not supported, give a dict where filter")
            hits = self._index.search_many(queries, top_k=top_k, namespace=namespace, metric=metric, where=where,
                                           distinct=distinct, mmr_lambda=mmr_lambda, fetch_k=fetch_k)
            return self._enrich_many(hits, namespace)
        if distinct is not None:
            if where is not None and not isinstance(where, Mapping):
                raise ValueError("distinct: where must be one dict filter (or None)")
            hits = self._index.search_many(queries, top_k=top_k, namespace=namespace, metric=metric, where=where,
                                           distinct=distinct)
            return self._enrich_many(hits, namespace)
        return self._enrich_many(self._search_many(queries, top_k, namespace, metric, where), namespace)

    def find_similar_to(self, positive_ids: Sequence[UUID], top_k: int, namespace: str = "default", metric: str = "cosine", *,
                        negative_ids: Optional[Sequence[UUID]] = None, query=None, where=None) -> List[dict]:
        """Additive: "more like this" -- the neighbours of stored vectors named by id (``Index.search_like``): of the mean
        of ``positive_ids``, pushed away from the mean of ``negative_ids`` when given, on top of ``query`` (a ``VectorDTO``
        or a row of values, e.g. a text query's embedding) when given.  The named vectors never come back as hits; the
        query is built and searched on the device.  ``where`` is ``None`` or one dict filter."""
        queries = None if query is None else np.asarray(getattr(query, "values", query), dtype=np.float32)[None, :]
        return self.find_similar_to_many([list(positive_ids)], top_k, namespace, metric, queries=queries, where=where,
                                         negative_ids=None if negative_ids is None else [list(negative_ids)])[0]

    def find_similar_to_many(self, positive_ids, top_k: int, namespace: str = "default", metric: str = "cosine", *,
                             negative_ids=None, queries=None, where=None) -> List[List[dict]]:
        """Batched ``find_similar_to``: one sequence of ids per query (``Index.search_like``)."""
        if where is not None and not isinstance(where, Mapping):
            raise ValueError("find_similar_to: where must be one dict filter (or None)")
        if not hasattr(self._index, "search_like"):
            raise ValueError("find_similar_to needs an index with search_like")
        hits = self._index.search_like(positive_ids, top_k, namespace, metric, negative=negative_ids, queries=queries,
                                       where=where)
        return self._enrich_many(hits, namespace)

    def find_documents(self, query_tokens, top_k: int, namespace: str, by: str, metric: str = "cosine", where=None,
                       with_matches: bool = False) -> List[dict]:
        """Additive: late-interaction (MaxSim) search for one query given as a bag of token vectors (``[T, dim]``, 1..128
        tokens; ``Index.search_late``): the ``top_k`` (<= 64) documents -- values of the declared attribute ``by`` -- ranked by
        the sum, over the tokens, of each token's score against the document's best vector.  One dict per document in rank
        order: ``value``, ``score`` and, with ``with_matches``, ``matches``: per token the matched vector as
        ``find_similar_many`` returns a hit.  ``where`` is ``None`` or one dict filter."""
        if where is not None and not isinstance(where, Mapping):
            raise ValueError("find_documents: where must be one dict filter (or None)")
        if not hasattr(self._index, "search_late"):
            raise ValueError("find_documents needs an index with search_late")
        docs = self._index.search_late([query_tokens], top_k, namespace, metric, by, where=where, matches=with_matches)[0]
        out = []
        for doc in docs:
            entry = {"value": doc.value, "score": doc.score}
            if with_matches:
                entry["matches"] = self._enrich(doc.matches, namespace)
            out.append(entry)
        return out

    def find_similar_sparse(self, query, top_k: int, namespace: str = "default", by: str = "", where=None) -> List[dict]:
        """Additive: lexical search for one sparse query -- a mapping ``{term: weight}`` or a pair ``(indices, values)`` --
        over the declared ``sparse`` attribute ``by`` (``Index.search_sparse``): the ``top_k`` (<= 64) vectors with the
        largest inner product, as ``find_similar_many`` returns a hit (``score``: the dot product)."""
        return self.find_similar_sparse_many([query], top_k, namespace, by, where=where)[0]

    def find_similar_sparse_many(self, queries, top_k: int, namespace: str = "default", by: str = "",
                                 where=None) -> List[List[dict]]:
        """Batched ``find_similar_sparse``: one sparse vector per query, one scan.  ``where`` is ``None`` or one dict filter."""
        if where is not None and not isinstance(where, Mapping):
            raise ValueError("find_similar_sparse: where must be one dict filter (or None)")
        if not hasattr(self._index, "search_sparse"):
            raise ValueError("find_similar_sparse needs an index with search_sparse")
        return self._enrich_many(self._index.search_sparse(queries, top_k, namespace, by, where=where), namespace)

    def find_similar_bits(self, query, top_k: int, namespace: str = "default", by: str = "", metric: str = "hamming",
                          where=None) -> List[dict]:
        """Additive: search for one bit code -- ``bytes``, a ``uint8`` array of ``N / 8`` entries or a bool / 0-1 array of
        ``N`` entries -- over the declared ``bits<N>`` attribute ``by`` (``Index.search_bits``): the ``top_k`` (<= 64) vectors
        with the smallest Hamming or Jaccard distance, as ``find_similar_many`` returns a hit (``score``: the distance)."""
        return self.find_similar_bits_many([query], top_k, namespace, by, metric=metric, where=where)[0]

    def find_similar_bits_many(self, queries, top_k: int, namespace: str = "default", by: str = "", metric: str = "hamming",
                               where=None) -> List[List[dict]]:
        """Batched ``find_similar_bits``: one code per query, one scan.  ``where`` is ``None`` or one dict filter."""
        if where is not None and not isinstance(where, Mapping):
            raise ValueError("find_similar_bits: where must be one dict filter (or None)")
        if not hasattr(self._index, "search_bits"):
            raise ValueError("find_similar_bits needs an index with search_bits")
        return self._enrich_many(self._index.search_bits(queries, top_k, namespace, by, metric=metric, where=where), namespace)

    def find_similar_hybrid(self, query, sparse_query, top_k: int, namespace: str = "default", metric: str = "cosine",
                            by: str = "", **options) -> List[dict]:
        """Additive: hybrid retrieval for one query -- a dense vector and a sparse one (a mapping ``{term: weight}`` or a
        pair ``(indices, values)``) over the declared ``sparse`` attribute ``by`` -- fused on the device
        (``Index.search_hybrid``, whose keywords ``fusion``, ``weights``, ``rrf_k``, ``fetch_k``, ``fetch_k_sparse`` and
        ``where`` pass through): the ``top_k`` (<= 64) vectors with the largest fused score, as ``find_similar_many``
        returns a hit (``score``: the fused score)."""
        values = getattr(query, "values", query)
        return self.find_similar_hybrid_many(np.asarray(values, dtype=np.float32)[None, :], [sparse_query], top_k, namespace,
                                             metric, by, **options)[0]

    def find_similar_hybrid_many(self, queries, sparse_queries, top_k: int, namespace: str = "default",
                                 metric: str = "cosine", by: str = "", *, fusion: str = "rrf", weights=(1.0, 1.0),
                                 rrf_k: float = 60.0, fetch_k: Optional[int] = None, fetch_k_sparse: Optional[int] = None,
                                 where=None) -> List[List[dict]]:
        """Batched ``find_similar_hybrid``: one dense and one sparse vector per query, one device call.  ``where`` is
        ``None`` or one dict filter; it restricts both legs."""
        if where is not None and not isinstance(where, Mapping):
            raise ValueError("find_similar_hybrid: where must be one dict filter (or None)")
        if not hasattr(self._index, "search_hybrid"):
            raise ValueError("find_similar_hybrid needs an index with search_hybrid")
        hits = self._index.search_hybrid(queries, sparse_queries, top_k, namespace, metric, by, fusion=fusion, weights=weights,
                                         rrf_k=rrf_k, fetch_k=fetch_k, fetch_k_sparse=fetch_k_sparse, where=where)
        return self._enrich_many(hits, namespace)

    def find_similar_scored(self, query, top_k: int, score, namespace: str = "default", metric: str = "cosine",
                            where=None) -> List[dict]:
        """Additive: "function score" search for one query (``Index.search_scored``): the ``top_k`` (<= 64) vectors with the
        smallest value of the formula ``score`` over the distance and the declared attributes (score.py), exact over all
        matching vectors, as ``find_similar_many`` returns a hit (``score``: the formula's value, lower is better).  Recipes:

            bonus               {"$sub": ["$distance", {"$mul": [0.2, {"$match": {"tier": "gold"}}]}]}
            popularity          {"$div": ["$distance", {"$add": [1, {"$attr": "likes", "$default": 0}]}]}
            linear age penalty  {"$add": ["$distance", {"$mul": [0.3, {"$min": [1, {"$div": [{"$abs": {"$sub": [
                                    {"$attr": "year"}, 2024]}}, 10]}]}]}]}
        """
        values = getattr(query, "values", query)
        return self.find_similar_scored_many(np.asarray(values, dtype=np.float32)[None, :], top_k, score, namespace, metric,
                                             where=where)[0]

    def find_similar_scored_many(self, queries, top_k: int, score, namespace: str = "default", metric: str = "cosine",
                                 where=None) -> List[List[dict]]:
        """Batched ``find_similar_scored``: one formula for all queries, one scan.  ``where`` is ``None`` or one dict filter
        (a predicate has no device form and is refused)."""
        if where is not None and not isinstance(where, Mapping):
            raise ValueError("find_similar_scored: where must be one dict filter (or None)")
        if not hasattr(self._index, "search_scored"):
            raise ValueError("find_similar_scored needs an index with search_scored")
        return self._enrich_many(self._index.search_scored(queries, top_k, namespace, metric, score, where=where), namespace)

    def recommend(self, positive, top_k: int, namespace: str = "default", metric: str = "cosine", negative=None,
                  where=None, exclude_examples: bool = True) -> List[dict]:
        """Additive: "recommend", best score, for one query (``Index.search_examples``): ``positive`` / ``negative`` are
        sequences of examples -- ids of stored vectors or vectors -- each judged on its own; hits as ``find_similar_many``
        returns them (``score``: the value inside the tier, a distance, lower is better) plus ``tier``."""
        return self.recommend_many([list(positive)], top_k, namespace, metric,
                                   negative=None if negative is None else [list(negative)], where=where,
                                   exclude_examples=exclude_examples)[0]

    def recommend_many(self, positive, top_k: int, namespace: str = "default", metric: str = "cosine", negative=None,
                       where=None, exclude_examples: bool = True) -> List[List[dict]]:
        """Batched ``recommend``: one sequence of examples per query, one chain of scans.  ``where`` is ``None`` or one dict
        filter (a predicate has no device form and is refused)."""
        self._examples_entry("recommend", "search_examples", where)
        hits = self._index.search_examples(positive, top_k, namespace, metric, negative=negative, where=where,
                                           exclude_examples=exclude_examples)
        return self._with_tiers(hits, namespace)

    def discover(self, top_k: int, namespace: str = "default", metric: str = "cosine", target=None, context=(),
                 where=None, exclude_examples: bool = True) -> List[dict]:
        """Additive: "discover" (with ``target``) / "context" (without) search for one query (``Index.search_discover``):
        ``context`` is a sequence of (positive, negative) pairs of examples; hits as ``recommend`` returns them."""
        return self.discover_many(top_k, namespace, metric, target=None if target is None else [target],
                                  context=[list(context)], where=where, exclude_examples=exclude_examples)[0]

    def discover_many(self, top_k: int, namespace: str = "default", metric: str = "cosine", target=None, context=(),
                      where=None, exclude_examples: bool = True) -> List[List[dict]]:
        """Batched ``discover``: one target (or none at all) and one sequence of pairs per query."""
        self._examples_entry("discover", "search_discover", where)
        hits = self._index.search_discover(top_k, namespace, metric, target=target, context=context, where=where,
                                           exclude_examples=exclude_examples)
        return self._with_tiers(hits, namespace)

    def _examples_entry(self, what: str, method: str, where) -> None:
        if where is not None and not isinstance(where, Mapping):
            raise ValueError(f"{what}: where must be one dict filter (or None)")
        if not hasattr(self._index, method):
            raise ValueError(f"{what} needs an index with {method}")

    def _with_tiers(self, hits, namespace: str) -> List[List[dict]]:
        """``_enrich_many`` plus each hit's ``tier``."""
        out = self._enrich_many(hits, namespace)
        by_id = [dict(zip(ids[:n].tolist(), tiers[:n].tolist()))
                 for ids, tiers, n in zip(hits.ids(), hits.tiers, hits.counts.tolist())]
        for rows, tier_of in zip(out, by_id):
            for row in rows:
                row["tier"] = tier_of[row["id"]]
        return out

    def _search_many(self, queries, top_k: int, namespace: str, metric: str, where):
        if where is None:
            return self._index.search_many(queries, top_k=top_k, namespace=namespace, metric=metric)
        if isinstance(where, Mapping):
            return self._index.search_many(queries, top_k=top_k, namespace=namespace, metric=metric, where=where)
        if isinstance(where, (list, tuple)):  # one dict filter (or None) per query: all on the device, one batched call
            if any(w is not None and not isinstance(w, Mapping) for w in where):
                raise ValueError("per-query where entries must be dict filters or None (per-query predicates have no host path)")
            return self._index.search_many(queries, top_k=top_k, namespace=namespace, metric=metric, where=list(where))
        allowed = [v.id for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata)]
        return self._index.search_many(queries, top_k=top_k, namespace=namespace, metric=metric, allowed_ids=allowed)

    def _enrich_many(self, per_query, namespace: str) -> List[List[dict]]:
        """``_enrich`` for a whole batch.  With an array-backed storage and this package's ``Index`` the 2,560 hits of a
        256-query wave are resolved by array operations -- id bytes -> storage rows by one sorted lookup, values by one
        gather (from the storage's matrix, or from the index's rows in HBM) -- and Python only builds the result
        dicts; any other storage / index goes hit list by hit list through ``_enrich``."""
        fast = getattr(self._storage, "read_rows_raw", None)
        if fast is None or not hasattr(per_query, "id_bytes"):
            return [self._enrich(hits, namespace) for hits in per_query]
        valid = per_query.valid()
        counts = valid.sum(axis=1).tolist()
        if not valid.any():
            return [[] for _ in counts]
        handles = per_query.handles()[valid] if hasattr(self._storage, "read_rows_at") else None
        if handles is not None and (handles >= 0).all():
            found, values, metas = self._storage.read_rows_at(handles, namespace)  # storage row numbers ride with the hits
        else:
            found, values, metas = fast(per_query.id_bytes()[valid], namespace)
        if values is None:
            values = self._index.fetch_values(namespace, per_query.labels[valid])
        ids = per_query.ids()[valid].tolist()
        scores = per_query.scores[valid].tolist()
        rows = list(values)  # one ndarray view per hit
        out, pos = [], 0
        if found.all():
            for n in counts:
                out.append([{"id": ids[j], "values": rows[j], "metadata": metas[j], "score": scores[j]}
                            for j in range(pos, pos + n)])
                pos += n
        else:
            ok = found.tolist()
            for n in counts:
                out.append([{"id": ids[j], "values": rows[j], "metadata": metas[j], "score": scores[j]}
                            for j in range(pos, pos + n) if ok[j]])
                pos += n
        return out

    def find_similar_stream(self, batches, top_k: int, namespace: str = "default", metric: str = "cosine"):
        """Additive: ``find_similar_many`` over an iterable of query batches, pipelined -- while the GPU scans batch
        i+1 (a worker thread inside the ctypes call, which holds no GIL) this thread enriches batch i.  Yields one
        ``List[List[dict]]`` per batch, in order."""
        stream = getattr(self._index, "search_stream", None)
        if stream is not None:  # this package's Index: one engine -> a prefetching worker; row shards -> scan / merge pipeline
            for hits in stream(batches, top_k, namespace, metric):
                yield self._enrich_many(hits, namespace)
            return
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=1) as pool:
            pending = None
            for q in batches:
                nxt = pool.submit(self._search_many, q, top_k, namespace, metric, None)
                if pending is not None:
                    yield self._enrich_many(pending.result(), namespace)
                pending = nxt
            if pending is not None:
                yield self._enrich_many(pending.result(), namespace)

    def find_similar_where(self, query: VectorDTO, top_k: int, where, namespace: str = "default",
                           metric: str = "cosine") -> List[dict]:
        """``find_similar`` restricted to the vectors whose metadata satisfies ``where``."""
        values = np.asarray(query.values, dtype=np.float32)
        if values.ndim != 1:
            return []
        return self.find_similar_many(values[None, :], top_k, namespace, metric, where=where)[0]

    def find_in_radius(self, query: VectorDTO, radius: float, namespace: str = "default",
                       metric: str = "cosine", max_results: int = 1024, where=None) -> List[dict]:
        """Range query (no reference counterpart; README.md:30-41 intent only).  ``where`` as in ``find_similar_many``: a
        dict filter is evaluated on the device; a predicate filters the hits (all of them, up to the index's 16384 per
        query) by their stored metadata before ``max_results`` applies."""
        if where is None or isinstance(where, Mapping):
            kw = {} if where is None else {"where": where}
            hits = self._index.range_search(query, radius, namespace=namespace, metric=metric, max_results=max_results, **kw)
            out = self._enrich(hits, namespace)
        else:
            hits = self._index.range_search(query, radius, namespace=namespace, metric=metric, max_results=None)
            out = [h for h in self._enrich(hits, namespace) if where(h["metadata"])]
            out = out if max_results is None else out[:max(1, int(max_results))]
        return self._fill_values(out, namespace)

    def _fill_values(self, out: List[dict], namespace: str) -> List[dict]:
        missing = [i for i, h in enumerate(out) if h["values"] is None]  # array storage that keeps the rows in HBM only
        if missing and hasattr(self._index, "fetch_values_by_id"):
            rows = self._index.fetch_values_by_id(namespace, [out[i]["id"] for i in missing])
            for i, r in zip(missing, rows):
                out[i]["values"] = r
        return out

    def find_in_radius_many(self, queries, radius: float, namespace: str = "default", metric: str = "cosine",
                            max_results: int = 1024, where=None) -> List[List[dict]]:
        """Batched ``find_in_radius``: ``queries`` is an [nq, dim] array or a sequence of VectorDTO, one ``radius`` for all.
        ``where`` as in ``find_similar_many``: a dict filter, or a list of ``nq`` entries, each a dict filter or ``None`` --
        every query its own filter, all evaluated on the device in one batched call (``Index.range_search_many``); a
        predicate filters every query's hits by their stored metadata, and inside the list it is a ``ValueError``."""
        if isinstance(where, (list, tuple)):
            if any(w is not None and not isinstance(w, Mapping) for w in where):
                raise ValueError("per-query where entries must be dict filters or None (per-query predicates have no host path)")
            where = list(where)
        if where is None or isinstance(where, (Mapping, list)):
            kw = {} if where is None else {"where": where}
            per_query = self._index.range_search_many(queries, radius, namespace=namespace, metric=metric,
                                                      max_results=max_results, **kw)
            out = [self._enrich(hits, namespace) for hits in per_query]
        else:
            per_query = self._index.range_search_many(queries, radius, namespace=namespace, metric=metric, max_results=None)
            out = [[h for h in self._enrich(hits, namespace) if where(h["metadata"])] for hits in per_query]
            if max_results is not None:
                out = [hits[:max(1, int(max_results))] for hits in out]
        return [self._fill_values(hits, namespace) for hits in out]

    # ---- additive: similarity join (Index.join_within / duplicate_groups)
    def _stored(self, ids, namespace: str) -> dict:
        """id -> {"id", "values", "metadata"} of the stored vectors among ``ids`` (values from the index where the storage
        keeps none)."""
        ids = list(dict.fromkeys(ids))
        rows = [{"id": v.id, "values": v.values, "metadata": v.metadata} for v in self._storage.read_vectors(ids, namespace) if v]
        return {r["id"]: r for r in self._fill_values(rows, namespace)}

    def _join_pairs(self, what: str, radius: float, namespace: str, metric: str, where, max_per_row: int, order: str = "left"):
        """The self-join's pairs for ``where`` = None, a dict filter (on the device) or a predicate (the host path: the
        matching stored vectors are the left rows of a by-ids join, whose pairs are kept when the partner matches too and
        was inserted later)."""
        if where is None or isinstance(where, Mapping):
            return self._index.join_within(namespace, metric, radius, where=where, max_per_row=max_per_row, order=order)
        if not callable(where):
            raise ValueError(f"{what}: where must be a dict filter, a predicate or None (got {type(where).__name__})")
        allowed = [v.id for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata)]
        hits = self._index.join_within(namespace, metric, radius, ids=allowed, max_per_row=max_per_row, order=order)
        inside = set(allowed)
        keep = np.array([r in inside for r in hits.right_ids.tolist()], dtype=bool) & (hits.right_labels > hits.left_labels)
        for name in ("left_ids", "right_ids", "scores", "left_labels", "right_labels", "distances"):
            setattr(hits, name, getattr(hits, name)[keep])
        return hits

    def find_near_pairs(self, radius: float, namespace: str = "default", metric: str = "cosine", where=None,
                        max_per_row: int = 1024, order: str = "left") -> dict:
        """Additive: every unordered pair of stored vectors within ``radius`` of each other (``Index.join_within``, the
        self-join), enriched like ``find_in_radius``: {"pairs": [{"left": {id, values, metadata}, "right": {...}, "score"},
        ...], "complete": no vector had more than ``max_per_row`` partners}.  The earlier-inserted vector is on the left.
        ``where``: a dict filter is evaluated on the device; a predicate picks the vectors by their stored metadata."""
        hits = self._join_pairs("find_near_pairs", radius, namespace, metric, where, max_per_row, order)
        stored = self._stored(hits.left_ids.tolist() + hits.right_ids.tolist(), namespace)
        pairs = [{"left": stored[a], "right": stored[b], "score": s} for a, b, s in hits.pairs() if a in stored and b in stored]
        return {"pairs": pairs, "complete": hits.complete}

    def find_duplicates(self, radius: float, namespace: str = "default", metric: str = "cosine", where=None,
                        max_per_row: int = 1024) -> List[List[dict]]:
        """Additive: the groups of near-duplicates (``Index.duplicate_groups``: the connected components of the pairs within
        ``radius``), every member enriched with values and metadata; groups and members in insertion order.  Raises
        ``engine.JoinOverflow`` when a vector has more than ``max_per_row`` partners.  ``where`` as in ``find_near_pairs``."""
        if where is None or isinstance(where, Mapping):
            groups = self._index.duplicate_groups(namespace, metric, radius, where=where, max_per_row=max_per_row)
        else:
            from .engine import JoinOverflow
            from .join import connected_groups

            hits = self._join_pairs("find_duplicates", radius, namespace, metric, where, max_per_row)
            if not hits.complete:
                raise JoinOverflow(int(max_per_row), int(hits.counts.max()))
            id_of = dict(zip(hits.left_labels.tolist(), hits.left_ids.tolist()))
            id_of.update(zip(hits.right_labels.tolist(), hits.right_ids.tolist()))
            groups = [[id_of[x] for x in g] for g in connected_groups(hits.left_labels, hits.right_labels)]
        stored = self._stored([u for g in groups for u in g], namespace)
        return [[stored[u] for u in g if u in stored] for g in groups]

    # ---- additive: clustering (Index.cluster / Index.assign_clusters)
    def cluster_vectors(self, k: int, namespace: str = "default", metric: str = "cosine", where=None, init="random",
                        seed: int = 0, max_iterations: int = 25, assign_to: Optional[str] = None):
        """Additive: k-means over the stored vectors of ``namespace`` (``Index.cluster``: on the device, from the rows in
        HBM).  With ``assign_to`` (a declared ``int`` attribute) every clustered vector's id goes into the index's column
        AND into the stored metadata under that key, as ``update_where`` keeps the two in step.  Returns the
        ``ClusterResult``."""
        return self._clustered("cluster_vectors", "cluster", namespace, where, assign_to,
                               lambda: self._index.cluster(namespace, metric, k, where=where, init=init, seed=seed,
                                                           max_iterations=max_iterations, assign_to=assign_to))

    def assign_clusters(self, centroids, namespace: str = "default", metric: str = "cosine", assign_to: Optional[str] = None,
                        where=None):
        """Additive: every stored vector matching ``where`` to the nearest of ``centroids`` (``Index.assign_clusters``), the
        cluster ids into ``assign_to`` in the index and in the stored metadata.  Returns (sizes, costs)."""
        return self._clustered("assign_clusters", "assign_clusters", namespace, where, assign_to,
                               lambda: self._index.assign_clusters(namespace, metric, centroids, assign_to=assign_to, where=where))

    def _clustered(self, what: str, method: str, namespace: str, where, assign_to, call):
        if where is not None and not isinstance(where, Mapping):
            raise ValueError(f"{what}: where must be one dict filter (or None)")
        if not hasattr(self._index, method):
            raise ValueError(f"{what} needs an index with {method}")
        if assign_to is None:
            return call()
        if assign_to not in (getattr(self._index, "attributes", None) or {}):
            return call()  # (the index refuses it, in its own words)
        # the candidates are the filter's matches BEFORE the call: it may read assign_to itself
        ids = self._index.query_by_metadata(namespace, where if where is not None else {})
        result = call()
        values = self._index._int_attribute_of(namespace, assign_to, ids)
        for vid, value in zip(ids, values):
            self._storage.update_metadata(vid, {assign_to: value}, namespace)
        return result

    # ---- additive: metadata queries (README.md:252,274: StorageEngine.query_by_metadata; no reference code)
    def count_where(self, where, namespace: str = "default") -> int:
        """Live vectors of ``namespace`` matching ``where`` (dict filter: counted on the device; predicate: over storage)."""
        if isinstance(where, Mapping):
            return self._index.count(namespace, where)
        return sum(1 for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata))

    def query_by_metadata(self, where, namespace: str = "default", *, order_by=None, descending: bool = False, limit=None,
                          offset: int = 0) -> List[UUID]:
        """Ids of the vectors of ``namespace`` matching ``where``, in insertion order; with ``order_by`` (and a ``limit``):
        ``top_by(order_by, limit, where, ...)["ids"]``."""
        if order_by is not None or descending is not False or limit is not None or offset != 0 or isinstance(offset, bool):
            self._index.check_order_keywords(order_by, descending, limit, offset)
            return self.top_by(order_by, limit, where, namespace, descending=descending, offset=offset)["ids"]
        if isinstance(where, Mapping):
            return self._index.query_by_metadata(namespace, where)
        return [v.id for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata)]

    # ---- additive: ordered metadata queries (Index.top_by; no reference code)
    def top_by(self, by: str, limit: int, where=None, namespace: str = "default", *, descending: bool = False,
               offset: int = 0):
        """``Index.top_by`` of ``namespace``: a dict filter (or no filter) is ranked on the device; a predicate is ranked over
        the storage's metadata on the host, as ``facets`` does -- the values ``Index.extract_attributes`` would store, rows
        of equal value in insertion order -- with the same answer format."""
        if where is None or isinstance(where, Mapping):
            return self._index.top_by(namespace, by, limit, where, descending=descending, offset=offset)
        if not callable(where):
            raise ValueError(f"top_by: where must be a dict filter, a predicate or None (got {type(where).__name__})")
        kind = self._index.check_top_by_args(by, limit, descending, offset)
        picked = [v for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata)]
        values = self._index.extract_attributes([v.metadata for v in picked])[by]
        if kind == "float":  # the column stores doubles: an int literal ranks as its double
            values = [None if x is None else float(x) for x in values]
        ranked = [(x, i) for i, x in enumerate(values) if x is not None and x == x]
        # a stable sort keeps insertion order among equal values (-0.0 == 0.0), and reverse=True keeps it too
        ranked.sort(key=lambda p: p[0], reverse=bool(descending))
        window = ranked[int(offset):int(offset) + int(limit)]
        return {"ids": [picked[i].id for _, i in window],
                "values": self._index.decode_order_values(kind, [x for x, _ in window]),
                "matched": len(picked), "absent": len(picked) - len(ranked)}

    # ---- additive: nearest by distance on a geo attribute (Index.nearest; no reference code)
    def find_nearby(self, point, limit: int, namespace: str, by: str, where=None, offset: int = 0) -> List[dict]:
        """The stored vectors of ``namespace`` nearest to ``point`` -- ``(lat, lon)`` or ``{"lat": .., "lon": ..}`` -- by the
        declared geo attribute ``by``, ranked on the device (``Index.nearest``; ``where``: a dict filter or ``None``, a
        maximum distance is a ``$geo_radius`` in it): ``[{"id", "values", "metadata", "distance": metres, "point": (lat,
        lon) as the index holds it}, ...]``, nearest first."""
        if where is not None and not isinstance(where, Mapping):
            raise ValueError(f"find_nearby: where must be a dict filter or None (got {type(where).__name__})")
        got = self._index.nearest(namespace, by, point, limit, where, offset=offset)
        stored = {v.id: v for v in self._storage.read_vectors(got["ids"], namespace) if v}
        out = []
        for vid, p, d in zip(got["ids"], got["points"], got["distances"]):
            v = stored.get(vid)
            if v:
                out.append({"id": v.id, "values": v.values, "metadata": v.metadata, "distance": d, "point": p})
        return self._fill_values(out, namespace)

    # ---- additive: facet counts and histograms (Index.facets / Index.histogram; no reference code)
    def _host_column(self, by: str, where, namespace: str):
        """(values of attribute ``by`` of the stored vectors ``where`` accepts -- ``None`` / NaN = absent --, their number)."""
        kind = self._index.attributes[by]
        picked = [None if v.metadata is None else v.metadata.get(by)
                  for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata)]
        present = [x for x in picked if x is not None and not (kind == "float" and isinstance(x, float) and x != x)]
        if kind.endswith("[]"):  # a list attribute: a row counts once under each element; an empty list contributes nothing
            present = [set(x) for x in present if len(x)]
        return present, len(picked)

    def facets(self, by, where=None, namespace: str = "default", *, limit=None, order: str = "count",
               max_values: int = 65536):
        """``Index.facets`` of ``namespace``: a dict filter (or no filter) is aggregated on the device; a predicate is
        computed over the storage's metadata on the host, as ``count_where`` does, with the same answer format."""
        if where is None or isinstance(where, Mapping):
            return self._index.facets(namespace, by, where, limit=limit, order=order, max_values=max_values)
        if not callable(where):
            raise ValueError(f"facets: where must be a dict filter, a predicate or None (got {type(where).__name__})")
        names = self._index.check_facet_args(by, order, limit, max_values)
        out = {}
        for name in names:
            present, matched = self._host_column(name, where, namespace)
            counts: Dict[Any, int] = {}
            listed = self._index.attributes[name].endswith("[]")
            for x in (present if not listed else [e for row in present for e in row]):
                counts[x] = counts.get(x, 0) + 1
            if self._index.attributes[name] == "int" and len(counts) > max_values:
                raise ValueError(f"facets: attribute {name!r} holds more than max_values={max_values} distinct values")
            out[name] = {"values": self._index.order_facets(list(counts.items()), order, limit), "matched": matched,
                         "absent": matched - len(present)}
        return out if isinstance(by, (list, tuple)) else out[names[0]]

    def histogram(self, by: str, edges, where=None, namespace: str = "default"):
        """``Index.histogram`` of ``namespace``; ``where`` as in ``facets``."""
        if where is None or isinstance(where, Mapping):
            return self._index.histogram(namespace, by, edges, where)
        if not callable(where):
            raise ValueError(f"histogram: where must be a dict filter, a predicate or None (got {type(where).__name__})")
        e = self._index.check_histogram_args(by, edges)
        present, matched = self._host_column(by, where, namespace)
        bins = np.searchsorted(e, np.asarray(present, dtype=e.dtype), side="right")
        return {"counts": np.bincount(bins, minlength=e.size + 1).astype(np.int64), "matched": matched,
                "absent": matched - len(present)}

    # ---- additive: attribute statistics (Index.stats; no reference code)
    def stats(self, attr, where=None, namespace: str = "default", by: Optional[str] = None, max_groups: int = 65536):
        """``Index.stats`` of ``namespace``: a dict filter (or no filter) is aggregated on the device; a predicate is
        computed over the storage's metadata on the host, as ``facets`` does, by the same rules -- exact integer sums, the
        fixed-point sum of floats (stats.py) -- so both paths return equal values."""
        if where is None or isinstance(where, Mapping):
            return self._index.stats(namespace, attr, where, by=by, max_groups=max_groups)
        if not callable(where):
            raise ValueError(f"stats: where must be a dict filter, a predicate or None (got {type(where).__name__})")
        names = self._index.check_stats_args(attr, by, max_groups)
        kinds = self._index.attributes
        picked = [v.metadata or {} for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata)]
        out = {}
        for name in names:
            kind = kinds[name]
            members: Dict[Any, list] = {} if by is not None else {None: []}
            by_absent = 0
            for m in picked:
                g = None if by is None else m.get(by)
                if by is not None and g is None:
                    by_absent += 1
                    continue
                x = m.get(name)
                members.setdefault(g, []).append(None if x is None else float(x) if kind == "float" else int(x))
            if by is not None and kinds[by] == "int" and len(members) > max_groups:
                raise ValueError(f"stats: by={by!r} holds more than max_groups={max_groups} distinct values")
            groups = []
            for xs in members.values():
                present = [x for x in xs if x is not None and x == x]
                if kind == "float":
                    groups.append((len(xs),) + _stats.float_group(present))
                else:
                    groups.append((len(xs), len(present), min(present, default=None), max(present, default=None), sum(present)))
            out[name] = self._index.shape_stats(kind, by, list(members), groups, len(picked), by_absent)
        return out if isinstance(attr, (list, tuple)) else out[names[0]]

    # ---- delete -> lazy rebuild (query_processor.py:51-62)
    def delete(self, ids: Sequence[UUID], namespace: str = "default") -> Sequence[UUID]:
        removed = [vid for vid in ids if self._storage.delete(vid, namespace)]
        self._index.remove(ids, namespace)
        self._rebuild_if_required(namespace)
        return removed

    def _rebuild_if_required(self, namespace: str) -> None:
        probe = getattr(self._index, "is_rebuild_required", None)
        if probe and probe(namespace):
            compact = getattr(self._index, "compact", None)
            if compact and self._rebuild_scope != "namespace" and compact(namespace):
                return  # same end state as the rebuild below, computed on the device
            full = self._storage.namespace_map
            if self._rebuild_scope == "namespace":
                source = {namespace: full.get(namespace, [])}
            else:
                source = dict(full)
                source.setdefault(namespace, [])
            self._index.rebuild(self._with_values(source), metric=self._index._space)

    # ---- additive: metadata updates and deletes by filter (Index.update_attributes / update_where / remove_where)
    def _declared(self, patch: Mapping) -> dict:
        declared = getattr(self._index, "attributes", None) or {}
        return {k: v for k, v in patch.items() if k in declared}

    def update_metadata(self, ids: Sequence[UUID], metadata, namespace: str = "default") -> List[UUID]:
        """Overlay the stored metadata of ``ids`` with ``metadata`` -- one mapping for every id, or a sequence with one per
        id; ``None`` deletes a key -- and set the index's declared attributes among its keys in place
        (``Index.update_attributes``): no new id, no re-sent vector.  The index's refusals come before anything is written.
        Returns the ids the storage holds."""
        ids = list(ids)
        patches = [metadata] * len(ids) if isinstance(metadata, Mapping) else list(metadata)
        if len(patches) != len(ids) or not all(isinstance(p, Mapping) for p in patches):
            raise ValueError(f"update_metadata: one mapping, or one mapping per id ({len(ids)} ids)")
        declared = [self._declared(p) for p in patches]
        indexed = any(declared) and hasattr(self._index, "update_attributes")
        if indexed:
            self._index.validate_attribute_update(len(ids), declared, namespace)
        updated = [vid for vid, p in zip(ids, patches) if self._storage.update_metadata(vid, p, namespace)]
        if indexed:
            self._index.update_attributes(ids, declared, namespace)
        return updated

    @staticmethod
    def _increment(value) -> bool:
        return isinstance(value, Mapping) and list(value) == ["$inc"]

    def _row_patch(self, stored: Mapping, metadata: Mapping) -> dict:
        """``metadata`` for one stored row: every ``{"$inc": x}`` becomes the row's new value, or is left out when the row
        holds no value to add to."""
        out = {}
        for key, value in metadata.items():
            if not self._increment(value):
                out[key] = value
                continue
            old = None if stored is None else stored.get(key)
            if old is not None:
                out[key] = old + value["$inc"]
        return out

    def update_where(self, where, metadata: Mapping, namespace: str = "default") -> int:
        """``update_metadata`` of every vector matching ``where``; a value may be ``{"$inc": x}``, which adds to the rows
        that hold a value and skips the others.  A dict filter updates the declared attributes in one pass on the device
        (``Index.update_where``, all or nothing: an increment that would overflow raises before anything is written); a
        predicate is evaluated over the storage and goes through ``update_metadata``.  Returns the matched count."""
        if not isinstance(metadata, Mapping) or not metadata:
            raise ValueError("update_where: metadata must be a non-empty mapping")
        if not isinstance(where, Mapping):
            if not callable(where):
                raise ValueError(f"update_where: where must be a dict filter or a predicate (got {type(where).__name__})")
            rows = [v for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata)]
            self.update_metadata([v.id for v in rows], [self._row_patch(v.metadata, metadata) for v in rows], namespace)
            return len(rows)
        declared = self._declared(metadata)
        if declared:
            self._index.stage_assignments(namespace, declared)  # the refusals, before anything is resolved or written
        ids = self._index.query_by_metadata(namespace, where)
        if declared:  # first: the only step that can still refuse (an overflowing increment), and then nothing has changed
            self._index.update_where(namespace, where, declared)
        stored = self._storage.read_vectors(ids, namespace)
        for vid, row in zip(ids, stored):
            if row is not None:
                self._storage.update_metadata(vid, self._row_patch(row.metadata, metadata), namespace)
        return len(ids)

    def delete_where(self, where, namespace: str = "default") -> List[UUID]:
        """``delete`` of every vector matching ``where``: a dict filter is tombstoned on the device
        (``Index.remove_where``), a predicate is evaluated over the storage.  Returns the ids removed from the storage."""
        if not isinstance(where, Mapping):
            if not callable(where):
                raise ValueError(f"delete_where: where must be a dict filter or a predicate (got {type(where).__name__})")
            return list(self.delete([v.id for v in self._storage.namespace_map.get(namespace, []) if where(v.metadata)],
                                    namespace))
        ids = self._index.remove_where(namespace, where, return_ids=True)
        removed = [vid for vid in ids if self._storage.delete(vid, namespace)]
        self._rebuild_if_required(namespace)
        return removed

    def _with_values(self, source):
        """Rebuild sources whose rows keep their values in HBM only (``upsert_arrays(keep_host_copy=False)``): the
        values are read back from the index BEFORE ``rebuild`` closes the engines that hold the only copy."""
        fetch = getattr(self._index, "fetch_values_by_id", None)
        out = {}
        for name, rows in source.items():
            rows = list(rows)
            missing = [i for i, v in enumerate(rows) if getattr(v, "values", None) is None]
            if missing:
                if fetch is None:
                    raise RuntimeError(f"namespace {name!r}: stored rows carry no values and the index cannot supply them")
                from .storage import StoredRow

                vals = fetch(name, [rows[i].id for i in missing])
                for i, val in zip(missing, vals):
                    rows[i] = StoredRow(rows[i].id, val, rows[i].metadata)
            out[name] = rows
        return out

    # ---- introspection (query_processor.py:64-82)
    def list_namespaces(self) -> List[str]:
        return self._storage.list_namespaces

    def get_namespace_vectors(self, namespace: str) -> List[Dict[str, Any]]:
        return [{"id": v.id, "values": v.values, "metadata": v.metadata}
                for v in self._storage.namespace_map.get(namespace, [])]

    def get_namespace_count(self, namespace: str) -> int:
        return len(self._storage.namespace_map.get(namespace, []))

    def get_storage_info(self) -> Dict[str, Any]:
        """Passthrough the REST layer relies on (query_processor.py:81-82; rest_api.py:283)."""
        return self._storage.get_storage_info()

    # ---- additive: bulk ingest without one Python object per row (ArrayStorage + Index.add_arrays)
    def upsert_arrays(self, values: np.ndarray, namespace: str = "default", metadata=None, *,
                      keep_host_copy: bool = True) -> np.ndarray:
        """``upsert_many`` for an ``[n, dim]`` matrix: mints ids, hands the rows to the index and (ids, metadata and --
        unless ``keep_host_copy=False`` -- the values) to the storage.  Returns the ``[n, 16] uint8`` id table."""
        if not hasattr(self._storage, "write_arrays") or not hasattr(self._index, "add_arrays"):
            raise RuntimeError("upsert_arrays needs an array-backed storage (ArrayStorage) and this package's Index")
        from .idtable import mint_uuid4_bytes

        values = np.ascontiguousarray(values, dtype=np.float32)
        if values.ndim != 2:
            raise RuntimeError(f"Wrong dimensionality of the vectors: expected a matrix, got shape {values.shape}")
        if not keep_host_copy and self._rebuild_scope == "namespace":
            # Q4's rebuild drops every other namespace from the index; with the values in HBM only that would be data loss
            raise ValueError('keep_host_copy=False needs rebuild_scope="all": a namespace-scoped rebuild closes the other '
                             "namespaces' engines, which would hold the only copy of their rows")
        # the index's refusals (dimension, non-finite rows) come before the storage is written: no ghost rows
        # declared attributes (Index(attributes=...)) come out of the metadata and are refused here too when mistyped
        attrs = None
        if metadata is not None and getattr(self._index, "attributes", None):
            if len(metadata) != values.shape[0]:
                raise ValueError(f"{len(metadata)} metadata entries for {values.shape[0]} rows")
            attrs = self._index.extract_attributes(metadata)
        if hasattr(self._index, "validate_arrays"):
            if attrs is None:
                self._index.validate_arrays(values, namespace)
            else:
                self._index.validate_arrays(values, namespace, attributes=attrs)
        ids = mint_uuid4_bytes(values.shape[0])
        first = self._storage.write_arrays(ids, namespace, values if keep_host_copy else None, metadata)
        kw = {} if attrs is None else {"attributes": attrs}
        self._index.add_arrays(values, namespace, ids=ids,
                               handles=np.arange(first, first + values.shape[0], dtype=np.int64), **kw)
        return ids
