"""The refusals and the empty answers of every ``Index`` entry family, without a GPU: one table of calls, each with the
exception type and the full message it raises, over one small index whose schema holds an attribute of every kind.  The
double-fault rows pin which refusal wins when a call has two faults; the lacking-engine rows pin the "needs an engine with"
sentence of every family; the empty rows pin the type and the shapes of an answer that needs no search."""
import re
from uuid import uuid4

import numpy as np
import pytest

from mlvectordb_amd import Index, Vector
from mlvectordb_amd.index import BatchHits, GroupedBatchHits, HybridBatchHits, LateBatchHits
from tests import geo_helpers
from tests.grouped_helpers import GroupedOracleEngine
from tests.hybrid_helpers import HybridOracleEngine
from tests.like_helpers import LikeOracleEngine
from tests.maxsim_helpers import MaxSimOracleEngine
from tests.mmr_helpers import MmrOracleEngine
from tests.order_helpers import OrderOracleEngine
from tests.stats_helpers import StatsOracleEngine
from tests.where_helpers import EachOracleEngine, EachRangeOracleEngine

SCHEMA = {"year": "int", "price": "float", "genre": "str", "in_stock": "bool", "nums": "int[]", "tags": "str[]",
          "terms": "sparse", "loc": "geo"}
DECLARED = f"(declared: {sorted(SCHEMA)})"
SHARDED = "is not supported on a row-sharded index (devices=[...] with more than one entry)"
SCALAR = {"terms": "is a sparse column; it needs a scalar attribute (a sparse vector is searched with search_sparse)",
          "loc": "is a geo column; it needs a scalar attribute (a location is filtered with $geo_radius / $geo_box and "
                 "ranked with nearest)",
          "nums": "is a int[] column; it needs a scalar attribute (a list has no one value to rank, bin or group by)",
          "tags": "is a str[] column; it needs a scalar attribute (a list has no one value to rank, bin or group by)"}
N, DIM = 6, 4
Q = np.eye(2, DIM, dtype=np.float32)
SQ = [{1: 1.0}, {2: 0.5}]
TOKENS = [np.ones((2, DIM), np.float32), np.ones((3, DIM), np.float32)]


class FullEngine(HybridOracleEngine, StatsOracleEngine, OrderOracleEngine, GroupedOracleEngine, MmrOracleEngine,
                 LikeOracleEngine, MaxSimOracleEngine, EachOracleEngine, EachRangeOracleEngine,
                 geo_helpers.oracle_engine_class()):
    """Every family's entry in one host engine."""


class Lacking(FullEngine):
    """``FullEngine`` without the methods named in ``lacking``: what a namespace that is not single-device looks like."""

    lacking = frozenset()

    def __getattribute__(self, name):
        if name in type(self).lacking:
            raise AttributeError(name)
        return super().__getattribute__(name)


def _filled(factory=FullEngine, **kw):
    index = Index(space="l2", engine_factory=factory, attributes=SCHEMA, **kw)
    rng = np.random.default_rng(3)
    vecs = [Vector(values=rng.standard_normal(DIM).astype(np.float32),
                   metadata={"year": 2000 + i, "price": 1.5 * i, "genre": "ab"[i % 2], "in_stock": bool(i % 2), "nums": [i, 7],
                             "tags": ["x", "yz"[i % 2]], "terms": {i: 1.0, 9: 0.5}, "loc": (10.0 + i, 20.0)})
            for i in range(N)]
    index.add(vecs, "ns")
    return index, vecs


@pytest.fixture(scope="module")
def filled():
    return _filled()


@pytest.fixture(scope="module")
def index(filled):
    return filled[0]


@pytest.fixture(scope="module")
def sharded():  # (a row-sharded index declares no attributes: the constructor refuses them)
    return Index(space="l2", engine_factory=FullEngine, devices=[0, 1])


def test_the_constructor_refuses_attributes_on_a_row_sharded_index():
    with pytest.raises(ValueError, match=re.escape(f"attributes= {SHARDED}")):
        Index(space="l2", engine_factory=FullEngine, devices=[0, 1], attributes=SCHEMA)


def _undeclared(what, name="nope"):
    return f"{what}: {name!r} is not a declared attribute of this index {DECLARED}"


ONE_FILTER = "where must be one dict filter or None (got list)"
COMPILE = "where must be a dict filter (where.py), got int"
EACH = "per-query where entries must be dict filters or None (where.py), got int"

# (id, call on the filled index, exception, full message)
REFUSALS = [
    # -- search_many
    ("many-group_size-alone", lambda ix: ix.search_many(Q, 3, "ns", "l2", group_size=2), ValueError,
     "search_many: group_size is the member count of distinct=, give both or neither"),
    ("many-fetch_k-alone", lambda ix: ix.search_many(Q, 3, "ns", "l2", fetch_k=8), ValueError,
     "search_many: fetch_k is the candidate count of mmr_lambda=, give both or neither"),
    ("many-where-and-ids", lambda ix: ix.search_many(Q, 3, "ns", "l2", allowed_ids=[uuid4()], where={"year": 2000}), ValueError,
     "search_many: give allowed_ids or where, not both"),
    ("many-where-type", lambda ix: ix.search_many(Q, 3, "ns", "l2", where=5), ValueError, COMPILE),
    ("many-each-count", lambda ix: ix.search_many(Q, 3, "ns", "l2", where=[None]), ValueError,
     "search_many: 1 per-query filters for 2 queries"),
    ("many-each-type", lambda ix: ix.search_many(Q, 3, "ns", "l2", where=[None, 5]), ValueError, EACH),
    # -- distinct / group_size
    ("distinct-group_size", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="year", group_size=0), ValueError,
     "group_size must be an int in [1, 64] (got 0)"),
    ("distinct-group_size-bool", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="year", group_size=True), ValueError,
     "group_size must be an int in [1, 64] (got True)"),
    ("distinct-undeclared", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="nope"), ValueError, _undeclared("distinct")),
    ("distinct-unstring", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct=5), ValueError, _undeclared("distinct", 5)),
    ("distinct-sparse", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="terms"), ValueError,
     f"distinct: attribute 'terms' {SCALAR['terms']}"),
    ("distinct-geo", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="loc"), ValueError,
     f"distinct: attribute 'loc' {SCALAR['loc']}"),
    ("distinct-list", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="tags"), ValueError,
     f"distinct: attribute 'tags' {SCALAR['tags']}"),
    ("distinct-float", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="price"), ValueError,
     "distinct: attribute 'price' is a float column; groups need an int, str or bool attribute"),
    ("distinct-top_k", lambda ix: ix.search_many(Q, 65, "ns", "l2", distinct="year"), ValueError,
     "distinct: top_k must be <= 64 (got 65)"),
    ("distinct-where-list", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="year", where=[None, None]), ValueError,
     "distinct: a per-query where list is not supported, give one dict filter"),
    ("distinct-ids", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="year", allowed_ids=[uuid4()]), ValueError,
     "distinct: allowed_ids is not supported, give a dict where filter"),
    ("distinct-where-type", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="year", where=5), ValueError, COMPILE),
    # -- mmr
    ("mmr-distinct", lambda ix: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=0.5, distinct="year"), ValueError,
     "mmr_lambda: distinct= cannot be combined with it, give one of the two"),
    ("mmr-lambda", lambda ix: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=1.5), ValueError,
     "mmr_lambda must lie in [0, 1] (got 1.5)"),
    ("mmr-top_k", lambda ix: ix.search_many(Q, 65, "ns", "l2", mmr_lambda=0.5), ValueError,
     "mmr_lambda: top_k must be <= 64 (got 65)"),
    ("mmr-fetch_k-high", lambda ix: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=0.5, fetch_k=1025), ValueError,
     "mmr_lambda: fetch_k must be <= 1024 (got 1025)"),
    ("mmr-fetch_k-low", lambda ix: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=0.5, fetch_k=2), ValueError,
     "mmr_lambda: fetch_k must be >= top_k (got fetch_k=2, top_k=3)"),
    ("mmr-where-list", lambda ix: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=0.5, where=[None, None]), ValueError,
     "mmr_lambda: a per-query where list is not supported, give one dict filter"),
    ("mmr-ids", lambda ix: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=0.5, allowed_ids=[uuid4()]), ValueError,
     "mmr_lambda: allowed_ids is not supported, give a dict where filter"),
    ("mmr-where-type", lambda ix: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=0.5, where=5), ValueError, COMPILE),
    # -- like
    ("like-where-list", lambda ix: ix.search_like([uuid4()], 3, "ns", "l2", where=[None]), ValueError,
     "search_like: a per-query where list is not supported, give one dict filter"),
    ("like-weights-negative", lambda ix: ix.search_like([uuid4()], 3, "ns", "l2", weights=[1.0], negative=[uuid4()]), ValueError,
     "search_like: weights= gives every example its own number and cannot be combined with negative="),
    ("like-positive", lambda ix: ix.search_like(5, 3, "ns", "l2"), ValueError,
     "search_like: positive must be a sequence with one sequence per query (or one flat sequence)"),
    ("like-top_k", lambda ix: ix.search_like([uuid4()], 1024, "ns", "l2"), ValueError,
     "search_like: top_k + examples must be <= 1024 (got 1024 + 1)"),
    ("like-where-type", lambda ix: ix.search_like([uuid4()], 3, "ns", "l2", where=5), ValueError, COMPILE),
    ("like-base-count", lambda ix: ix.search_like([uuid4()], 3, "ns", "l2", queries=Q), ValueError,
     "search_like: 1 positive entries, 2 queries"),
    # -- late interaction
    ("late-euclidean", lambda ix: ix.search_late(TOKENS, 3, "ns", "euclidean", "year"), ValueError,
     'search_late: metric "euclidean" is not supported (a root does not distribute over the sum), use "l2"'),
    ("late-undeclared", lambda ix: ix.search_late(TOKENS, 3, "ns", "l2", "nope"), ValueError, _undeclared("search_late")),
    ("late-unstring", lambda ix: ix.search_late(TOKENS, 3, "ns", "l2", 5), ValueError, _undeclared("search_late", 5)),
    ("late-list", lambda ix: ix.search_late(TOKENS, 3, "ns", "l2", "nums"), ValueError,
     f"search_late: attribute 'nums' {SCALAR['nums']}"),
    ("late-float", lambda ix: ix.search_late(TOKENS, 3, "ns", "l2", "price"), ValueError,
     "search_late: attribute 'price' is a float column; documents need an int, str or bool attribute"),
    ("late-top_k", lambda ix: ix.search_late(TOKENS, 65, "ns", "l2", "year"), ValueError,
     "search_late: top_k must be <= 64 (got 65)"),
    ("late-where-list", lambda ix: ix.search_late(TOKENS, 3, "ns", "l2", "year", where=[None, None]), ValueError,
     "search_late: a per-query where list is not supported, give one dict filter"),
    ("late-ids", lambda ix: ix.search_late(TOKENS, 3, "ns", "l2", "year", allowed_ids=[uuid4()]), ValueError,
     "search_late: allowed_ids is not supported, give a dict where filter"),
    ("late-queries", lambda ix: ix.search_late(np.ones((2, DIM), np.float32), 3, "ns", "l2", "year"), ValueError,
     "search_late: queries must be a sequence of [T_i, dim] arrays or one [nq, T, dim] array"),
    ("late-tokens", lambda ix: ix.search_late([np.ones((129, DIM), np.float32)], 3, "ns", "l2", "year"), ValueError,
     "search_late: query 0 holds 129 tokens, 1 to 128 are supported"),
    ("late-dim", lambda ix: ix.search_late([np.ones((2, DIM + 1), np.float32)], 3, "ns", "l2", "year"), ValueError,
     "search_late: query 0 has token vectors of dim 5, expected 4"),
    ("late-where-type", lambda ix: ix.search_late(TOKENS, 3, "ns", "l2", "year", where=5), ValueError, COMPILE),
    # -- sparse
    ("sparse-undeclared", lambda ix: ix.search_sparse(SQ, 3, "ns", "nope"), ValueError, _undeclared("search_sparse")),
    ("sparse-unhashable", lambda ix: ix.search_sparse(SQ, 3, "ns", ["a"]), ValueError, _undeclared("search_sparse", ["a"])),
    ("sparse-kind", lambda ix: ix.search_sparse(SQ, 3, "ns", "year"), ValueError,
     "search_sparse: attribute 'year' is a int column; it needs a sparse attribute"),
    ("sparse-where-type", lambda ix: ix.search_sparse(SQ, 3, "ns", "terms", where=[None, None]), ValueError,
     f"search_sparse: {ONE_FILTER}"),
    ("sparse-one-mapping", lambda ix: ix.search_sparse({1: 1.0}, 3, "ns", "terms"), ValueError,
     "search_sparse: queries is a sequence of sparse vectors (got one mapping: wrap it in a list)"),
    ("sparse-query", lambda ix: ix.search_sparse([{1: 1.0}, {-1: 1.0}], 3, "ns", "terms"), ValueError,
     "search_sparse: query 1: term -1 is outside [0, 2^31)"),
    # -- hybrid
    ("hybrid-undeclared", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "nope"), ValueError, _undeclared("search_hybrid")),
    ("hybrid-kind", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "tags"), ValueError,
     "search_hybrid: attribute 'tags' is a str[] column; it needs a sparse attribute"),
    ("hybrid-fusion", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms", fusion="sum"), ValueError,
     "search_hybrid: fusion must be one of ('rrf', 'linear', 'relative') (got 'sum')"),
    ("hybrid-weights-type", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms", weights=("a", 1)), ValueError,
     "search_hybrid: weights is a pair of numbers and rrf_k a number (got ('a', 1), 60.0)"),
    ("hybrid-weights", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms", weights=(-1, 1)), ValueError,
     "search_hybrid: weights must be finite and >= 0 (got (-1, 1))"),
    ("hybrid-rrf_k", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms", rrf_k=-1), ValueError,
     "search_hybrid: rrf_k must be finite and >= 0 (got -1)"),
    ("hybrid-where-type", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms", where=[None, None]), ValueError,
     f"search_hybrid: {ONE_FILTER}"),
    ("hybrid-top_k", lambda ix: ix.search_hybrid(Q, SQ, 65, "ns", "l2", "terms"), ValueError,
     "search_hybrid: top_k must be <= 64 (got 65)"),
    ("hybrid-fetch_k", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms", fetch_k=0), ValueError,
     "search_hybrid: fetch_k must lie in [1, 1024] (got 0)"),
    ("hybrid-fetch_k_sparse", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms", fetch_k_sparse=65), ValueError,
     "search_hybrid: fetch_k_sparse must lie in [1, 64] (got 65)"),
    ("hybrid-top_k-fetch", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms", fetch_k=1, fetch_k_sparse=1), ValueError,
     "search_hybrid: top_k must be <= fetch_k + fetch_k_sparse (got 3 > 1 + 1)"),
    ("hybrid-one-mapping", lambda ix: ix.search_hybrid(Q, {1: 1.0}, 3, "ns", "l2", "terms"), ValueError,
     "search_hybrid: sparse_queries is a sequence of sparse vectors (got one mapping: wrap it in a list)"),
    ("hybrid-count", lambda ix: ix.search_hybrid(Q, SQ[:1], 3, "ns", "l2", "terms"), ValueError,
     "search_hybrid: 2 dense queries but 1 sparse queries"),
    ("hybrid-finite", lambda ix: ix.search_hybrid(np.full((2, DIM), np.inf, np.float32), SQ, 3, "ns", "l2", "terms"), ValueError,
     "search_hybrid: a dense query holds a non-finite value (NaN / inf)"),
    ("hybrid-query", lambda ix: ix.search_hybrid(Q, [{1: 1.0}, {1.5: 1.0}], 3, "ns", "l2", "terms"), ValueError,
     "search_hybrid: sparse query 1: term 1.5 is not an integer"),
    # -- range
    ("range-each-count", lambda ix: ix.range_search_many(Q, 1.0, "ns", "l2", where=[None]), ValueError,
     "range_search_many: 1 per-query filters for 2 queries"),
    ("range-each-type", lambda ix: ix.range_search_many(Q, 1.0, "ns", "l2", where=[None, 5]), ValueError, EACH),
    ("range-where-type", lambda ix: ix.range_search_many(Q, 1.0, "ns", "l2", where=5), ValueError, COMPILE),
    # -- count / query_by_metadata
    ("count-where-type", lambda ix: ix.count("ns", 5), ValueError, COMPILE),
    ("count_many-none", lambda ix: ix.count_many("ns", [{"year": 2000}, None]), ValueError,
     "count_many: every entry must be a dict filter"),
    ("count_many-type", lambda ix: ix.count_many("ns", [{"year": 2000}, 5]), ValueError, EACH),
    ("qbm-keywords", lambda ix: ix.query_by_metadata("ns", {"year": 2000}, limit=3), ValueError,
     "query_by_metadata: descending, limit and offset need order_by"),
    ("qbm-limit", lambda ix: ix.query_by_metadata("ns", {"year": 2000}, order_by="year"), ValueError,
     "query_by_metadata: order_by needs a limit (at most 4096 rows are ranked per call)"),
    ("qbm-where-type", lambda ix: ix.query_by_metadata("ns", 5), ValueError, COMPILE),
    # -- updates and deletes
    ("update-count", lambda ix: ix.update_attributes([uuid4()], [{"year": 1}, {"year": 2}], "ns"), ValueError,
     "update_attributes: 1 ids but 2 value mappings"),
    ("update-type", lambda ix: ix.update_attributes([uuid4()], [5], "ns"), ValueError,
     "update_attributes: values must be mappings, got int"),
    ("update-undeclared", lambda ix: ix.update_attributes([uuid4()], {"nope": 1}, "ns"), ValueError,
     f"'nope' is not a declared attribute of this index {DECLARED}"),
    ("update_where-values", lambda ix: ix.update_where("ns", {"year": 2000}, {}), ValueError,
     "update_where: values must be a non-empty mapping of declared attributes"),
    ("update_where-undeclared", lambda ix: ix.update_where("ns", {"year": 2000}, {"nope": 1}), ValueError,
     f"'nope' is not a declared attribute of this index {DECLARED}"),
    ("update_where-sparse", lambda ix: ix.update_where("ns", {"year": 2000}, {"terms": {1: 1.0}}), ValueError,
     "update_where: 'terms' is a sparse attribute: one vector for every matching row is not supported, use "
     "update_attributes with ids"),
    ("update_where-operator", lambda ix: ix.update_where("ns", {"year": 2000}, {"year": {"$mul": 2}}), ValueError,
     "update_where: 'year': the only operator is $inc (got ['$mul'])"),
    ("update_where-where-type", lambda ix: ix.update_where("ns", 5, {"year": 1}), ValueError, COMPILE),
    ("update_where-clash", lambda ix: ix.update_where("ns", {"year": 2000}, {"year": 1, "tags": ["x"]}), ValueError,
     "update_where: the filter reads ['year'], which this call assigns together with other attributes in several passes; "
     "assign them in a call of their own"),
    ("remove_where-where-type", lambda ix: ix.remove_where("ns", 5), ValueError, COMPILE),
    ("add-undeclared", lambda ix: ix.add_arrays(np.zeros((1, DIM), np.float32), "ns", attributes={"nope": [1]}), ValueError,
     f"'nope' is not a declared attribute of this index {DECLARED}"),
    # -- top_by
    ("top_by-undeclared", lambda ix: ix.top_by("ns", "nope", 3), ValueError, _undeclared("top_by")),
    ("top_by-unhashable", lambda ix: ix.top_by("ns", ["a"], 3), ValueError, _undeclared("top_by", ["a"])),
    ("top_by-list", lambda ix: ix.top_by("ns", "tags", 3), ValueError, f"top_by: attribute 'tags' {SCALAR['tags']}"),
    ("top_by-str", lambda ix: ix.top_by("ns", "genre", 3), ValueError,
     "top_by: attribute 'genre' is a str column; its codes are in order of first use, not in lexical order, so ranking "
     "needs an int, float or bool attribute"),
    ("top_by-limit", lambda ix: ix.top_by("ns", "year", 0), ValueError, "top_by: limit must be an int >= 1 (got 0)"),
    ("top_by-limit-bool", lambda ix: ix.top_by("ns", "year", True), ValueError, "top_by: limit must be an int >= 1 (got True)"),
    ("top_by-limit-float", lambda ix: ix.top_by("ns", "year", 2.0), ValueError, "top_by: limit must be an int >= 1 (got 2.0)"),
    ("top_by-offset", lambda ix: ix.top_by("ns", "year", 3, offset=-1), ValueError, "top_by: offset must be an int >= 0 (got -1)"),
    ("top_by-window", lambda ix: ix.top_by("ns", "year", 4096, offset=1), ValueError,
     "top_by: offset + limit must be <= 4096 (got 4097)"),
    ("top_by-descending", lambda ix: ix.top_by("ns", "year", 3, descending=1), ValueError,
     "top_by: descending must be a bool (got 1)"),
    ("top_by-where-type", lambda ix: ix.top_by("ns", "year", 3, [None]), ValueError, f"top_by: {ONE_FILTER}"),
    # -- nearest
    ("nearest-undeclared", lambda ix: ix.nearest("ns", "nope", (0, 0), 3), ValueError, _undeclared("nearest")),
    ("nearest-kind", lambda ix: ix.nearest("ns", "year", (0, 0), 3), ValueError,
     "nearest: attribute 'year' is a int column; it needs a geo attribute"),
    ("nearest-limit", lambda ix: ix.nearest("ns", "loc", (0, 0), 0), ValueError, "nearest: limit must be an int >= 1 (got 0)"),
    ("nearest-offset", lambda ix: ix.nearest("ns", "loc", (0, 0), 3, offset=True), ValueError,
     "nearest: offset must be an int >= 0 (got True)"),
    ("nearest-window", lambda ix: ix.nearest("ns", "loc", (0, 0), 4000, offset=97), ValueError,
     "nearest: offset + limit must be <= 4096 (got 4097)"),
    ("nearest-point", lambda ix: ix.nearest("ns", "loc", 5, 3), ValueError,
     "nearest: point: 5 is not a point, (lat, lon) or {'lat': .., 'lon': ..}"),
    ("nearest-where-type", lambda ix: ix.nearest("ns", "loc", (0, 0), 3, [None]), ValueError, f"nearest: {ONE_FILTER}"),
    # -- facets / histogram
    ("facets-undeclared", lambda ix: ix.facets("ns", "nope"), ValueError, _undeclared("facets")),
    ("facets-undeclared-listed", lambda ix: ix.facets("ns", ["year", "nope"]), ValueError, _undeclared("facets")),
    ("facets-unstring", lambda ix: ix.facets("ns", [5]), ValueError, _undeclared("facets", 5)),
    ("facets-sparse", lambda ix: ix.facets("ns", "terms"), ValueError, f"facets: attribute 'terms' {SCALAR['terms']}"),
    ("facets-geo", lambda ix: ix.facets("ns", "loc"), ValueError, f"facets: attribute 'loc' {SCALAR['loc']}"),
    ("facets-float", lambda ix: ix.facets("ns", "price"), ValueError,
     "facets: attribute 'price' is a float column; value facets need an int, str or bool attribute (histogram() bins floats)"),
    ("facets-order", lambda ix: ix.facets("ns", "year", order="name"), ValueError,
     'facets: order must be "count" or "value" (got \'name\')'),
    ("facets-limit", lambda ix: ix.facets("ns", "year", limit=0), ValueError, "facets: limit must be None or an int >= 1 (got 0)"),
    ("facets-max_values", lambda ix: ix.facets("ns", "year", max_values=(1 << 20) + 1), ValueError,
     "facets: max_values must be in 1..1048576 (got 1048577)"),
    ("facets-max_values-bool", lambda ix: ix.facets("ns", "year", max_values=True), ValueError,
     "facets: max_values must be in 1..1048576 (got True)"),
    ("facets-where-type", lambda ix: ix.facets("ns", "year", [None]), ValueError, f"facets: {ONE_FILTER}"),
    ("histogram-undeclared", lambda ix: ix.histogram("ns", "nope", [1]), ValueError, _undeclared("histogram")),
    ("histogram-list", lambda ix: ix.histogram("ns", "nums", [1]), ValueError, f"histogram: attribute 'nums' {SCALAR['nums']}"),
    ("histogram-kind", lambda ix: ix.histogram("ns", "genre", [1]), ValueError,
     "histogram: attribute 'genre' is a str column; bins need an int or float attribute"),
    ("histogram-edges", lambda ix: ix.histogram("ns", "year", []), ValueError, "histogram: 1..4096 edges (got 0)"),
    ("histogram-order", lambda ix: ix.histogram("ns", "year", [2, 1]), ValueError,
     "histogram: edges must be strictly ascending (unsorted or duplicate edges)"),
    ("histogram-where-type", lambda ix: ix.histogram("ns", "year", [1], [None]), ValueError, f"histogram: {ONE_FILTER}"),
    # -- stats
    ("stats-undeclared", lambda ix: ix.stats("ns", "nope"), ValueError, _undeclared("stats")),
    ("stats-by-undeclared", lambda ix: ix.stats("ns", "year", by="nope"), ValueError, _undeclared("stats")),
    ("stats-by-unhashable", lambda ix: ix.stats("ns", "year", by=["genre"]), ValueError, _undeclared("stats", ["genre"])),
    ("stats-geo", lambda ix: ix.stats("ns", "loc"), ValueError, f"stats: attribute 'loc' {SCALAR['loc']}"),
    ("stats-kind", lambda ix: ix.stats("ns", "genre"), ValueError,
     "stats: attribute 'genre' is a str column; min, max and sum need an int, float or bool attribute"),
    ("stats-by-float", lambda ix: ix.stats("ns", "year", by="price"), ValueError,
     "stats: by='price' is a float column; groups need an int, str or bool attribute"),
    ("stats-max_groups", lambda ix: ix.stats("ns", "year", by="genre", max_groups=0), ValueError,
     "stats: max_groups must be in 1..1048576 (got 0)"),
    ("stats-where-type", lambda ix: ix.stats("ns", "year", [None]), ValueError, f"stats: {ONE_FILTER}"),
    # ---------------------------------------------------------------- two faults in one call: the refusal that wins
    ("2-undeclared-then-kind-stats", lambda ix: ix.stats("ns", ["genre", "nope"]), ValueError, _undeclared("stats")),
    ("2-scalar-then-undeclared-stats", lambda ix: ix.stats("ns", ["terms", "nope"]), ValueError,
     f"stats: attribute 'terms' {SCALAR['terms']}"),
    ("2-kind-then-undeclared-facets", lambda ix: ix.facets("ns", ["price", "nope"]), ValueError,
     "facets: attribute 'price' is a float column; value facets need an int, str or bool attribute (histogram() bins floats)"),
    ("2-undeclared-then-kind-facets", lambda ix: ix.facets("ns", ["nope", "price"]), ValueError, _undeclared("facets")),
    ("2-undeclared-then-limit-top_by", lambda ix: ix.top_by("ns", "nope", 0), ValueError, _undeclared("top_by")),
    ("2-kind-then-limit-nearest", lambda ix: ix.nearest("ns", "year", 5, 0), ValueError,
     "nearest: attribute 'year' is a int column; it needs a geo attribute"),
    ("2-top_k-then-where-list-distinct", lambda ix: ix.search_many(Q, 65, "ns", "l2", distinct="year", where=[None, None]),
     ValueError, "distinct: top_k must be <= 64 (got 65)"),
    ("2-top_k-then-where-list-mmr", lambda ix: ix.search_many(Q, 65, "ns", "l2", mmr_lambda=0.5, where=[None, None]),
     ValueError, "mmr_lambda: top_k must be <= 64 (got 65)"),
    ("2-top_k-then-where-list-late", lambda ix: ix.search_late(TOKENS, 65, "ns", "l2", "year", where=[None, None]),
     ValueError, "search_late: top_k must be <= 64 (got 65)"),
    ("2-where-list-then-ids-distinct",
     lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="year", where=[None, None], allowed_ids=[uuid4()]), ValueError,
     "distinct: a per-query where list is not supported, give one dict filter"),
    ("2-group_size-then-undeclared", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="nope", group_size=65), ValueError,
     "group_size must be an int in [1, 64] (got 65)"),
    ("2-fetch_k-then-ids-mmr", lambda ix: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=0.5, fetch_k=2, allowed_ids=[uuid4()]),
     ValueError, "mmr_lambda: fetch_k must be >= top_k (got fetch_k=2, top_k=3)"),
    ("2-where-type-then-namespace-many", lambda ix: ix.search_many(Q, 3, "nowhere", "l2", where=5), ValueError, COMPILE),
    ("2-where-type-then-namespace-top_by", lambda ix: ix.top_by("nowhere", "year", 3, [None]), ValueError, f"top_by: {ONE_FILTER}"),
    ("2-where-type-then-namespace-facets", lambda ix: ix.facets("nowhere", "year", [None]), ValueError, f"facets: {ONE_FILTER}"),
    ("2-where-type-then-namespace-stats", lambda ix: ix.stats("nowhere", "year", [None]), ValueError, f"stats: {ONE_FILTER}"),
    ("2-where-type-then-namespace-sparse", lambda ix: ix.search_sparse(SQ, 3, "nowhere", "terms", where=[None, None]),
     ValueError, f"search_sparse: {ONE_FILTER}"),
    ("2-where-type-then-namespace-count", lambda ix: ix.count("nowhere", 5), ValueError, COMPILE),
    ("2-limit-then-offset-top_by", lambda ix: ix.top_by("ns", "year", 0, offset=-1), ValueError,
     "top_by: limit must be an int >= 1 (got 0)"),
    ("2-limit-then-offset-nearest", lambda ix: ix.nearest("ns", "loc", (0, 0), 0, offset=-1), ValueError,
     "nearest: limit must be an int >= 1 (got 0)"),
    ("2-offset-then-descending-top_by", lambda ix: ix.top_by("ns", "year", 3, descending=1, offset=-1), ValueError,
     "top_by: offset must be an int >= 0 (got -1)"),
    ("2-window-then-point-nearest", lambda ix: ix.nearest("ns", "loc", 5, 4096, offset=1), ValueError,
     "nearest: offset + limit must be <= 4096 (got 4097)"),
    ("2-args-then-where-type-histogram", lambda ix: ix.histogram("ns", "year", [], [None]), ValueError,
     "histogram: 1..4096 edges (got 0)"),
    # (the filter is compiled last: whatever the arguments themselves have wrong is said first)
    ("2-query-then-filter-sparse", lambda ix: ix.search_sparse([{-1: 1.0}], 3, "ns", "terms", where={"nope": 1}), ValueError,
     "search_sparse: query 0: term -1 is outside [0, 2^31)"),
    ("2-query-then-filter-hybrid", lambda ix: ix.search_hybrid(Q, [{1: 1.0}, {-1: 1.0}], 3, "ns", "l2", "terms", where={"nope": 1}),
     ValueError, "search_hybrid: sparse query 1: term -1 is outside [0, 2^31)"),
    ("2-where-type-then-top_k-hybrid", lambda ix: ix.search_hybrid(Q, SQ, 65, "ns", "l2", "terms", where=[None, None]),
     ValueError, f"search_hybrid: {ONE_FILTER}"),
    ("2-tokens-then-filter-late", lambda ix: ix.search_late([np.ones((129, DIM), np.float32)], 3, "ns", "l2", "year", where=5),
     ValueError, "search_late: query 0 holds 129 tokens, 1 to 128 are supported"),
    ("2-top_k-then-filter-like", lambda ix: ix.search_like([uuid4()], 1024, "ns", "l2", where=5), ValueError,
     "search_like: top_k + examples must be <= 1024 (got 1024 + 1)"),
    ("2-filter-then-base-count-like", lambda ix: ix.search_like([uuid4()], 3, "ns", "l2", where=5, queries=Q), ValueError,
     COMPILE),
    ("2-filter-then-values-update_where", lambda ix: ix.update_where("ns", 5, {}), ValueError, COMPILE),
    ("2-keywords-then-where-type-qbm", lambda ix: ix.query_by_metadata("ns", 5, limit=3), ValueError,
     "query_by_metadata: descending, limit and offset need order_by"),
    ("2-count-then-filter-each", lambda ix: ix.search_many(Q, 3, "ns", "l2", where=[5]), ValueError,
     "search_many: 1 per-query filters for 2 queries"),
]


@pytest.mark.parametrize("call, exc, message", [pytest.param(*row[1:], id=row[0]) for row in REFUSALS])
def test_refusal(index, call, exc, message):
    with pytest.raises(exc, match="^" + re.escape(message) + "$"):
        call(index)


def test_refusals_left_the_index_as_it_was(index, filled):
    assert index.namespace_counts("ns") == (N, 0)
    assert index.count("ns", {"year": {"$gte": 2000}}) == N
    assert [h.vector_id for h in index.search_many(filled[1][2].values[None, :], 1, "ns", "l2")[0]] == [filled[1][2].id]


# ---------------------------------------------------------------- a row-sharded index: its refusal comes first
SHARDED_REFUSALS = [
    ("distinct", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="nope"), f"distinct= {SHARDED}"),
    ("mmr", lambda ix: ix.search_many(Q, 65, "ns", "l2", mmr_lambda=2.0), f"mmr_lambda= {SHARDED}"),
    ("late", lambda ix: ix.search_late(TOKENS, 3, "ns", "euclidean", "nope"), f"search_late {SHARDED}"),
    ("sparse", lambda ix: ix.search_sparse(SQ, 3, "ns", "nope"), f"search_sparse {SHARDED}"),
    ("hybrid", lambda ix: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "nope"), f"search_hybrid {SHARDED}"),
    ("like", lambda ix: ix.search_like([uuid4()], 3, "ns", "l2", where=[None]), f"search_like {SHARDED}"),
    ("stats", lambda ix: ix.stats("ns", "nope"), f"stats {SHARDED}"),
    # group_size is checked before the devices; the families below have no sharded refusal of their own: no attribute is declared
    ("group_size", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct="nope", group_size=0),
     "group_size must be an int in [1, 64] (got 0)"),
    ("top_by", lambda ix: ix.top_by("ns", "nope", 3), "top_by: 'nope' is not a declared attribute of this index (declared: [])"),
    ("nearest", lambda ix: ix.nearest("ns", "nope", (0, 0), 3),
     "nearest: 'nope' is not a declared attribute of this index (declared: [])"),
    ("facets", lambda ix: ix.facets("ns", "nope"), "facets: 'nope' is not a declared attribute of this index (declared: [])"),
    ("histogram", lambda ix: ix.histogram("ns", "nope", [1]),
     "histogram: 'nope' is not a declared attribute of this index (declared: [])"),
]


@pytest.mark.parametrize("call, message", [pytest.param(*row[1:], id=row[0]) for row in SHARDED_REFUSALS])
def test_sharded_refusal(sharded, call, message):
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        call(sharded)


# ---------------------------------------------------------------- the one refusal that changed when the helpers came
# Every other row of this file passed unchanged on the commit before ``Index`` got its shared helpers.  These three did
# not: their sites tested ``name not in self._attributes`` without asking first whether the name is a string, so an
# unhashable name raised ``TypeError: unhashable type: 'list'`` there and the family's ``ValueError`` at the other nine
# sites.  ``Index._declared`` always asks, so the three now raise their ``ValueError`` too (against the commit before,
# this table held ``TypeError`` and "unhashable type: 'list'" three times, and passed).
UNHASHABLE = [
    ("distinct", lambda ix: ix.search_many(Q, 3, "ns", "l2", distinct=["a"]), ValueError, _undeclared("distinct", ["a"])),
    ("late", lambda ix: ix.search_late(TOKENS, 3, "ns", "l2", ["a"]), ValueError, _undeclared("search_late", ["a"])),
    ("facets", lambda ix: ix.facets("ns", [["a"]]), ValueError, _undeclared("facets", ["a"])),
]


@pytest.mark.parametrize("call, exc, message", [pytest.param(*row[1:], id=row[0]) for row in UNHASHABLE])
def test_unhashable_attribute_name(index, call, exc, message):
    with pytest.raises(exc, match="^" + re.escape(message) + "$"):
        call(index)


# ---------------------------------------------------------------- an engine without the family's entry
def _needs(subject, method):
    return f"{subject} an engine with {method} (a single-device namespace)"


LACKING = [
    ("search_distinct", lambda ix, v: ix.search_many(Q, 3, "ns", "l2", distinct="year"), _needs("distinct= needs", "search_distinct")),
    ("search_grouped", lambda ix, v: ix.search_many(Q, 3, "ns", "l2", distinct="year", group_size=2),
     _needs("group_size= needs", "search_grouped")),
    ("search_maxsim", lambda ix, v: ix.search_late(TOKENS, 3, "ns", "l2", "year"), _needs("search_late needs", "search_maxsim")),
    ("search_batch_sparse", lambda ix, v: ix.search_sparse(SQ, 3, "ns", "terms"),
     _needs("sparse attributes need", "search_batch_sparse")),
    ("search_hybrid", lambda ix, v: ix.search_hybrid(Q, SQ, 3, "ns", "l2", "terms"), _needs("search_hybrid needs", "search_hybrid")),
    ("search_mmr", lambda ix, v: ix.search_many(Q, 3, "ns", "l2", mmr_lambda=0.5), _needs("mmr_lambda= needs", "search_mmr")),
    ("search_like", lambda ix, v: ix.search_like([v[0].id], 3, "ns", "l2"), _needs("search_like needs", "search_like")),
    ("search_each", lambda ix, v: ix.search_many(Q, 3, "ns", "l2", where=[{"year": 2000}, None]),
     _needs("per-query filters need", "search_each")),
    ("range_each", lambda ix, v: ix.range_search_many(Q, 1.0, "ns", "l2", where=[{"year": 2000}, None]),
     _needs("per-query filters need", "range_each")),
    ("where_ordered", lambda ix, v: ix.top_by("ns", "year", 3), _needs("top_by needs", "where_ordered")),
    ("geo_nearest", lambda ix, v: ix.nearest("ns", "loc", (0, 0), 3), _needs("nearest needs", "geo_nearest")),
    ("facet_values", lambda ix, v: ix.facets("ns", "year"), _needs("facets needs", "facet_values")),
    ("facet_list_values", lambda ix, v: ix.facets("ns", "tags"), _needs("facets needs", "facet_values")),
    ("facet_bins", lambda ix, v: ix.histogram("ns", "year", [2001]), _needs("histogram needs", "facet_bins")),
    ("attr_stats", lambda ix, v: ix.stats("ns", "year"), _needs("stats needs", "attr_stats")),
    ("set_attr_at", lambda ix, v: ix.update_attributes([v[0].id], {"year": 1}, "ns"), _needs("update_attributes needs", "set_attr_at")),
    ("set_attr_list_at", lambda ix, v: ix.update_attributes([v[0].id], {"tags": ["x"]}, "ns"),
     _needs("list attributes need", "set_attr_list_at")),
    ("set_attr_sparse_at", lambda ix, v: ix.update_attributes([v[0].id], {"terms": {1: 1.0}}, "ns"),
     _needs("sparse attributes need", "set_attr_sparse_at")),
    ("update_where", lambda ix, v: ix.update_where("ns", {"year": 2000}, {"year": 1}), _needs("update_where needs", "update_where")),
    ("update_where_list", lambda ix, v: ix.update_where("ns", {"year": 2000}, {"tags": ["x"]}),
     _needs("list attributes need", "update_where_list")),
    ("tombstone_where", lambda ix, v: ix.remove_where("ns", {"year": 2000}), _needs("remove_where needs", "tombstone_where")),
]


@pytest.mark.parametrize("method, call, message", [pytest.param(*row, id=row[0]) for row in LACKING])
def test_an_engine_without_the_entry(method, call, message):
    index, vecs = _filled(type("Without", (Lacking,), {"lacking": frozenset([method])}))
    with pytest.raises(ValueError, match="^" + re.escape(message) + "$"):
        call(index, vecs)


@pytest.mark.parametrize("method, subject", [("set_attr_list", "list attributes need"), ("set_attr_sparse", "sparse attributes need")])
def test_an_engine_without_the_ingest_entry(method, subject):
    with pytest.raises(ValueError, match="^" + re.escape(_needs(subject, method)) + "$"):
        _filled(type("Without", (Lacking,), {"lacking": frozenset([method])}))


@pytest.mark.parametrize("method, subject", [("get_attr_list", "list attributes need"), ("get_attr_sparse", "sparse attributes need")])
def test_an_engine_without_the_snapshot_entry(method, subject, tmp_path):
    index, _ = _filled(type("Without", (Lacking,), {"lacking": frozenset([method])}))
    with pytest.raises(ValueError, match="^" + re.escape(_needs(subject, method)) + "$"):
        index.save_index(str(tmp_path))


def test_an_engine_without_search_stream_is_no_refusal():
    index, _ = _filled(type("Without", (Lacking,), {"lacking": frozenset(["search_stream"])}))
    got = list(index.search_stream([Q, Q[:1]], 3, "ns", "l2"))
    assert [type(g) for g in got] == [BatchHits, BatchHits] and [g.labels.shape for g in got] == [(2, 3), (1, 3)]


# ---------------------------------------------------------------- the answers that need no search
def _batch(got, cls, nq):
    assert type(got) is cls and len(got) == nq
    assert got.labels.shape == (nq, 0) and got.labels.dtype == np.int64
    assert got.scores.shape == (nq, 0) and got.scores.dtype == np.float64
    assert got.counts.shape == (nq,) and got.counts.dtype == np.int32 and not got.counts.any()
    assert list(got) == [[] for _ in range(nq)]


def _late(got, lengths, matches):
    nq, ntok = len(lengths), sum(lengths)
    assert type(got) is LateBatchHits and len(got) == nq
    assert got.values.shape == (nq, 0) and got.scores.shape == (nq, 0) and got.counts.shape == (nq,) and not got.counts.any()
    assert got.offsets.tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist() and got.offsets.dtype == np.int64
    if matches:
        assert got.match_labels.shape == (ntok, 0) and got.match_scores.shape == (ntok, 0)
    else:
        assert got.match_labels is None and got.match_scores is None


def _kNN_families(ix, ns, k, q, sq, tokens):
    """Every kNN-shaped family on ``ns`` with ``k`` and the query batch given three ways -> {family: answer}."""
    nq = len(q)
    return {
        "plain": ix.search_many(q, k, ns, "l2"),
        "where": ix.search_many(q, k, ns, "l2", where={"year": 2000}),
        "ids": ix.search_many(q, k, ns, "l2", allowed_ids=[uuid4()]),
        "each": ix.search_many(q, k, ns, "l2", where=[None] * nq),
        "each-filtered": ix.search_many(q, k, ns, "l2", where=[{"year": 2000}] * nq),
        "distinct": ix.search_many(q, k, ns, "l2", distinct="genre"),
        "grouped": ix.search_many(q, k, ns, "l2", distinct="genre", group_size=2),
        "mmr": ix.search_many(q, k, ns, "l2", mmr_lambda=0.5),
        "sparse": ix.search_sparse(sq, k, ns, "terms"),
        "hybrid": ix.search_hybrid(q, sq, k, ns, "l2", "terms"),
        "hybrid-components": ix.search_hybrid(q, sq, k, ns, "l2", "terms", components=True),
        "like": ix.search_like([[uuid4()]] * nq, k, ns, "l2"),
        "late": ix.search_late(tokens, k, ns, "l2", "genre"),
        "late-matches": ix.search_late(tokens, k, ns, "l2", "genre", matches=True),
    }


def _check_kNN_families(got, nq, lengths):
    for family, answer in got.items():
        if family.startswith("late"):
            _late(answer, lengths, family == "late-matches")
        else:
            _batch(answer, {"grouped": GroupedBatchHits, "hybrid-components": HybridBatchHits}.get(family, BatchHits), nq)
    assert got["grouped"].group_sizes.shape == (nq, 0) and got["grouped"].group_sizes.dtype == np.int32
    assert got["grouped"].group_values.shape == (nq, 0) and got["grouped"].group_values.dtype == object
    comp = got["hybrid-components"]
    assert comp.dense.shape == comp.sparse.shape == comp.rank_dense.shape == comp.rank_sparse.shape == (nq, 0)
    assert comp.dense.dtype == comp.sparse.dtype == np.float64 and comp.rank_dense.dtype == comp.rank_sparse.dtype == np.int32


@pytest.fixture(scope="module")
def emptied():
    index, vecs = _filled()
    index.remove([v.id for v in vecs], "ns")
    return index


def test_empty_answers_of_the_kNN_families_unknown_namespace(index):
    _check_kNN_families(_kNN_families(index, "nowhere", 3, Q, SQ, TOKENS), 2, [2, 3])


def test_empty_answers_of_the_kNN_families_all_rows_removed(emptied):
    _check_kNN_families(_kNN_families(emptied, "ns", 3, Q, SQ, TOKENS), 2, [2, 3])


@pytest.mark.parametrize("k", [0, -1])
def test_empty_answers_of_the_kNN_families_top_k_zero(index, k):
    _check_kNN_families(_kNN_families(index, "ns", k, Q, SQ, TOKENS), 2, [2, 3])


def test_empty_answers_of_the_kNN_families_zero_queries(index):
    got = _kNN_families(index, "ns", 3, np.zeros((0, DIM), np.float32), [], [])
    _check_kNN_families(got, 0, [])


def test_empty_answers_of_the_kNN_families_wrong_query_dim(index):
    wide = np.ones((2, DIM + 1), np.float32)
    got = {
        "plain": index.search_many(wide, 3, "ns", "l2"),
        "where": index.search_many(wide, 3, "ns", "l2", where={"year": 2000}),
        "each": index.search_many(wide, 3, "ns", "l2", where=[{"year": 2000}, None]),
        "distinct": index.search_many(wide, 3, "ns", "l2", distinct="genre"),
        "mmr": index.search_many(wide, 3, "ns", "l2", mmr_lambda=0.5),
        "hybrid": index.search_hybrid(wide, SQ, 3, "ns", "l2", "terms"),
        "like": index.search_like([[uuid4()]] * 2, 3, "ns", "l2", queries=wide),
    }
    for answer in got.values():
        _batch(answer, BatchHits, 2)
    _batch(index.search_many(wide, 3, "ns", "l2", distinct="genre", group_size=2), GroupedBatchHits, 2)
    _batch(index.search_hybrid(wide, SQ, 3, "ns", "l2", "terms", components=True), HybridBatchHits, 2)
    assert index.range_search_many(wide, 1.0, "ns", "l2") == [[], []]
    assert index.range_search_many(wide, 1.0, "ns", "l2", where=[{"year": 2000}, None]) == [[], []]
    assert index.search(Vector(values=np.ones((2, 2), np.float32), metadata={}), 3, "ns", "l2") == []
    assert index.range_search(Vector(values=np.ones((2, 2), np.float32), metadata={}), 1.0, "ns", "l2") == []
    assert [len(b) for b in index.search_stream([wide, wide[:1]], 3, "ns", "l2")] == [2, 1]


def test_empty_answers_of_range_and_stream(index, emptied):
    for ix, ns in ((index, "nowhere"), (emptied, "ns")):
        assert ix.range_search_many(Q, 1.0, ns, "l2") == [[], []]
        assert ix.range_search_many(Q, 1.0, ns, "l2", where={"year": 2000}) == [[], []]
        assert ix.range_search_many(Q, 1.0, ns, "l2", where=[{"year": 2000}, None]) == [[], []]
        got = list(ix.search_stream([Q, Q[:1]], 3, ns, "l2"))
        _batch(got[0], BatchHits, 2)
        _batch(got[1], BatchHits, 1)
    assert index.range_search_many(np.zeros((0, DIM), np.float32), 1.0, "ns", "l2") == []
    _batch(next(iter(index.search_stream([Q], 0, "ns", "l2"))), BatchHits, 2)


NO_STATS = {"matched": 0, "absent": 0, "count": 0, "min": None, "max": None, "sum": 0, "mean": None}


def _check_metadata_families(ix, ns):
    assert ix.count(ns, {"year": 2000}) == 0 and type(ix.count(ns, {"year": 2000})) is int
    assert ix.count_many(ns, [{"year": 2000}, {"genre": "a"}]) == [0, 0]
    assert ix.query_by_metadata(ns, {"year": 2000}) == []
    assert ix.query_by_metadata(ns, {"year": 2000}, order_by="year", limit=3) == []
    assert ix.top_by(ns, "year", 3) == {"ids": [], "values": [], "matched": 0, "absent": 0}
    assert ix.nearest(ns, "loc", (0, 0), 3) == {"ids": [], "points": [], "distances": [], "matched": 0, "absent": 0}
    assert ix.facets(ns, "genre") == {"values": [], "matched": 0, "absent": 0}
    assert ix.facets(ns, ["genre", "tags"]) == {name: {"values": [], "matched": 0, "absent": 0} for name in ("genre", "tags")}
    hist = ix.histogram(ns, "year", [2001, 2003])
    assert set(hist) == {"counts", "matched", "absent"} and hist["matched"] == hist["absent"] == 0
    assert hist["counts"].dtype == np.int64 and hist["counts"].tolist() == [0, 0, 0]
    assert ix.stats(ns, "year") == NO_STATS
    assert ix.stats(ns, ["year", "price"]) == {"year": NO_STATS, "price": NO_STATS}
    assert ix.stats(ns, "year", by="genre") == {"groups": [], "matched": 0, "by_absent": 0}
    assert ix.update_where(ns, {"year": 2000}, {"year": 1}) == 0
    assert ix.remove_where(ns, {"year": 2000}) == 0
    assert ix.remove_where(ns, {"year": 2000}, return_ids=True) == []
    assert ix.update_attributes([uuid4()], {"year": 1}, ns) == 0


def test_empty_answers_of_the_metadata_families_unknown_namespace(index):
    _check_metadata_families(index, "nowhere")
    assert index.update_attributes([], {"year": 1}, "ns") == 0
    assert index.update_attributes([uuid4()], {}, "ns") == 0
    assert index.count_many("ns", []) == []


def test_empty_answers_of_the_metadata_families_all_rows_removed(emptied):
    """Rows that are all tombstoned still reach the engine (its columns hold them): the answers are the engine's."""
    _check_metadata_families(emptied, "ns")
