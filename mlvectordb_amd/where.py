"""Dict metadata filters -> the postfix predicate program the device evaluates (include/mlvdb_where.h).

A filter is a dict over a namespace's declared attributes (``Index(attributes={"genre": "str", "year": "int", ...})``):

    {"genre": "jazz"}                              equality
    {"year": {"$gte": 2000, "$lt": 2010}}          several operators on one key: AND
    {"$or": [{"genre": "jazz"}, {"year": {"$lt": 1960}}]}
    {"genre": {"$in": ["jazz", "blues"]}, "in_stock": True}   several keys: AND;  {} matches every row

Operators ``$eq $ne $lt $lte $gt $gte $in $nin $exists``; combinators ``$and $or $not``.  Semantics on a row without a value
(key missing, ``None``, NaN for a float attribute): every comparison, ``$eq`` and ``$in`` is false; ``$ne`` / ``$nin`` are
their negations, so such a row matches them; ``$exists: False`` matches it.

Type rules: ``int`` / ``bool`` attributes take int and bool literals only (a float literal is refused), ``float`` attributes
take int and float literals, ``str`` attributes take strings and only ``$eq $ne $in $nin $exists`` (matched through the
namespace's dictionary codes: a string never ingested matches nothing).  A key that is not a declared attribute, or a
program longer than 64 ops or deeper than 32, is a ``ValueError``: there is no slow host path to fall back to.

List attributes (``"str[]"`` / ``"int[]"``: a set of at most 255 tags per row, include/mlvdb_list.h) take

    {"tags": "jazz"} / $eq      the list contains it        $ne      it does not (a row without a list matches)
    {"tags": {"$in": [...]}}    any of them                 $nin     none of them (a row without a list matches)
    {"tags": {"$all": [...]}}   all of them (not empty)     $size    3, or {"$gte": 1, "$lt": 4}: the list's length
    $exists                     as above; an empty list ``[]`` exists, ``None`` / a missing key does not

A string never ingested matches nothing, so ``$all`` with one is false as a whole.  ``$lt`` .. ``$gte`` on a list
attribute, and ``$all`` / ``$size`` on a scalar one, are a ``ValueError``.

A sparse attribute (``"sparse"``: at most 255 (term, weight) pairs per row, include/mlvdb_sparse.h) takes ``$exists`` and
``$size`` (the number of its nonzeros) only; an empty vector ``{}`` exists.  Everything else on it is a ``ValueError``.

A bits attribute (``"bits<N>"``, e.g. ``"bits256"``: one ``N``-bit code per row, ``N`` a multiple of 64 in [64, 16320],
include/mlvdb_bits.h) takes ``$exists`` only: it is searched with ``Index.search_bits``, not filtered by value.

A geo attribute (``"geo"``: one location per row, include/mlvdb_geo.h) holds a point ``(lat, lon)`` or
``{"lat": .., "lon": ..}`` in degrees, quantised to 1e-7 degree, and takes

    {"loc": {"$geo_radius": {"center": point, "radius": metres}}}    great-circle distance <= radius (R = 6371008.8 m)
    {"loc": {"$geo_box": {"sw": point, "ne": point}}}                inclusive; sw.lon > ne.lon: across the antimeridian
    $exists

only; centres and corners are quantised exactly as stored points are.  Everything else on it, and both geo operators on
another attribute, are a ``ValueError``.
"""
from __future__ import annotations

import math
import re
import struct
from dataclasses import dataclass
from typing import Any, Dict, List, Mapping, Tuple

import numpy as np

ATTR_TYPES = ("int", "float", "str", "bool")
LIST_TYPES = ("str[]", "int[]")  # list-valued attributes: a set of strings / ints per row
LIST_MAX_LEN = 255               # MLVDB_LIST_MAX_LEN
SPARSE_TYPES = ("sparse",)       # sparse vectors: (term, weight) pairs per row, searched by Index.search_sparse
SPARSE_MAX_NNZ = 255             # MLVDB_SPARSE_MAX_NNZ
SPARSE_MAX_QUERY_TERMS = 1024    # MLVDB_SPARSE_MAX_QUERY_TERMS
BITS_TYPES = ("bits<N>",)        # bit codes: "bits64" .. "bits16320", N a multiple of 64, searched by Index.search_bits
BITS_MAX_WORDS = 255             # MLVDB_BITS_MAX_WORDS
_BITS_TYPE = re.compile(r"bits([1-9][0-9]*)\Z")
GEO_TYPES = ("geo",)             # one location per row: (lat_e7 << 32) | uint32(lon_e7) in an int64 column
GEO_LAT_MAX_E7 = 900_000_000     # MLVDB_GEO_LAT_MAX_E7
GEO_LON_MAX_E7 = 1_800_000_000   # MLVDB_GEO_LON_MAX_E7
GEO_EARTH_RADIUS_M = 6371008.8   # MLVDB_GEO_EARTH_RADIUS_M
MAX_ATTRS = 16
MAX_OPS = 64
MAX_DEPTH = 32

# op codes (MLVDB_WHERE_*)
TRUE, EQ, NE, LT, LE, GT, GE, IN, EXISTS, AND, OR, NOT = range(12)
HAS, HAS_ANY, HAS_ALL, LEN = range(12, 16)  # list columns only (include/mlvdb_list.h)
GEO_BOX, GEO_RADIUS = 16, 17  # geo columns only (include/mlvdb_geo.h)
_COMBINATORS = (AND, OR, NOT)
OP_DTYPE = np.dtype([("op", "<i4"), ("attr", "<i4"), ("a", "<i8"), ("b", "<i8")])  # mlvdb_where_op

_ORDERED = {"$lt": LT, "$lte": LE, "$gt": GT, "$gte": GE}
_FIELD_OPS = ("$eq", "$ne", "$lt", "$lte", "$gt", "$gte", "$in", "$nin", "$exists", "$all", "$size", "$geo_radius",
              "$geo_box")
_LIST_ONLY = ("$all", "$size")
_GEO_ONLY = ("$geo_radius", "$geo_box")


@dataclass
class Program:
    """A compiled filter: ``ops`` (structured array in the layout of ``mlvdb_where_op``) and the int64 ``set`` table the IN
    ops index into (each op's range sorted ascending)."""

    ops: np.ndarray
    set: np.ndarray


def float_bits(x: float) -> int:
    """The int64 carrying a double's bit pattern (the ``a`` of an op on a float64 column)."""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def is_list(attr_type: str) -> bool:
    return attr_type in LIST_TYPES


def is_sparse(attr_type: str) -> bool:
    return attr_type in SPARSE_TYPES


def is_geo(attr_type: str) -> bool:
    return attr_type in GEO_TYPES


def is_bits(attr_type: str) -> bool:
    """``"bits<N>"`` with ``N`` a multiple of 64 in [64, 64 * BITS_MAX_WORDS]."""
    m = _BITS_TYPE.match(attr_type) if isinstance(attr_type, str) else None
    return m is not None and int(m.group(1)) % 64 == 0 and int(m.group(1)) <= 64 * BITS_MAX_WORDS


def bits_width(attr_type: str) -> int:
    """The ``N`` of a ``"bits<N>"`` attribute type."""
    if not is_bits(attr_type):
        raise ValueError(f"{attr_type!r} is not a bits type: 'bits<N>' with N a multiple of 64 in [64, {64 * BITS_MAX_WORDS}]")
    return int(attr_type[4:])


def geo_pack(point: Any, what: str = "a point") -> int:
    """A point -- ``(lat, lon)`` or ``{"lat": .., "lon": ..}``, finite degrees with lat in [-90, 90] and lon in
    [-180, 180] -- as the int64 a geo column holds: ``(lat_e7 << 32) | uint32(lon_e7)``, each ``np.rint(x * 1e7)``.
    ``ValueError`` (starting with ``what``) for anything else."""
    if isinstance(point, Mapping):
        if set(point) != {"lat", "lon"}:
            raise ValueError(f"{what}: a point dict holds exactly 'lat' and 'lon', got {sorted(map(str, point))}")
        pair = (point["lat"], point["lon"])
    elif isinstance(point, (tuple, list)) and len(point) == 2:
        pair = tuple(point)
    else:
        raise ValueError(f"{what}: {point!r} is not a point, (lat, lon) or {{'lat': .., 'lon': ..}}")
    for x in pair:
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what}: the coordinate {x!r} is not a number")
    lat, lon = float(pair[0]), float(pair[1])
    if not (math.isfinite(lat) and math.isfinite(lon) and -90.0 <= lat <= 90.0 and -180.0 <= lon <= 180.0):
        raise ValueError(f"{what}: ({lat}, {lon}) is outside lat in [-90, 90], lon in [-180, 180]")
    return (int(np.rint(lat * 1e7)) << 32) | (int(np.rint(lon * 1e7)) & 0xFFFFFFFF)


def geo_unpack(value: int) -> Tuple[int, int]:
    """A stored geo value -> ``(lat_e7, lon_e7)``."""
    value = int(value)
    lon = value & 0xFFFFFFFF
    return value >> 32, lon - (1 << 32) if lon >= 1 << 31 else lon


def geo_degrees(value: int) -> Tuple[float, float]:
    """A stored geo value -> ``(lat, lon)`` in degrees."""
    lat, lon = geo_unpack(value)
    return lat / 1e7, lon / 1e7


def geo_radius_threshold(radius: Any, what: str = "$geo_radius") -> float:
    """``sin^2(r / 2R)`` clamped to 1 for a radius in metres (finite, >= 0): what GEO_RADIUS compares hav against."""
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: the radius {radius!r} is not a number of metres")
    r = float(radius)
    if not math.isfinite(r) or r < 0.0:
        raise ValueError(f"{what}: the radius must be finite and >= 0 metres, got {r}")
    half = r / (2.0 * GEO_EARTH_RADIUS_M)
    return 1.0 if half >= math.pi / 2 else min(1.0, math.sin(half) ** 2)


def is_pooled(attr_type: str) -> bool:
    """A list, a sparse or a bits attribute: the column holds slots into a pool, not values."""
    return is_list(attr_type) or is_sparse(attr_type) or is_bits(attr_type)


def column_kind(attr_type: str) -> str:
    """The device column type of an attribute type: float -> float64, a list type -> int64_list, sparse -> sparse,
    bits<N> -> bits, geo -> geo, everything else -> int64."""
    return "float64" if attr_type == "float" else "int64_list" if is_list(attr_type) else \
        "sparse" if is_sparse(attr_type) else "bits" if is_bits(attr_type) else "geo" if is_geo(attr_type) else "int64"


class _Builder:
    def __init__(self, schema: Mapping[str, str], strings: Mapping[str, Mapping[str, int]]) -> None:
        self.schema = schema
        self.index = {name: i for i, name in enumerate(schema)}
        self.strings = strings
        self.ops: List[Tuple[int, int, int, int]] = []
        self.sets: List[np.ndarray] = []
        self.n_set = 0

    # -- emission
    def emit(self, op: int, attr: int = 0, a: int = 0, b: int = 0) -> None:
        self.ops.append((op, attr, a, b))

    def false(self) -> None:
        self.emit(TRUE)
        self.emit(NOT)

    def fold(self, parts: List[Any], combine: int, empty_true: bool, fn) -> None:
        if not parts:
            self.emit(TRUE) if empty_true else self.false()
            return
        for i, part in enumerate(parts):
            fn(part)
            if i:
                self.emit(combine)

    # -- filters
    def node(self, where: Any) -> None:
        if not isinstance(where, Mapping):
            raise ValueError(f"a filter is a dict, got {type(where).__name__}")
        self.fold(list(where.items()), AND, True, lambda kv: self.clause(*kv))

    def clause(self, key: Any, value: Any) -> None:
        if key in ("$and", "$or"):
            if not isinstance(value, (list, tuple)):
                raise ValueError(f"{key} takes a list of filters")
            self.fold(list(value), AND if key == "$and" else OR, key == "$and", self.node)
        elif key == "$not":
            self.node(value)
            self.emit(NOT)
        elif isinstance(key, str) and key.startswith("$"):
            raise ValueError(f"unknown combinator {key!r}")
        else:
            if key not in self.schema:
                raise ValueError(f"{key!r} is not a declared attribute of this index (declared: {sorted(self.schema)})")
            if isinstance(value, Mapping):
                if not value:
                    raise ValueError(f"{key!r}: an empty operator dict")
                for op in value:
                    if op not in _FIELD_OPS:
                        raise ValueError(f"{key!r}: unknown operator {op!r}")
                self.fold(list(value.items()), AND, True, lambda kv: self.field(key, *kv))
            else:
                self.field(key, "$eq", value)

    def literal(self, key: str, value: Any) -> int:
        """A scalar literal as the int64 the column holds (int / bool / str code; float bits), or None: matches no row."""
        kind = self.schema[key]
        if is_list(kind):  # an element of the list: typed as the scalar attribute of its element type
            kind = kind[:-2]
        if kind in ("int", "bool"):
            if isinstance(value, (bool, np.bool_)) or (isinstance(value, (int, np.integer))):
                v = int(value)
                if not -(2 ** 63) < v < 2 ** 63:
                    return None  # no stored value can equal it (INT64_MIN is the absent marker)
                return v
            raise ValueError(f"{key!r} is an {kind} attribute: literal {value!r} is not an int or bool")
        if kind == "float":
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
                raise ValueError(f"{key!r} is a float attribute: literal {value!r} is not an int or float")
            return float_bits(float(value))
        if not isinstance(value, str):
            raise ValueError(f"{key!r} is a str attribute: literal {value!r} is not a string")
        return self.strings.get(key, {}).get(value)

    def field(self, key: str, op: str, value: Any) -> None:
        attr, kind = self.index[key], self.schema[key]
        if is_geo(kind) != (op in _GEO_ONLY) and op != "$exists":
            if is_geo(kind):
                raise ValueError(f"{key!r} is a geo attribute: only $geo_radius, $geo_box and $exists apply, {op} does not")
            raise ValueError(f"{key!r} is a {kind} attribute: {op} applies to geo attributes only")
        if op in _GEO_ONLY:
            self.geo_field(key, attr, op, value)
            return
        if is_sparse(kind):
            if op == "$size":
                self.size(key, attr, value)
                return
            if op != "$exists":
                raise ValueError(f"{key!r} is a sparse attribute: only $exists and $size apply (it is searched with "
                                 f"search_sparse, not filtered by value)")
        if is_bits(kind) and op != "$exists":
            raise ValueError(f"{key!r} is a {kind} attribute: only $exists applies (it is searched with search_bits, not "
                             f"filtered by value)")
        if op in _LIST_ONLY and not is_pooled(kind):
            raise ValueError(f"{key!r} is a {kind} attribute: {op} applies to list attributes ({', '.join(LIST_TYPES)}) only")
        if is_list(kind) and op != "$exists":
            self.list_field(key, attr, kind, op, value)
            return
        if op == "$exists":
            if not isinstance(value, (bool, np.bool_)):
                raise ValueError(f"{key!r}: $exists takes True or False")
            self.emit(EXISTS, attr)
            if not value:
                self.emit(NOT)
            return
        if op in ("$in", "$nin"):
            if not isinstance(value, (list, tuple, set, frozenset)):
                raise ValueError(f"{key!r}: {op} takes a list")
            self.member(key, attr, kind, list(value))
            if op == "$nin":
                self.emit(NOT)
            return
        if op in _ORDERED and kind == "str":
            raise ValueError(f"{key!r} is a str attribute: only $eq, $ne, $in, $nin and $exists apply")
        v = self.literal(key, value)
        if kind == "float" and math.isnan(float(value)) and op != "$ne":
            self.false()  # NaN equals / orders against nothing (the ops would say so too; no column read needed)
            return
        if v is None and op in _ORDERED:  # an int literal outside int64: every present value lies on one side of it
            below = (int(value) > 0) == (op in ("$lt", "$lte"))
            self.emit(EXISTS, attr) if below else self.false()
            return
        if v is None:  # a string never ingested, an int outside int64: no row holds it
            self.false() if op != "$ne" else self.emit(TRUE)
            return
        self.emit({"$eq": EQ, "$ne": NE}.get(op) or _ORDERED[op], attr, v)

    # -- geo attributes
    def geo_field(self, key: str, attr: int, op: str, value: Any) -> None:
        names = ("center", "radius") if op == "$geo_radius" else ("sw", "ne")
        if not isinstance(value, Mapping) or set(value) != set(names):
            raise ValueError(f"{key!r}: {op} takes a dict with exactly {names[0]!r} and {names[1]!r}")
        a = geo_pack(value[names[0]], f"{key!r}: {op} {names[0]}")
        if op == "$geo_radius":
            self.emit(GEO_RADIUS, attr, a, float_bits(geo_radius_threshold(value["radius"], f"{key!r}: $geo_radius")))
            return
        b = geo_pack(value["ne"], f"{key!r}: {op} ne")
        if geo_unpack(a)[0] > geo_unpack(b)[0]:
            raise ValueError(f"{key!r}: $geo_box: sw lies north of ne (a box that crosses the antimeridian has sw.lon > ne.lon; "
                             f"its latitudes stay ordered)")
        self.emit(GEO_BOX, attr, a, b)

    # -- list attributes
    def list_set(self, key: str, values: Any, what: str) -> List[Any]:
        if not isinstance(values, (list, tuple, set, frozenset)):
            raise ValueError(f"{key!r}: {what} takes a list")
        return [self.literal(key, x) for x in values]

    def emit_set(self, op: int, attr: int, codes) -> None:
        vals = np.unique(np.array(list(codes), dtype=np.int64))
        self.emit(op, attr, self.n_set, int(vals.size))
        self.sets.append(vals)
        self.n_set += int(vals.size)

    def list_field(self, key: str, attr: int, kind: str, op: str, value: Any) -> None:
        if op in _ORDERED:
            raise ValueError(f"{key!r} is a {kind} attribute: $eq, $ne, $in, $nin, $all, $size and $exists apply, {op} does not")
        if op in ("$eq", "$ne"):
            v = self.literal(key, value)
            self.false() if v is None else self.emit(HAS, attr, v)  # (a value no list can hold is in none)
            if op == "$ne":
                self.emit(NOT)
        elif op in ("$in", "$nin"):
            seen = [v for v in self.list_set(key, value, op) if v is not None]
            self.emit_set(HAS_ANY, attr, seen) if seen else self.false()
            if op == "$nin":
                self.emit(NOT)
        elif op == "$all":
            lits = self.list_set(key, value, op)
            if not lits:
                raise ValueError(f"{key!r}: $all takes a list that is not empty")
            if any(v is None for v in lits) or len(set(lits)) > LIST_MAX_LEN:
                self.false()  # one of them is in no list (or they are more than a list holds): the clause is false
            else:
                self.emit_set(HAS_ALL, attr, lits)
        else:
            self.size(key, attr, value)

    def size(self, key: str, attr: int, value: Any) -> None:
        """``$size``: an int, or a dict of ``$eq $lt $lte $gt $gte`` over ints -> one LEN lo hi."""
        def integer(x):
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                raise ValueError(f"{key!r}: $size takes an int or a dict of $eq / $lt / $lte / $gt / $gte over ints (got {x!r})")
            return int(x)
        lo, hi = 0, LIST_MAX_LEN
        if isinstance(value, Mapping):
            if not value:
                raise ValueError(f"{key!r}: $size: an empty operator dict")
            for op, x in value.items():
                if op != "$eq" and op not in _ORDERED:
                    raise ValueError(f"{key!r}: $size: unknown operator {op!r}")
                x = integer(x)
                if op in ("$eq", "$gte", "$gt"):
                    lo = max(lo, x + (op == "$gt"))
                if op in ("$eq", "$lte", "$lt"):
                    hi = min(hi, x - (op == "$lt"))
        else:
            lo = hi = integer(value)
        self.emit(LEN, attr, lo, hi) if 0 <= lo <= hi <= LIST_MAX_LEN else self.false()

    def member(self, key: str, attr: int, kind: str, values: List[Any]) -> None:
        lits = [self.literal(key, x) for x in values]
        if kind == "float":  # IN reads int64 columns: a float membership is an OR of equalities
            lits = [v for v, x in zip(lits, values) if not math.isnan(float(x))]
            self.fold(sorted(set(lits)), OR, False, lambda v: self.emit(EQ, attr, v))
            return
        vals = np.unique(np.array([v for v in lits if v is not None], dtype=np.int64))
        if vals.size == 0:
            self.false()
            return
        self.emit(IN, attr, self.n_set, int(vals.size))
        self.sets.append(vals)
        self.n_set += int(vals.size)

    def program(self) -> Program:
        if len(self.ops) > MAX_OPS:
            raise ValueError(f"the filter compiles to {len(self.ops)} ops; the device evaluates at most {MAX_OPS}")
        depth = deepest = 0
        for op, _, _, _ in self.ops:
            depth += -1 if op in (AND, OR) else 0 if op == NOT else 1
            deepest = max(deepest, depth)
        if deepest > MAX_DEPTH:
            raise ValueError(f"the filter needs a stack {deepest} deep; the device evaluates at most {MAX_DEPTH}")
        table = np.concatenate(self.sets) if self.sets else np.zeros(0, dtype=np.int64)  # each IN range sorted by itself
        return Program(np.array(self.ops, dtype=OP_DTYPE), np.ascontiguousarray(table, dtype=np.int64))


def compile_where(where: Mapping[str, Any], schema: Mapping[str, str],
                  strings: Mapping[str, Mapping[str, int]] | None = None) -> Program:
    """Compile ``where`` against ``schema`` (attribute name -> "int" / "float" / "str" / "bool", in declaration order:
    attribute i is column i) and the namespace's string dictionaries (attribute -> {string: code})."""
    b = _Builder(schema, strings or {})
    b.node(where)
    return b.program()


# ---------------------------------------------------------------- per-query filters (include/mlvdb_where_each.h)
EACH_MAX_PROGRAMS = 64  # MLVDB_WHERE_EACH_MAX_PROGRAMS: distinct programs per native call
EACH_MAX_OPS = 1024     # MLVDB_WHERE_EACH_MAX_OPS: ops over all programs of one native call


def _program_key(program: Program) -> Tuple[bytes, bytes]:
    return program.ops.tobytes(), np.ascontiguousarray(program.set, dtype=np.int64).tobytes()


def compile_each(wheres, schema: Mapping[str, str],
                 strings: Mapping[str, Mapping[str, int]] | None = None) -> Tuple[List[Program], np.ndarray]:
    """Per-query filters: ``wheres[i]`` is a dict filter or ``None`` (unfiltered) -> (the distinct compiled programs,
    ``program_of_query`` int32 [len(wheres)]: an index into them or -1).  Filters that compile to the same program (same
    ops and set table) share one entry, so a batch of many queries over few tenants scans the columns for few programs."""
    programs: List[Program] = []
    seen: Dict[Tuple[bytes, bytes], int] = {}
    of = np.full(len(wheres), -1, dtype=np.int32)
    for i, w in enumerate(wheres):
        if w is None:
            continue
        prog = compile_where(w, schema, strings)
        key = _program_key(prog)
        j = seen.get(key)
        if j is None:
            j = seen[key] = len(programs)
            programs.append(prog)
        of[i] = j
    return programs, of


def chunk_programs(programs: List[Program], program_of_query, max_programs: int = EACH_MAX_PROGRAMS,
                   max_ops: int = EACH_MAX_OPS) -> List[Tuple[np.ndarray, List[Program], np.ndarray]]:
    """Split per-query programs into native calls within the per-call limits: a list of (query indices, the call's
    programs, the call's ``program_of_query`` for those queries).  Programs are taken in order; every call holds at most
    ``max_programs`` of them and ``max_ops`` ops in all.  The unfiltered queries (-1) ride with the first call (a call of
    their own when there is no program).  Queries keep their batch order inside each call."""
    of = np.asarray(program_of_query, dtype=np.int32)
    groups: List[List[int]] = []
    ops = 0
    for j, prog in enumerate(programs):
        n = int(prog.ops.size)
        if n > max_ops:
            raise ValueError(f"a filter compiles to {n} ops; one call evaluates at most {max_ops}")
        if not groups or len(groups[-1]) >= max_programs or ops + n > max_ops:
            groups.append([])
            ops = 0
        groups[-1].append(j)
        ops += n
    if not groups:
        groups.append([])
    out = []
    for c, members in enumerate(groups):
        local = np.full(len(programs) + 1, -1, dtype=np.int32)  # (slot len(programs): the unfiltered queries' -1)
        local[members] = np.arange(len(members), dtype=np.int32)
        take = np.isin(of, members) | ((of < 0) if c == 0 else False)
        idx = np.flatnonzero(take)
        sub = of[idx]
        out.append((idx, [programs[j] for j in members], local[np.where(sub >= 0, sub, len(programs))]))
    return out


# ---------------------------------------------------------------- ingest: metadata values -> column values
INT64_ABSENT = np.iinfo(np.int64).min


@dataclass
class ListColumn:
    """A batch of a list attribute in CSR form, as ``mlvdb_attr_list_set`` takes it: row i holds
    ``values[offsets[i]:offsets[i + 1]]`` (strictly ascending) when ``present[i]``, and no list at all otherwise."""

    offsets: np.ndarray  # int64 [n + 1], offsets[0] == 0
    values: np.ndarray   # int64
    present: np.ndarray  # uint8 [n]

    def __len__(self) -> int:
        return int(self.present.size)

    def row(self, i: int):
        """The codes of row i as a list, or ``None``."""
        return self.values[self.offsets[i]:self.offsets[i + 1]].tolist() if self.present[i] else None

    def take(self, rows) -> "ListColumn":
        """The rows ``rows`` (indices, in that order) as a column of their own."""
        rows = np.asarray(rows, dtype=np.int64)
        lens = (self.offsets[1:] - self.offsets[:-1])[rows]
        offsets = np.zeros(rows.size + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        parts = [self.values[self.offsets[r]:self.offsets[r + 1]] for r in rows.tolist()]
        values = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        return ListColumn(offsets, np.ascontiguousarray(values, dtype=np.int64), self.present[rows].copy())


def encode_list_column(name: str, kind: str, values, codes: Dict[str, int]) -> ListColumn:
    """One list attribute's values of a batch -> ``ListColumn``.  A value is a list, tuple or set of str (``"str[]"``) or
    int (``"int[]"``): ``None`` = absent, ``[]`` = an empty list (present), duplicates collapse, the codes are sorted.
    More than 255 distinct elements, an element of the wrong type or a bare scalar raise ``ValueError`` naming the
    attribute.  New strings get codes in ``codes`` (a copy of the caller's, kept only if the whole batch is accepted)."""
    n = len(values)
    offsets = np.zeros(n + 1, dtype=np.int64)
    present = np.zeros(n, dtype=np.uint8)
    parts: List[List[int]] = []
    for i, v in enumerate(values):
        row: List[int] = []
        if v is not None:
            if not isinstance(v, (list, tuple, set, frozenset)):
                raise ValueError(f"attribute {name!r} ({kind}): row {i} holds {v!r}, not a list, tuple or set")
            seen = set()
            for x in v:
                if kind == "str[]":
                    if not isinstance(x, str):
                        raise ValueError(f"attribute {name!r} ({kind}): row {i} holds the element {x!r}")
                    code = codes.get(x)
                    if code is None:
                        code = codes[x] = len(codes)
                else:
                    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                        raise ValueError(f"attribute {name!r} ({kind}): row {i} holds the element {x!r}")
                    code = int(x)
                    if not -(2 ** 63) < code < 2 ** 63:
                        raise ValueError(f"attribute {name!r} ({kind}): row {i} holds {x!r}, outside int64 "
                                         f"(INT64_MIN marks absent)")
                seen.add(code)
            if len(seen) > LIST_MAX_LEN:
                raise ValueError(f"attribute {name!r} ({kind}): row {i} holds {len(seen)} distinct elements; a list holds "
                                 f"at most {LIST_MAX_LEN}")
            row = sorted(seen)
            present[i] = 1
        parts.append(row)
        offsets[i + 1] = offsets[i] + len(row)
    flat = np.array([c for row in parts for c in row], dtype=np.int64)
    return ListColumn(offsets, flat, present)


@dataclass
class SparseColumn:
    """A batch of a sparse attribute in CSR form, as ``mlvdb_sparse_set`` takes it: row i holds the pairs
    ``(terms[j], weights[j])`` for j in ``offsets[i]:offsets[i + 1]`` (terms strictly ascending) when ``present[i]``, and
    no vector at all otherwise."""

    offsets: np.ndarray  # int64 [n + 1], offsets[0] == 0
    terms: np.ndarray    # int32
    weights: np.ndarray  # float32
    present: np.ndarray  # uint8 [n]

    def __len__(self) -> int:
        return int(self.present.size)

    def row(self, i: int):
        """Row i as a dict term -> weight, or ``None``."""
        if not self.present[i]:
            return None
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        return dict(zip(self.terms[lo:hi].tolist(), self.weights[lo:hi].tolist()))

    def take(self, rows) -> "SparseColumn":
        """The rows ``rows`` (indices, in that order) as a column of their own."""
        rows = np.asarray(rows, dtype=np.int64)
        lens = (self.offsets[1:] - self.offsets[:-1])[rows]
        offsets = np.zeros(rows.size + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        pick = [np.arange(self.offsets[r], self.offsets[r + 1]) for r in rows.tolist()]
        pick = np.concatenate(pick).astype(np.int64) if pick else np.zeros(0, dtype=np.int64)
        return SparseColumn(offsets, np.ascontiguousarray(self.terms[pick], dtype=np.int32),
                            np.ascontiguousarray(self.weights[pick], dtype=np.float32), self.present[rows].copy())


def encode_sparse_vector(value, what: str, max_nnz: int = SPARSE_MAX_NNZ) -> Tuple[List[int], List[float]]:
    """One sparse vector -- a mapping ``{term: weight}`` or a pair ``(indices, values)`` -- as (terms ascending, weights):
    explicit zero weights are dropped.  ``ValueError`` (starting with ``what``) for a duplicate term, a term that is not an
    integer in [0, 2^31), a weight that is not a finite float32, or more than ``max_nnz`` nonzeros."""
    if isinstance(value, Mapping):
        pairs = list(value.items())
    else:
        try:
            indices, values = value
            indices = indices.tolist() if isinstance(indices, np.ndarray) else list(indices)
            values = values.tolist() if isinstance(values, np.ndarray) else list(values)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: {value!r} is not a mapping term -> weight or a pair (indices, values)") from None
        if len(indices) != len(values):
            raise ValueError(f"{what}: {len(indices)} indices but {len(values)} values")
        pairs = list(zip(indices, values))
    seen: Dict[int, float] = {}
    for t, w in pairs:
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
            raise ValueError(f"{what}: term {t!r} is not an integer")
        t = int(t)
        if not 0 <= t < 2 ** 31:
            raise ValueError(f"{what}: term {t} is outside [0, 2^31)")
        if t in seen:
            raise ValueError(f"{what}: term {t} appears twice")
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what}: the weight {w!r} of term {t} is not a number")
        with np.errstate(over="ignore"):
            w32 = float(np.float32(w))
        if not math.isfinite(w32):
            raise ValueError(f"{what}: the weight {w!r} of term {t} is not a finite float32")
        seen[t] = w32
    kept = sorted((t, w) for t, w in seen.items() if w != 0.0)
    if len(kept) > max_nnz:
        raise ValueError(f"{what}: {len(kept)} nonzeros; a sparse vector holds at most {max_nnz}")
    return [t for t, _ in kept], [w for _, w in kept]


def encode_sparse_column(name: str, values, max_nnz: int = SPARSE_MAX_NNZ) -> SparseColumn:
    """One sparse attribute's values of a batch -> ``SparseColumn``.  A value is a mapping ``{term: weight}`` or a pair
    ``(indices, values)``; ``None`` = absent, ``{}`` = an empty vector (present).  See ``encode_sparse_vector`` for what is
    dropped, sorted and refused; the whole batch is checked before anything is returned."""
    n = len(values)
    offsets = np.zeros(n + 1, dtype=np.int64)
    present = np.zeros(n, dtype=np.uint8)
    terms: List[int] = []
    weights: List[float] = []
    for i, v in enumerate(values):
        if v is not None:
            t, w = encode_sparse_vector(v, f"attribute {name!r} (sparse): row {i}", max_nnz)
            terms.extend(t)
            weights.extend(w)
            present[i] = 1
        offsets[i + 1] = len(terms)
    return SparseColumn(offsets, np.array(terms, dtype=np.int32), np.array(weights, dtype=np.float32), present)


@dataclass
class BitsColumn:
    """A batch of a bits attribute, as ``mlvdb_bits_set`` takes it: row i holds the code ``words[i]`` (word w = bits
    64w .. 64w + 63) when ``present[i]``, and no code at all otherwise (its words are then zero and ignored)."""

    words: np.ndarray    # uint64 [n, N / 64]
    present: np.ndarray  # uint8 [n]

    def __len__(self) -> int:
        return int(self.present.size)

    def row(self, i: int):
        """Row i's code as ``N / 8`` bytes (little-endian words), or ``None``."""
        return self.words[i].astype("<u8").tobytes() if self.present[i] else None

    def take(self, rows) -> "BitsColumn":
        """The rows ``rows`` (indices, in that order) as a column of their own."""
        rows = np.asarray(rows, dtype=np.int64)
        return BitsColumn(np.ascontiguousarray(self.words[rows]), self.present[rows].copy())


def encode_bits_code(value, nbits: int, what: str) -> np.ndarray:
    """One ``nbits``-bit code as ``nbits / 64`` uint64 words (word w = bits 64w .. 64w + 63).  ``value`` is ``bytes`` of
    ``nbits / 8`` bytes read as little-endian 64-bit words, a ``uint8`` array of ``nbits / 8`` entries read the same way, or
    a bool / 0-1 array (or list) of ``nbits`` entries, entry b being bit b.  ``ValueError`` (starting with ``what``) for
    anything else: a wrong length, a wrong dtype, an entry that is neither 0 nor 1."""
    if isinstance(value, (bytes, bytearray, memoryview)):
        raw = bytes(value)
        if len(raw) != nbits // 8:
            raise ValueError(f"{what}: {len(raw)} bytes; a {nbits}-bit code is {nbits // 8} bytes")
        return np.frombuffer(raw, dtype="<u8").astype(np.uint64)
    if isinstance(value, (str, Mapping)) or value is None:
        raise ValueError(f"{what}: {value!r} is not a bit code (bytes, a uint8 array of {nbits // 8} entries or a bool / 0-1 "
                         f"array of {nbits} entries)")
    try:
        arr = np.asarray(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {value!r} is not a bit code") from None
    if arr.ndim != 1 or arr.dtype.kind not in "bui":
        raise ValueError(f"{what}: an array of shape {arr.shape} and dtype {arr.dtype}; a bit code is a 1-d uint8 array of "
                         f"{nbits // 8} entries or a 1-d bool / 0-1 array of {nbits} entries")
    if arr.dtype == np.uint8 and arr.size == nbits // 8:
        return np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype="<u8").astype(np.uint64)
    if arr.size != nbits:
        raise ValueError(f"{what}: {arr.size} entries; a {nbits}-bit code is {nbits} bits (or {nbits // 8} uint8 bytes)")
    if arr.dtype.kind != "b" and ((arr != 0) & (arr != 1)).any():
        raise ValueError(f"{what}: a bit array holds 0 and 1 only")
    packed = np.packbits(arr.astype(bool), bitorder="little")
    return np.frombuffer(packed.tobytes(), dtype="<u8").astype(np.uint64)


def encode_bits_column(name: str, kind: str, values) -> BitsColumn:
    """One bits attribute's values of a batch -> ``BitsColumn``.  ``None`` = absent; see ``encode_bits_code`` for the forms a
    code comes in and what is refused; the whole batch is checked before anything is returned."""
    nbits = bits_width(kind)
    n = len(values)
    words = np.zeros((n, nbits // 64), dtype=np.uint64)
    present = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        v = values[i]
        if v is not None:
            words[i] = encode_bits_code(v, nbits, f"attribute {name!r} ({kind}): row {i}")
            present[i] = 1
    return BitsColumn(words, present)


def encode_column(name: str, kind: str, values, codes: Dict[str, int]) -> np.ndarray:
    """One attribute's values of a batch (``None`` = absent) as the device column (int64 with INT64_MIN absent, float64
    with NaN absent).  New strings get codes in ``codes`` (the caller passes a copy and keeps it only if the whole batch
    is accepted).  A value of the wrong type raises ``ValueError`` naming the attribute.  A geo attribute's values are
    points (``geo_pack``), packed into int64."""
    if is_geo(kind):
        out = np.full(len(values), INT64_ABSENT, dtype=np.int64)
        for i, v in enumerate(values.tolist() if isinstance(values, np.ndarray) else values):
            if v is not None:
                out[i] = geo_pack(v, f"attribute {name!r} (geo): row {i}")
        return out
    if isinstance(values, np.ndarray) and values.dtype != object:
        return _encode_array(name, kind, values, codes)
    n = len(values)
    if kind == "float":
        out = np.full(n, np.nan)
        for i, v in enumerate(values):
            if v is None:
                continue
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"attribute {name!r} (float): row {i} holds {v!r}")
            out[i] = float(v)
        return out
    out = np.full(n, INT64_ABSENT, dtype=np.int64)
    for i, v in enumerate(values):
        if v is None:
            continue
        if kind == "str":
            if not isinstance(v, str):
                raise ValueError(f"attribute {name!r} (str): row {i} holds {v!r}")
            code = codes.get(v)
            if code is None:
                code = codes[v] = len(codes)
            out[i] = code
        elif kind == "bool":
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"attribute {name!r} (bool): row {i} holds {v!r}")
            out[i] = int(v)
        else:
            if not isinstance(v, (int, np.integer)):  # (bool is an int)
                raise ValueError(f"attribute {name!r} (int): row {i} holds {v!r}")
            if not -(2 ** 63) < int(v) < 2 ** 63:
                raise ValueError(f"attribute {name!r} (int): row {i} holds {v!r}, outside int64 (INT64_MIN marks absent)")
            out[i] = int(v)
    return out


def _encode_array(name: str, kind: str, values: np.ndarray, codes: Dict[str, int]) -> np.ndarray:
    values = values.ravel()
    ch = values.dtype.kind
    if kind == "float":
        if ch not in "iuf":
            raise ValueError(f"attribute {name!r} (float): array of dtype {values.dtype}")
        return values.astype(np.float64)
    if kind == "str":
        if ch not in "US":
            raise ValueError(f"attribute {name!r} (str): array of dtype {values.dtype}")
        return encode_column(name, kind, values.astype(str).tolist(), codes)
    if kind == "bool" and ch != "b":
        raise ValueError(f"attribute {name!r} (bool): array of dtype {values.dtype}")
    if kind == "int" and ch not in "iub":
        raise ValueError(f"attribute {name!r} (int): array of dtype {values.dtype}")
    if ch == "u" and values.size and values.max() > np.iinfo(np.int64).max:
        raise ValueError(f"attribute {name!r} (int): values outside int64")
    out = values.astype(np.int64)
    if (out == INT64_ABSENT).any():
        raise ValueError(f"attribute {name!r} (int): INT64_MIN is the absent marker, not a value")
    return out
