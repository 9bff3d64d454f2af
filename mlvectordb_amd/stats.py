"""The host side of attribute statistics (include/mlvdb_stats.h): the 128-bit sums of ``HipScanEngine.attr_stats`` turned
into Python numbers, and the same arithmetic over plain Python values for the callers that aggregate on the host
(``QueryProcessor.stats`` with a predicate), so that both paths return equal values.

An int column's sum is exact.  A float column's sum is the fixed-point sum of the header: with ``m`` the largest finite
magnitude of the group and ``E = floor(log2 m)``, ``S = sum(rint(v * 2**(61 - E)))`` over the finite values, half to even,
and the answer is ``S * 2**(E - 61)`` rounded once -- a function of the set of values, whatever their order."""
from __future__ import annotations

import math
import struct
from typing import Iterable, Optional, Tuple

_SCALE = 61


def int128(hi: int, lo: int) -> int:
    """The signed 128-bit integer ``hi:lo`` (hi int64, lo uint64)."""
    return (int(hi) << 64) + int(lo)


def split128(value: int) -> Tuple[int, int]:
    """``value`` as (hi int64, lo uint64), two's complement."""
    return value >> 64, value & (2 ** 64 - 1)


def total_order_key(v: float) -> int:
    """An integer that orders doubles as IEEE totalOrder does: -0.0 below +0.0, the infinities at the ends."""
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    return bits ^ (2 ** 64 - 1) if bits >> 63 else bits | (1 << 63)


def fixed_exponent(lo: float, hi: float) -> Optional[int]:
    """``E`` of a group from its least and greatest value, or ``None`` when its fixed-point sum is 0 by definition (an
    infinity in the group, or nothing but zeros)."""
    m = max(abs(lo), abs(hi))
    if math.isinf(m) or m == 0.0:
        return None
    return math.frexp(m)[1] - 1  # m = f * 2**e with 0.5 <= f < 1, subnormals included


def fixed_term(v: float, exponent: int) -> int:
    """``rint(v * 2**(61 - E))``: the scaling is exact (or lands below 1/2, which rounds to 0 either way)."""
    return int(round(math.ldexp(v, _SCALE - exponent)))  # round(): half to even, to an int


def float_sum(fixed: int, lo: float, hi: float) -> float:
    """The sum of a float group from its fixed-point sum and its least and greatest value."""
    if math.isinf(lo) or math.isinf(hi):
        return math.nan if (lo == -math.inf and hi == math.inf) else (lo if math.isinf(lo) else hi)
    e = fixed_exponent(lo, hi)
    if e is None or fixed == 0:
        return 0.0
    try:
        # float(int) rounds half to even; whatever ldexp could round again (a subnormal result) is a multiple of 2**-1074
        # with at most 52 bits and was exact already
        return math.ldexp(float(fixed), e - _SCALE)
    except OverflowError:
        return math.copysign(math.inf, fixed)


def float_group(values: Iterable[float]):
    """(count, min, max, fixed-point sum) of the non-NaN ``values`` by the rule above -- what the device returns for them;
    ``min`` / ``max`` are ``None`` for an empty group."""
    present = [float(v) for v in values if v == v]
    if not present:
        return 0, None, None, 0
    lo, hi = min(present, key=total_order_key), max(present, key=total_order_key)
    e = fixed_exponent(lo, hi)
    fixed = 0 if e is None else sum(fixed_term(v, e) for v in present)
    return len(present), lo, hi, fixed


def summary(kind: str, count: int, lo, hi, total: int) -> dict:
    """{"count", "min", "max", "sum", "mean"} of one group of a declared ``int`` / ``float`` / ``bool`` attribute:
    ``total`` is the exact sum (int, bool) or the fixed-point sum (float)."""
    if count == 0:
        return {"count": 0, "min": None, "max": None, "sum": 0, "mean": None}
    if kind == "float":
        s = float_sum(total, float(lo), float(hi))
        return {"count": count, "min": float(lo), "max": float(hi), "sum": s, "mean": s / count}
    cast = bool if kind == "bool" else int
    return {"count": count, "min": cast(lo), "max": cast(hi), "sum": int(total), "mean": int(total) / count}
