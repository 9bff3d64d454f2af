"""NumPy oracle of the geo attributes (include/mlvdb_geo.h), shared by tests/test_geo_host.py and tests/test_gpu_geo.py.

The distance is the header's definition evaluated in np.longdouble from the integer coordinates:

    dphi = (lat - lat_c) K,  dlam = wrap(lon - lon_c) K,  K = pi / (180 * 1e7),  differences taken in integers first
    hav  = sin^2(dphi / 2) + cos(lat_c K) cos(lat K) sin^2(dlam / 2),   d = 2 R asin(sqrt(min(hav, 1)))

Box tests are integer tests and are compared bit for bit.  Radius membership and distance order can differ from the device
only where two fp64 evaluations round apart, so the two guards below are ASSERTED on the CPU before any device call (nothing is
filtered, no row is set aside; a seed that trips one is replaced by another seed, G is never relaxed):

    radius guard   no candidate has |d - r| <= G max(r, 1 m)   (rows with d == 0 under r == 0 are exact, and exempt)
    rank guard     among the oracle's ranks [0, min(4097, candidates)) any two rows with different coordinates differ in d by
                   more than G d
    G = 1e-10      about 5,000 x the fp64 rounding it covers (a plain NumPy fp64 evaluation deviates from the long double
                   one by ~2e-14 relative), 100 x below the smallest gaps random data shows

Returned distances are compared with the long double oracle under a relative tolerance of 16 x the largest deviation of a
plain NumPy fp64 evaluation of the same formula from it, measured over the test's own inputs (`fp64_deviation`; the factor
covers a device libm a few ulp per call away from glibc over the five transcendental calls).  A parametrised test whose
cases are prefixes of one pool of points measures it over the pool: a sample of one row is no estimate of a rounding error.
"""
import numpy as np

from mlvectordb_amd import where as W

R = 6371008.8
G = 1e-10
ABSENT = np.iinfo(np.int64).min
LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")
MAX_ROWS = 4096
TURN = 3_600_000_000


def pack(lat_e7, lon_e7):
    """int arrays of 1e-7 degree -> the int64 column values."""
    return (np.asarray(lat_e7, dtype=np.int64) << 32) | (np.asarray(lon_e7, dtype=np.int64) & 0xFFFFFFFF)


def unpack(col):
    """int64 column values -> (lat_e7, lon_e7) as int64 arrays (the low half sign-extended)."""
    col = np.asarray(col, dtype=np.int64)
    return col >> 32, ((col & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000


def quantise(lat_deg, lon_deg):
    """Degrees -> column values, as where.geo_pack quantises one point."""
    return pack(np.rint(np.asarray(lat_deg, dtype=np.float64) * 1e7).astype(np.int64),
                np.rint(np.asarray(lon_deg, dtype=np.float64) * 1e7).astype(np.int64))


def hav(points, centre, dtype=LD):
    """hav of every value of `points` (present ones) from the packed point `centre`, in `dtype`."""
    lat, lon = unpack(points)
    lat_c, lon_c = unpack(np.int64(centre))
    dlat = lat - lat_c
    dlon = lon - lon_c
    dlon = np.where(dlon >= TURN // 2, dlon - TURN, dlon)
    dlon = np.where(dlon < -TURN // 2, dlon + TURN, dlon)
    k = (PI_LD if dtype is LD else dtype(np.pi)) / dtype(180.0 * 1e7)
    sp = np.sin(dlat.astype(dtype) * k / dtype(2))
    sl = np.sin(dlon.astype(dtype) * k / dtype(2))
    return sp * sp + np.cos(dtype(int(lat_c)) * k) * np.cos(lat.astype(dtype) * k) * (sl * sl)


def metres(h):
    dtype = h.dtype.type
    return dtype(2) * dtype(R) * np.arcsin(np.sqrt(np.minimum(h, dtype(1))))


def dist(points, centre, dtype=LD):
    return metres(hav(points, centre, dtype))


def fp64_deviation(points, centres):
    """The largest relative deviation of a plain NumPy fp64 evaluation of d from the long double one over the present
    `points` and the packed `centres` (rows at d == 0 are exact in both and are left out)."""
    points = np.asarray(points, dtype=np.int64)
    points = points[points != ABSENT]
    worst = 0.0
    for c in centres:
        want = dist(points, c)
        got = dist(points, c, np.float64)
        assert np.array_equal(got == 0, want == 0)
        nz = want > 0
        if nz.any():
            worst = max(worst, float(np.max(np.abs(got[nz].astype(LD) - want[nz]) / want[nz])))
    return worst


# ---------------------------------------------------------------- filters
def radius_mask(col, centre, radius, h=None):
    """Rows of `col` inside the circle (absent rows never), after the radius guard over every row that holds a point.
    `h`: hav(col, centre) when the caller has it already (whatever it holds at absent rows)."""
    col = np.asarray(col, dtype=np.int64)
    have = col != ABSENT
    out = np.zeros(col.size, dtype=bool)
    d = metres(hav(col[have], centre) if h is None else h[have])  # (r >= pi R: every d <= r, the threshold is clamped to 1)
    near = np.abs(d - LD(radius)) <= LD(G) * max(LD(radius), LD(1))
    if radius == 0:
        near &= d != 0
    assert not near.any(), f"radius guard: {int(near.sum())} candidates within G of r = {radius} m (choose another seed)"
    out[have] = d <= LD(radius)
    return out


def box_mask(col, sw, ne):
    """Rows of `col` inside the box of the packed corners (inclusive; lon_sw > lon_ne: across the antimeridian)."""
    col = np.asarray(col, dtype=np.int64)
    lat, lon = unpack(col)
    (s, w), (n, e) = unpack(np.int64(sw)), unpack(np.int64(ne))
    in_lon = ((lon >= w) & (lon <= e)) if w <= e else ((lon >= w) | (lon <= e))
    return (col != ABSENT) & (lat >= s) & (lat <= n) & in_lon


def radius_program(attr, centre, radius):
    return W.Program(np.array([(W.GEO_RADIUS, attr, int(centre), W.float_bits(W.geo_radius_threshold(radius)))], W.OP_DTYPE),
                     np.zeros(0, np.int64))


def box_program(attr, sw, ne):
    return W.Program(np.array([(W.GEO_BOX, attr, int(sw), int(ne))], W.OP_DTYPE), np.zeros(0, np.int64))


def negate(program):
    return W.Program(np.concatenate([program.ops, np.array([(W.NOT, 0, 0, 0)], W.OP_DTYPE)]), program.set)


# ---------------------------------------------------------------- nearest
def nearest_oracle(col, mask, centre, h=None):
    """The ranking of the rows of `mask` (live and matching) that hold a point, by (hav, label), after the rank guard:
    (labels int64 of the first min(4096, candidates) ranks, their distances in long double, matched, absent).
    `h`: hav(col, centre) when the caller has it already (whatever it holds at absent rows)."""
    col = np.asarray(col, dtype=np.int64)
    matched = int(mask.sum())
    labels = np.flatnonzero(mask & (col != ABSENT))
    absent = matched - int(labels.size)
    h = hav(col[labels], centre) if h is None else h[labels]
    if labels.size > 4 * (MAX_ROWS + 1):  # only the first 4097 ranks are needed: cut at their hav before sorting
        keep = h <= np.partition(h, MAX_ROWS)[MAX_ROWS]
        labels, h = labels[keep], h[keep]
    order = np.lexsort((labels, h))[:MAX_ROWS + 1]
    top = labels[order]
    d = metres(h[order])
    other = col[top][1:] != col[top][:-1]
    close = other & ~(d[1:] - d[:-1] > LD(G) * d[1:])
    assert not close.any(), f"rank guard: {int(close.sum())} neighbouring ranks within G of each other (choose another seed)"
    return top[:MAX_ROWS], d[:MAX_ROWS], matched, absent


# ---------------------------------------------------------------- data
def random_points(rng, n, centre_deg, absent=0.1, sigma=0.2):
    """n column values: half in a cluster of `sigma` degrees around `centre_deg`, the rest uniform on the sphere; a share
    `absent` of them absent."""
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, n)))
    lon = rng.uniform(-180, 180, n)
    near = rng.random(n) < 0.5
    lat = np.where(near, np.clip(centre_deg[0] + sigma * rng.standard_normal(n), -90, 90), lat)
    lon = np.where(near, (centre_deg[1] + sigma * rng.standard_normal(n) + 180) % 360 - 180, lon)
    col = quantise(lat, lon)
    col[rng.random(n) < absent] = ABSENT
    return col


# ---------------------------------------------------------------- a host engine for the Index-level tests without a device
def eval_program(program, cols, n):
    """where_helpers.eval_program with the two geo ops.  GEO_RADIUS compares the long double hav with the op's threshold, as
    the device compares its fp64 one (no guard here: this serves the host model, whose inputs the tests choose well apart)."""
    from tests import where_helpers

    stack = []
    for row in program.ops:
        op, attr, a, b = row.tolist()
        if op in (W.AND, W.OR):
            y, x = stack.pop(), stack.pop()
            stack.append(x & y if op == W.AND else x | y)
        elif op == W.NOT:
            stack.append(~stack.pop())
        elif op == W.GEO_BOX:
            stack.append(box_mask(cols[attr], a, b))
        elif op == W.GEO_RADIUS:
            have = cols[attr] != ABSENT
            bit = np.zeros(n, dtype=bool)
            bit[have] = hav(cols[attr][have], a) <= LD(np.array([b], dtype=np.int64).view(np.float64)[0])
            stack.append(bit)
        else:
            stack.append(where_helpers.eval_program(W.Program(np.array([row], W.OP_DTYPE), program.set), cols, n))
    assert len(stack) == 1
    return stack[0]


def oracle_engine_class():
    """``MutateOracleEngine`` + the geo ops in its filters + ``geo_nearest`` (built on demand: the import pulls the oracle in)."""
    from tests.mutate_helpers import MutateOracleEngine

    class GeoOracleEngine(MutateOracleEngine):
        def match(self, program):
            return eval_program(program, self._cols, self._rows.shape[0]) & ~self._deleted

        def geo_nearest(self, attr, center, limit, where=None, offset=0):
            mask = ~self._deleted if where is None else self.match(where)
            top, d, matched, absent = nearest_oracle(self._cols[attr], mask, center)
            top, d = top[offset:offset + limit], d[offset:offset + limit]
            return top.astype(np.int64), self._cols[attr][top], d.astype(np.float64), matched, absent

    return GeoOracleEngine
