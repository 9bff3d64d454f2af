"""mlvdb_range_batch_bits on the MI355X against the model of tests/bits_range_helpers.py: labels, counts, offsets and the 64
bits of every distance, no tolerance.  The corpora are those of tests/test_gpu_bits.py (ties at the radius are the rule)."""
from types import SimpleNamespace

import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.bits_helpers import METRICS, BitsOracleEngine, distances
from tests.bits_range_helpers import MAX_HITS, range_bits
from tests.test_gpu_bits import BT, INT, FLT, D, N, WIDTHS, Pair, column, prog

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, OVERFLOW = 0, 1, 6, 7  # include/mlvdb_hip.h
TILE = 32  # kBitsRangeQT


def raw(eng, queries, metric, radius, capacity=MAX_HITS, total=0, where=None, attr=BT, words=None, arrays=True, nq=None,
        offsets=True):
    """One mlvdb_range_batch_bits call -> (status, labels, dist, dist64, offsets, counts); the outputs are pre-filled with -7."""
    queries = np.ascontiguousarray(queries, dtype=np.uint64)
    nq = queries.shape[0] if nq is None else nq
    lab, d32, d64 = np.full(max(total, 1), -7, np.int64), np.full(max(total, 1), -7, np.float32), np.full(max(total, 1), -7.0)
    off, cnt = np.full(max(nq, 0) + 1, -7, np.int64), np.full(max(nq, 1), -7, np.int64)
    w, keep = HipScanEngine._where_arg(where)
    ptr = lambda a: a.ctypes.data if arrays else None
    rc = _native.load().mlvdb_range_batch_bits(
        eng.handle, attr, queries.ctypes.data, nq, queries.shape[1] if words is None else words,
        metric if isinstance(metric, int) else _native.BITS_METRIC_CODES[metric], float(radius), capacity, total, w, ptr(lab),
        ptr(d32), ptr(d64), off.ctypes.data if offsets else None, cnt.ctypes.data)
    return rc, lab[:total], d32[:total], d64[:total], off, cnt[:max(nq, 0)]


def check(p, queries, metric, radius, capacity=MAX_HITS, where=None, tag=""):
    """The call with exactly the entries it needs against the model; returns the model's (labels, dist64, offsets, counts)."""
    want = labels, w64, offsets, counts = range_bits(p.model, BT, queries, radius, metric, capacity, where)
    rc, lab, d32, d64, off, cnt = raw(p.eng, queries, metric, radius, capacity, int(offsets[-1]), where)
    tag = f"{tag} words={queries.shape[1]} {metric} nq={len(queries)} r={radius!r} cap={capacity}"
    assert rc == (OVERFLOW if (counts > capacity).any() else OK), tag
    assert np.array_equal(cnt, counts) and np.array_equal(off, offsets), f"{tag}: counts / offsets"
    assert np.array_equal(lab, labels), f"{tag}: labels"
    assert np.array_equal(d64.view(np.int64), w64.view(np.int64)), f"{tag}: dist64 bits"
    assert np.array_equal(d32.view(np.int32), w64.astype(np.float32).view(np.int32)), f"{tag}: float distances"
    return want


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(words):
        if words not in made:
            made[words] = Pair(N, words)
        return made[words]

    yield get
    for p in made.values():
        p.close()


def radii(p, queries, metric):
    """The last query's 151st smallest distance, the next value below it, 0, a negative radius, one no distance exceeds."""
    idx = np.flatnonzero(p.model.candidates(BT, None, p.words))
    codes = np.array([p.model.bits_rows(BT)[i] for i in idx.tolist()], dtype=np.uint64)
    d = np.sort(distances(queries[-1:], codes, metric)[0])
    at = float(d[min(150, d.size - 1)])
    return [at, float(np.nextafter(at, -np.inf)), 0.0, -1.0, 64.0 * p.words if metric == "hamming" else 1.0]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("words", WIDTHS)
def test_every_width_against_the_model(pairs, words, metric):
    p = pairs(words)
    for nq in (1, TILE - 1, TILE, TILE + 1):
        queries = p.queries(nq)
        for i, r in enumerate(radii(p, queries, metric)):
            labels, d64, offsets, counts = check(p, queries, metric, r)
            if r == 0.0:
                assert counts[0] >= 1 and labels[0] == N - 1 and d64[0] == 0  # the planted copy of the target
            if r < 0:
                assert not counts.any()
            if i == 4:
                assert (counts == p.model.candidates(BT, None, words).sum()).all()
    at, below = radii(p, p.queries(2), metric)[:2]
    a, b = check(p, p.queries(2), metric, at)[3], check(p, p.queries(2), metric, below)[3]
    assert a[1] > b[1], "the radius is inclusive: the tie group on it is in, and out just below it"


@pytest.mark.parametrize("words", [2, 33])
def test_more_queries_than_one_pass_and_a_query_is_the_same_alone(pairs, words):
    p = pairs(words)
    queries = p.queries(257)
    half = prog([(W.GE, INT, 1, 0)])
    for metric, where in (("hamming", None), ("jaccard", half)):
        r = radii(p, queries[:2], metric)[0]
        labels, d64, offsets, counts = check(p, queries, metric, r, where=where, tag="257 queries")
        assert counts[256] > 0 or counts[255] > 0
        for q in (0, 31, 32, 255, 256):
            one = check(p, queries[q:q + 1], metric, r, where=where, tag=f"query {q} alone")
            assert np.array_equal(one[0], labels[offsets[q]:offsets[q + 1]])
            assert np.array_equal(one[1].view(np.int64), d64[offsets[q]:offsets[q + 1]].view(np.int64))


def test_where_programs_and_the_all_zero_jaccard_query(pairs):
    p = pairs(3)
    queries = np.concatenate([np.zeros((1, 3), np.uint64), p.queries(5)])
    lit = np.array([0.25]).view(np.int64)[0]
    for where in (prog([(W.EQ, INT, 3, 0)]), prog([(W.EXISTS, BT, 0, 0), (W.NOT, 0, 0, 0)]),
                  prog([(W.LT, FLT, int(lit), 0), (W.IN, INT, 0, 2), (W.OR, 0, 0, 0)], [0, 5]), None):
        for metric in METRICS:
            check(p, queries, metric, radii(p, queries, metric)[0], where=where, tag="where")
    # the all-zero query: distance 0.0 to the all-zero rows (u == 0), exactly 1 to every other row
    rows = p.model.bits_rows(BT)
    zeros = [i for i in np.flatnonzero(p.model.candidates(BT, None, 3)).tolist() if rows[i] == (0, 0, 0)]
    labels, d64, offsets, counts = check(p, queries[:1], "jaccard", 0.0, tag="zero query")
    assert labels.tolist() == zeros and len(zeros) >= 2 and not d64.any() and not np.signbit(d64).any()
    assert check(p, queries[:1], "jaccard", np.nextafter(1.0, 0.0))[3][0] == len(zeros)
    assert check(p, queries[:1], "jaccard", np.inf)[3][0] == p.model.candidates(BT, None, 3).sum()


@pytest.fixture(scope="module")
def graded():
    """20,011 shuffled 64-bit codes with 1, 2, 3, 1,023, 1,024, 1,025, 16,384 and 16,385 rows within Hamming 1 .. 8 of the
    all-zero code (the nearest at row 0), 40 copies of one dense code (one at the last row), the rest of 9 or more bits."""
    rng = np.random.default_rng(77)
    n = 20_011
    pops = [1, 2, 3] + [4] * 1020 + [5, 6] + [7] * 15359 + [8]
    pops += rng.integers(9, 65, size=n - 40 - len(pops)).tolist()
    codes = np.zeros((n, 1), np.uint64)
    for r, k in enumerate(pops):
        codes[r, 0] = sum(1 << int(b) for b in rng.choice(64, size=k, replace=False))
    dense = np.uint64(0x9E3779B97F4A7C15)
    codes[len(pops):, 0] = dense
    order = rng.permutation(n)  # new row i holds old row order[i]: old row 0 stays first, old row n - 1 last
    for old in (0, n - 1):
        at = int(np.flatnonzero(order == old)[0])
        order[[old, at]] = order[[at, old]]
    codes = codes[order]
    eng, model = HipScanEngine(D, "ip", device=0), BitsOracleEngine(D, "ip")
    for e in (eng, model):
        e.define_attr(BT, "bits")
        e.append(np.ones((n, D), np.float32))
        e.bits_set(BT, 0, column(codes))
    yield SimpleNamespace(eng=eng, model=model, words=1, dense=np.array([[dense]], np.uint64))
    eng.close()


def test_segments_of_every_length_are_sorted(graded):
    zero = np.zeros((1, 1), np.uint64)
    for r, n_hits in zip(range(1, 8), (1, 2, 3, 1023, 1024, 1025, 16384)):
        labels, d64, offsets, counts = check(graded, zero, "hamming", float(r), tag="graded")
        assert counts[0] == n_hits and labels[0] == 0 and d64[0] == 1  # the nearest row is row 0
    check(graded, zero, "hamming", 4.0, capacity=1023, tag="capacity met")
    # one tie group, ordered by label alone, its last member the last row; and all of these in one batch
    labels, d64, offsets, counts = check(graded, graded.dense, "jaccard", 0.0, tag="ties")
    assert counts[0] == 40 and labels[-1] == 20_010 and (np.diff(labels) > 0).all() and not d64.any()
    batch = np.concatenate([zero, graded.dense, ~graded.dense, zero])
    check(graded, batch, "hamming", 7.0, tag="batch")
    # Jaccard over a segment of the 1,024-thread sort: the all-ones query is at (64 - popcount) / 64
    labels, d64, offsets, counts = check(graded, ~zero, "jaccard", 1 - 9 / 64, tag="jaccard")
    assert 2048 < counts[0] <= 4096


def test_capacity_and_the_packed_protocol(graded):
    zero = np.zeros((1, 1), np.uint64)
    batch = np.concatenate([graded.dense, zero, graded.dense])
    # 16,385 hits: over the limit -- the exact count, an empty segment, the other queries served
    labels, d64, offsets, counts = check(graded, batch, "hamming", 8.0, tag="capacity + 1")
    assert counts.tolist()[1] == 16385 and offsets[1] == offsets[2] and counts[0] == counts[2] > 0
    check(graded, batch, "hamming", 4.0, capacity=1022, tag="capacity + 1, small")
    labels, d64, offsets, counts = range_bits(graded.model, BT, batch, 4.0, "hamming")
    need = int(offsets[-1])
    # one entry short: nothing written, the layout exact; then the repeat call succeeds (check, above, is that call)
    rc, lab, d32, o64, off, cnt = raw(graded.eng, batch, "hamming", 4.0, total=need - 1)
    assert rc == OVERFLOW and (lab == -7).all() and (d32 == -7).all() and (o64 == -7).all()
    assert np.array_equal(off, offsets) and np.array_equal(cnt, counts)
    check(graded, batch, "hamming", 4.0)
    # the counting call: NULL arrays
    rc, lab, d32, o64, off, cnt = raw(graded.eng, batch, "hamming", 4.0, total=0, arrays=False)
    assert rc == OVERFLOW and off[-1] == need and np.array_equal(cnt, counts)
    rc, lab, d32, o64, off, cnt = raw(graded.eng, batch, "hamming", -1.0, total=0, arrays=False)
    assert rc == OK and not off.any() and not cnt.any()
    rc, lab, d32, o64, off, cnt = raw(graded.eng, batch, "hamming", 4.0, capacity=MAX_HITS + 1, total=need)
    assert rc == UNSUPPORTED and (lab == -7).all() and (off == -7).all() and (cnt == -7).all()


def test_the_blocks_stride_over_a_large_index():
    """512 blocks of 16 rows per step sweep 8,192 rows: a one-tile call walks 40,000 33-word rows five times, three tiles 15."""
    p = Pair(40_000, 33, seed=11, batches=2)
    try:
        for metric in METRICS:
            r = radii(p, p.queries(1), metric)[0]  # (a distance of the target: its copy and its neighbour lie inside)
            labels, d64, offsets, counts = check(p, p.queries(3), metric, r, tag="one tile")
            assert labels[0] == 39_999 and labels[1] == 0
        r = radii(p, p.queries(1), "hamming")[0]
        check(p, p.queries(65), "hamming", r, where=prog([(W.GE, INT, 1, 0)]), tag="three tiles")
    finally:
        p.close()


def test_refusals_leave_the_handle_as_it_was(pairs):
    p = pairs(4)
    q = p.queries(3)
    refused = {
        "an int column": dict(attr=INT), "a float column": dict(attr=FLT), "an undefined column": dict(attr=9),
        "words 0": dict(words=0), "words 256": dict(words=256), "metric 2": dict(metric=2), "metric -1": dict(metric=-1),
        "a NaN radius": dict(radius=float("nan")), "capacity 0": dict(capacity=0), "total -1": dict(total=-1),
        "null arrays": dict(arrays=False), "null offsets": dict(offsets=False), "nq -1": dict(nq=-1),
        "a bad program": dict(where=prog([(W.LT, BT, 0, 0)])),
    }
    for tag, kw in refused.items():
        args = dict(metric="hamming", radius=3.0, total=8)
        args.update(kw)
        rc, lab, d32, d64, off, cnt = raw(p.eng, q, **args)
        assert rc == INVALID and (lab == -7).all() and (off == -7).all() and (cnt == -7).all(), tag
    rc, lab, d32, d64, off, cnt = raw(p.eng, q, "hamming", 3.0, nq=0)
    assert rc == OK and off.tolist() == [0]
    for metric in METRICS:
        check(p, q, metric, radii(p, q, metric)[0], tag="after the refusals")
