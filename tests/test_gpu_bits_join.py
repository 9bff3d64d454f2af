"""mlvdb_join_within_bits on the MI355X against its defining rule, bit for bit: ``bits_range_helpers.range_bits`` over the left
rows' stored codes (once per corpus and metric, at the radius nothing exceeds), the row itself or every label <= it dropped."""
import numpy as np
import pytest

from mlvectordb_amd import _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from tests.bits_helpers import METRICS
from tests.bits_range_helpers import MAX_HITS, range_bits
from tests.test_gpu_bits import BT, INT, N, Pair, column, prog

pytestmark = pytest.mark.gpu

OK, OVERFLOW = 0, 7  # include/mlvdb_hip.h
OTHERS, LATER, KC, TL = _native.JOIN_OTHERS, _native.JOIN_LATER, 8, 128  # (kBitsJoinKC, kBitsJoinTile)
WIDTHS = (1, 4, KC - 1, KC, KC + 1, 2 * KC + 1, 33, 255)
HALF = prog([(W.GE, INT, 1, 0)])


def raw(eng, left, mode, words, metric, radius, capacity=MAX_HITS, total=0, where=None, arrays=True):
    """One mlvdb_join_within_bits call -> (status, labels, dist, dist64, offsets, counts); the outputs are pre-filled with -7."""
    left, n = np.ascontiguousarray(left, dtype=np.int64), len(left)
    lab, d32, d64 = np.full(max(total, 1), -7, np.int64), np.full(max(total, 1), -7, np.float32), np.full(max(total, 1), -7.0)
    off, cnt = np.full(n + 1, -7, np.int64), np.full(max(n, 1), -7, np.int64)
    w, keep = HipScanEngine._where_arg(where)
    ptr = lambda a: a.ctypes.data if arrays else None
    rc = _native.load().mlvdb_join_within_bits(
        eng.handle, BT, left.ctypes.data, n, mode, words, _native.BITS_METRIC_CODES[metric],
        float(radius), capacity, total, w, ptr(lab), ptr(d32), ptr(d64), off.ctypes.data, cnt.ctypes.data)
    return rc, lab[:total], d32[:total], d64[:total], off, cnt[:n]


def rule(p, metric, where=None):
    """{a: (labels, dist64)}: range_bits for the stored code of every live row a that holds a code of p.words words."""
    cand = np.flatnonzero(p.model.candidates(BT, None, p.words))
    codes = np.array([p.model.bits_rows(BT)[i] for i in cand.tolist()], dtype=np.uint64).reshape(cand.size, p.words)
    lab, d64, off, _ = range_bits(p.model, BT, codes, 64.0 * p.words if metric == "hamming" else 1.0, metric, MAX_HITS, where)
    return {a: (lab[off[i]:off[i + 1]], d64[off[i]:off[i + 1]]) for i, a in enumerate(cand.tolist())}


def partners(ref, left, mode, radius, capacity=MAX_HITS):
    none = (np.zeros(0, np.int64), np.zeros(0))
    labels, d64, counts = [], [], np.zeros(len(left), np.int64)
    for i, a in enumerate(np.asarray(left).tolist()):
        lab, d = ref.get(a, none)
        keep = (d <= radius) & ((lab > a) if mode == LATER else (lab != a))
        counts[i] = keep.sum()
        if counts[i] <= capacity:
            labels.append(lab[keep])
            d64.append(d[keep])
    offsets = np.concatenate([[0], np.cumsum(np.where(counts <= capacity, counts, 0))]).astype(np.int64)
    return np.concatenate(labels + [none[0]]), np.concatenate(d64 + [none[1]]), offsets, counts


def check(p, ref, left, mode, metric, radius, capacity=MAX_HITS, where=None, tag=""):
    want = labels, w64, offsets, counts = partners(ref, left, mode, radius, capacity)
    got = rc, lab, d32, d64, off, cnt = raw(p.eng, left, mode, p.words, metric, radius, capacity, int(offsets[-1]), where)
    tag = f"{tag} words={p.words} {metric} mode={mode} n={len(left)} r={radius!r} cap={capacity}"
    assert rc == (OVERFLOW if (counts > capacity).any() else OK), tag
    assert np.array_equal(cnt, counts) and np.array_equal(off, offsets), f"{tag}: counts / offsets"
    assert np.array_equal(lab, labels), f"{tag}: labels"
    assert np.array_equal(d64.view(np.int64), w64.view(np.int64)), f"{tag}: dist64 bits"
    assert np.array_equal(d32.view(np.int32), w64.astype(np.float32).view(np.int32)), f"{tag}: float distances"
    return want, got


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(words, metric, where=None):
        if words not in made:
            made[words] = (Pair(N, words), {})
        p, refs = made[words]
        if (metric, where is None) not in refs:
            refs[metric, where is None] = rule(p, metric, where)
        return p, refs[metric, where is None]

    yield get
    for p, _ in made.values():
        p.close()


def radii(ref, left, metric, words):
    """A tie value (the 151st smallest distance of the last left row with a code), just below it, 0, negative, the largest."""
    d = ref[[a for a in np.asarray(left).tolist() if a in ref][-1]][1]
    at = float(d[min(150, d.size - 1)])
    return [at, float(np.nextafter(at, -np.inf)), 0.0, -1.0, 64.0 * words if metric == "hamming" else 1.0]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mode", (OTHERS, LATER))
@pytest.mark.parametrize("words", WIDTHS)
def test_every_width_mode_and_metric_against_the_rule(pairs, words, mode, metric):
    p, ref = pairs(words, metric)
    rng = np.random.default_rng(words)
    cand = np.array(sorted(ref))
    for n_left in (1, TL - 1, TL, TL + 1, None):
        left = cand if n_left is None else np.sort(rng.choice(N, size=n_left, replace=False)) if n_left > 1 else cand[-1:]
        for i, r in enumerate(radii(ref, left, metric, words)):
            (labels, d64, offsets, counts), _ = check(p, ref, left, mode, metric, r)
            if i == 4:  # every candidate but the removed labels, and the early exit never fires
                below = np.searchsorted(cand, left, side="right" if mode == LATER else "left")
                removed = below if mode == LATER else np.isin(left, cand).astype(np.int64)
                assert np.array_equal(counts, np.where(np.isin(left, cand), cand.size - removed, 0))
    if words == 255:  # four waves of 512 left rows give the bytes of one wave
        p.eng.set_tuning(BITS_JOIN_WS_MB=1)
        check(p, ref, cand, mode, metric, radii(ref, cand, metric, words)[0], tag="waves")
        p.eng.set_tuning(BITS_JOIN_WS_MB=32)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("mode", (OTHERS, LATER))
@pytest.mark.parametrize("words", (2 * KC + 1, 33))
def test_the_early_exit_drops_no_hit_and_keeps_no_miss(words, mode, metric):
    """Copies of a code that differ in the last chunk alone by R (a hit), R + 1 and 3 R bits, in the first alone by R + 1."""
    R, p = 5, Pair(300, words, seed=3)
    try:
        rng = np.random.default_rng(words + mode)
        base = rng.integers(0, 2 ** 64, size=words, dtype=np.uint64)
        last = ((words - 1) // KC) * KC * 64  # the first bit of the last chunk

        def flipped(lo, hi, k):
            out = base.copy()
            for b in rng.choice(np.arange(lo, hi), size=k, replace=False).tolist():
                out[b >> 6] ^= np.uint64(1 << (b & 63))
            return out

        at = np.array([3, 120, 140, 160, 290], np.int64)  # rows of three tiles (moved to the next live row that holds a code)
        codes = np.stack([base, flipped(last, 64 * words, R), flipped(last, 64 * words, R + 1), flipped(0, 64 * KC, R + 1),
                          flipped(last, 64 * words, 3 * R)])
        live = np.flatnonzero(p.model.candidates(BT, None, None))
        at = live[np.searchsorted(live, at)]
        assert p.both("bits_set_at", BT, at, column(codes)) == (5, 5)
        ref = rule(p, metric)
        radius = float(R) if metric == "hamming" else float(ref[int(at[0])][1][1])  # Jaccard: the distance of the R-bit copy
        left = np.array(sorted(ref))
        (labels, d64, offsets, counts), _ = check(p, ref, left, mode, metric, radius, tag="planted")
        i = int(np.searchsorted(left, at[0]))
        assert labels[offsets[i]:offsets[i + 1]].tolist() == [int(at[1])]
    finally:
        p.close()


def test_where_restricts_the_partners_and_a_left_label_without_a_code_has_none(pairs):
    for metric in METRICS:
        p, ref = pairs(3, metric, HALF)
        left = np.arange(0, N, 3)
        cand = np.isin(left, sorted(pairs(3, metric)[1]))
        for mode in (OTHERS, LATER):
            r = radii(ref, left, metric, 3)[0]
            (labels, d64, offsets, counts), _ = check(p, ref, left, mode, metric, r, where=HALF, tag="where")
            assert not counts[~cand].any() and counts[cand].any()  # (dead, absent and 4-word rows are among the labels)


def test_capacity_the_packed_protocol_and_repeatability(pairs):
    p, ref = pairs(4, "hamming")
    left = np.array(sorted(ref))[::2]
    r = radii(ref, left, "hamming", 4)[0]
    labels, d64, offsets, counts = partners(ref, left, OTHERS, r)
    (_, _, cut, _), (rc, *_) = check(p, ref, left, OTHERS, "hamming", r, capacity=int(counts.max()) - 1, tag="capacity")
    assert rc == OVERFLOW and cut[-1] < offsets[-1]
    need = int(offsets[-1])
    rc, lab, d32, o64, off, cnt = raw(p.eng, left, OTHERS, 4, "hamming", r, total=need - 1)
    assert rc == OVERFLOW and (lab == -7).all() and (d32 == -7).all() and (o64 == -7).all() and np.array_equal(off, offsets)
    rc, lab, d32, o64, off, cnt = raw(p.eng, left, OTHERS, 4, "hamming", r, total=0, arrays=False)
    assert rc == OVERFLOW and off[-1] == need and np.array_equal(cnt, counts)
    one, two = (raw(p.eng, left, LATER, 4, "jaccard", 0.4, total=need * 4) for _ in range(2))
    assert one[0] == two[0] == OK and all(a.tobytes() == b.tobytes() for a, b in zip(one[1:], two[1:]))

