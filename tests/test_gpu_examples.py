"""Recommend / discover on the MI355X (include/mlvdb_examples.h), at the engine level through the C ABI.
1. Replay: the model of tests/examples_helpers.py run on the device's own bits -- ``pair_distances(example, every label)`` for
   every d_j(x) -- must reproduce ``search_examples`` bit for bit: labels, tiers, values, counts, padding.  No tolerance.  The
   bags cover the tile edges (1, 8, 9, 16, 17, 63, 64 examples: one tile, a full one, the first carried state, eight launches),
   stored and raw examples mixed, repeated labels, tombstoned examples; exclusion on and off.
2. Identities with the plain exact search, bit for bit.
3. Against the NumPy fp64 oracle under an asserted gap precondition.
4. Structure: the workspace budget, repeat calls, split batches, filters, mutations, empty cases, the C-level refusals.
Rows are Gaussian."""
import numpy as np
import pytest

from mlvectordb_amd import Index, Vector, _native
from mlvectordb_amd import where as W
from mlvectordb_amd.engine import HipScanEngine
from oracle import exact_scan
from tests.conftest import dump_mismatch
from tests.examples_helpers import (BEST, CONTEXT, DISCOVER, NEG, NO_TIER, POS, TARGET, ExamplesOracleEngine,
                                    example_vectors, model_search, random_bags)
from tests.helpers import SCORE_ATOL
from tests.scored_helpers import GAP_MIN

pytestmark = pytest.mark.gpu

MODES = {"best": BEST, "discover": DISCOVER, "context": CONTEXT}
BAG_SIZES = (1, 8, 9, 16, 17, 63, 64)
NAMES = ("labels", "tiers", "values", "counts")
TRUE = W.Program(np.array([(W.TRUE, 0, 0, 0)], dtype=W.OP_DTYPE), np.zeros(0, np.int64))
INT, LIST = 0, 1


def W1(op, attr, a=0, b=0, table=()):
    return W.Program(np.array([(op, attr, a, b)], dtype=W.OP_DTYPE), np.array(table, dtype=np.int64))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _mask(labels, n):
    m = np.zeros(n, bool)
    m[labels] = True
    return m


def _corpus(space, n, d, seed, tomb=0.0):
    rng = np.random.default_rng(seed)
    eng = HipScanEngine(d, space, device=0)
    rows = rng.standard_normal((n, d), dtype=np.float32)
    eng.append(rows)
    if tomb:
        eng.tombstone(np.flatnonzero(rng.random(n) < tomb))
    return eng, rows, rng


class Bits:
    """What the model reads, from the device: d_j(x) for every example of a call and every row, and the live rows."""

    def __init__(self, eng, rows, bags):
        self.eng, self.bags = eng, bags
        labels, vectors, roles, offsets = bags
        self.n = eng.counts()[0]
        ex = example_vectors(rows, labels, vectors)
        self.D = eng.pair_distances(ex, np.broadcast_to(np.arange(self.n), (ex.shape[0], self.n)))[0]
        self.live = _mask(eng.where_labels(TRUE), self.n)

    def head(self, nq):
        labels, vectors, roles, offsets = self.bags
        e = int(offsets[nq])
        return labels[:e], vectors[:e], roles[:e], offsets[:nq + 1]

    def want(self, mode, k, exclude=True, where=None, nq=None):
        labels, _, roles, offsets = self.bags if nq is None else self.head(nq)
        live = self.live if where is None else _mask(self.eng.where_labels(where), self.n)
        return model_search(mode, self.D, labels, roles, offsets, k, live, exclude)

    def got(self, mode, k, exclude=True, where=None, nq=None):
        labels, vectors, roles, offsets = self.bags if nq is None else self.head(nq)
        return self.eng.search_examples(mode, labels, vectors, roles, offsets, k, exclude=exclude, where=where)


def _same(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        if g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
            dump_mismatch(f"examples_{tag}", **{f"got_{n}": a for n, a in zip(NAMES, got)},
                          **{f"want_{n}": a for n, a in zip(NAMES, want)})
            bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(g.shape[0], -1).any(axis=1))
            raise AssertionError(f"{tag}: {name} differs in {bad.size} queries, first {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


def _replay(b, mode, k, tag, **kw):
    got = b.got(mode, k, **kw)
    _same(got, b.want(mode, k, **kw), tag)
    labels, tiers, values, counts = got
    pad = np.arange(k)[None, :] >= counts[:, None]  # the padding, stated on its own
    assert (labels[pad] == -1).all() and (tiers[pad] == NO_TIER).all() and np.isposinf(values[pad]).all()
    assert (labels[~pad] >= 0).all()
    return got


# ---------------------------------------------------------------- 1. replay of the device's own bits
SHAPES = ((1, 16), (15, 16), (16, 16), (17, 16), (5000, 16), (300, 768), (700, 300))


@pytest.mark.parametrize("n,d", SHAPES)
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_search_examples_equals_the_model_replayed_on_the_devices_own_bits(space, n, d):
    eng, rows, rng = _corpus(space, n, d, 11 * n + d + len(space), tomb=1 / 3 if n >= 15 else 0.0)
    try:
        dead = ~_mask(eng.where_labels(TRUE), n)
        for name, mode in MODES.items():
            # 70 queries: every bag size ten times -- one query tile row per query, several launches for most
            bags = random_bags(rng, mode, BAG_SIZES * 10, n, d)
            labels, _, roles, offsets = bags
            assert (labels == -1).any() and (labels >= 0).any()
            if n >= 15:
                assert dead[labels[labels >= 0]].any(), "no tombstoned example"
                assert any(np.unique(l[l >= 0]).size < (l >= 0).sum() for l in np.split(labels, offsets[1:-1])), "no repeat"
            b = Bits(eng, rows, bags)
            for nq, k in ((70, 10), (9, 64), (1, 1)):  # k = 64 is above the candidate count of the small corpora
                tag = f"{space}_{n}x{d}_{name}_{nq}_{k}"
                got = _replay(b, mode, k, tag, nq=nq)
                _replay(b, mode, k, tag + "_keep", nq=nq, exclude=False)
                assert k < 64 or n >= 64 or (got[3] < k).all()
            # bags of at most 1, 2 and 4 examples: the narrower tiles of the geometry
            for sizes in ((1, 1, 1), (2, 1, 2), (3, 4, 1, 2)):
                small = Bits(eng, rows, random_bags(rng, mode, sizes, n, d))
                _replay(small, mode, 10, f"{space}_{n}x{d}_{name}_bags{max(sizes)}")
            if mode == BEST and n >= 5000:
                # an example that is itself the best row: a live stored POS example has distance 0 (l2) / the least (cosine)
                on, off = b.got(mode, 1), b.got(mode, 1, exclude=False)
                own = [set(l[l >= 0].tolist()) for l in np.split(labels, offsets[1:-1])]
                assert sum(int(off[0][q, 0]) in own[q] for q in range(70)) >= 10
                assert not any(int(on[0][q, 0]) in own[q] for q in range(70))
    finally:
        eng.close()


@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_rows_too_wide_for_a_tile_of_two_take_one_example_per_launch_and_carry_the_pairs(space):
    n, d = 40, 8192  # 64 KiB of LDS per staged example: a pair spans two launches, its POS distance travels with the state
    eng, rows, rng = _corpus(space, n, d, 2, tomb=0.25)
    try:
        for name, mode in MODES.items():
            b = Bits(eng, rows, random_bags(rng, mode, (1, 3, 2, 7, 4), n, d))
            _replay(b, mode, 10, f"wide_{space}_{name}")
            _replay(b, mode, 64, f"wide_{space}_{name}_keep", exclude=False)
    finally:
        eng.close()


# ---------------------------------------------------------------- 2. identities with the plain exact search
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_discover_without_pairs_and_best_with_one_positive_are_the_plain_exact_search(space):
    n, d, k = 3000, 100, 10
    rng = np.random.default_rng(5)
    eng = HipScanEngine(d, space, device=0, strategy="exact")
    try:
        rows = rng.standard_normal((n, d), dtype=np.float32)
        eng.append(rows)
        eng.tombstone(np.arange(0, n, 3))
        live = np.flatnonzero(np.arange(n) % 3 != 0)
        nq = 9
        labels = np.where(np.arange(nq) % 2 == 0, -1, rng.choice(live, nq)).astype(np.int64)  # raw and stored targets
        vectors = rng.standard_normal((nq, d)).astype(np.float32)
        qs = example_vectors(rows, labels, vectors)
        offsets = np.arange(nq + 1, dtype=np.int64)
        plain_lab, _, plain_cnt, plain_d64 = eng.search64(qs, k)
        for mode, role in ((DISCOVER, TARGET), (BEST, POS)):
            lab, tiers, values, cnt = eng.search_examples(mode, labels, vectors, np.full(nq, role, np.int32), offsets, k,
                                                          exclude=False)
            assert np.array_equal(lab, plain_lab) and np.array_equal(cnt, plain_cnt) and (tiers == 0).all()
            assert np.array_equal(_bits(values), _bits(plain_d64))
    finally:
        eng.close()


# ---------------------------------------------------------------- 3. against the NumPy oracle
def _oracle_case(space, mode, seed, n=3000, d=48, nq=8, k=10):
    """Rows, bags and the oracle's answer for k + 1, with the gaps the comparison needs: (rows, bags, want, min gap)."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    sizes = [(3, 5, 9, 12, 17, 4, 6, 11)[i % 8] for i in range(nq)]
    bags = random_bags(rng, mode, sizes, n, d, repeat_share=0.0)
    labels, vectors, roles, offsets = bags
    D = exact_scan.exact_distances(example_vectors(rows, labels, vectors), rows, space)
    want = model_search(mode, D, labels, roles, offsets, k + 1, np.ones(n, bool), True)
    gap = np.inf
    for q in range(nq):
        a, e = int(offsets[q]), int(offsets[q + 1])
        cand = np.ones(n, bool)
        cand[labels[a:e][labels[a:e] >= 0]] = False
        Dq, r = D[a:e][:, cand], roles[a:e]
        if mode == BEST:  # the one comparison: p against n
            if (r == POS).any() and (r == NEG).any():
                gap = min(gap, np.abs(Dq[r == POS].min(axis=0) - Dq[r == NEG].min(axis=0)).min())
        else:  # every pair of every candidate row
            head = 1 if mode == DISCOVER else 0
            gap = min(gap, np.abs(Dq[head::2] - Dq[head + 1::2]).min())
        t, v = want[1][q].astype(np.int64), want[2][q]
        # adjacent ranked keys through rank k + 1: apart inside a tier -- or both exactly 0.0, which a CONTEXT sum over no
        # missed pair is on the device as well once no comparison can flip
        near = (np.diff(t) == 0) & ~((v[1:] == 0.0) & (v[:-1] == 0.0))
        if near.any():
            gap = min(gap, np.diff(v)[near].min())
    return rows, bags, want, gap


ORACLE_SEEDS = {(s, m): 40 + i for i, (s, m) in enumerate((s, m) for s in ("l2", "cosine", "ip") for m in MODES)}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("space", ["l2", "cosine", "ip"])
def test_search_examples_equals_the_numpy_oracle_where_its_keys_are_apart(space, mode):
    k = 10
    rows, bags, want, gap = _oracle_case(space, MODES[mode], ORACLE_SEEDS[(space, mode)], k=k)
    assert (want[3] == k + 1).all() and gap > GAP_MIN, \
        f"precondition: oracle comparisons or keys closer than {GAP_MIN} ({gap}): choose another seed"
    eng = HipScanEngine(rows.shape[1], space, device=0)
    try:
        eng.append(rows)
        labels, vectors, roles, offsets = bags
        lab, tiers, values, cnt = eng.search_examples(MODES[mode], labels, vectors, roles, offsets, k)
        print(f"{space} {mode}: max |value - oracle| {np.abs(values - want[2][:, :k]).max():.3e}, min gap {gap:.3e}")
        assert np.array_equal(lab, want[0][:, :k]) and np.array_equal(tiers, want[1][:, :k]) and (cnt == k).all()
        assert np.abs(values - want[2][:, :k]).max() <= SCORE_ATOL
    finally:
        eng.close()


# ---------------------------------------------------------------- 4. structure
def test_every_workspace_budget_repeat_calls_and_split_batches_return_the_same_bytes():
    eng, rows, rng = _corpus("cosine", 5000, 100, 3, tomb=0.2)
    try:
        assert eng.get_tuning("EXAMPLES_WS_MB") == 1024
        for name, mode in MODES.items():
            bags = random_bags(rng, mode, BAG_SIZES * 10, 5000, 100)
            b = Bits(eng, rows, bags)
            one = _replay(b, mode, 10, f"budget_{name}")
            two = b.got(mode, 10)
            eng.set_tuning(EXAMPLES_WS_MB=1)  # 80 kB of state per query with a carried bag: a dozen such queries a chunk
            small = b.got(mode, 10)
            eng.set_tuning(EXAMPLES_WS_MB=1024)
            labels, vectors, roles, offsets = bags
            e = int(offsets[33])
            head = eng.search_examples(mode, labels[:e], vectors[:e], roles[:e], offsets[:34], 10)
            tail = eng.search_examples(mode, labels[e:], vectors[e:], roles[e:], offsets[33:] - e, 10)
            for a, b2, c, h, t in zip(one, two, small, head, tail):
                assert a.tobytes() == b2.tobytes() == c.tobytes()
                assert a.tobytes() == np.concatenate([h, t]).tobytes()
    finally:
        eng.close()


def test_a_budget_below_one_querys_state_still_takes_one_query_per_chunk():
    n, d = 70_000, 16  # 1.12 MB of state per carried query against a budget of 1 MiB
    eng, rows, rng = _corpus("l2", n, d, 17, tomb=0.1)
    try:
        for name, mode in MODES.items():
            bags = random_bags(rng, mode, (9, 17, 1, 64, 12), n, d)
            b = Bits(eng, rows, bags)
            whole = _replay(b, mode, 10, f"one_query_budget_{name}")
            eng.set_tuning(EXAMPLES_WS_MB=1)
            tight = b.got(mode, 10)
            eng.set_tuning(EXAMPLES_WS_MB=0)  # (anything below 1 is 1)
            least = b.got(mode, 10)
            eng.set_tuning(EXAMPLES_WS_MB=1024)
            for a, t, l in zip(whole, tight, least):
                assert a.tobytes() == t.tobytes() == l.tobytes()
    finally:
        eng.close()


def test_a_where_program_with_a_list_op_and_mutations_are_followed():
    n, d = 2000, 24
    eng, rows, rng = _corpus("l2", n, d, 9)
    try:
        eng.define_attr(INT, "int64")
        eng.define_attr(LIST, "int64_list")
        eng.set_attr(INT, 0, rng.integers(-2, 6, n).astype(np.int64))
        lists = [sorted(set(rng.integers(0, 10, rng.integers(0, 5)).tolist())) for _ in range(n)]
        eng.set_attr_list(LIST, 0, W.encode_list_column("tags", "int[]", lists, {}))
        where = W.Program(np.array([(W.HAS_ANY, LIST, 0, 3), (W.GE, INT, 2, 0), (W.AND, 0, 0, 0)], dtype=W.OP_DTYPE),
                          np.array([1, 4, 7], np.int64))
        assert 0 < eng.where_count(where) < n

        def check(tag, rows):
            for name, mode in MODES.items():
                bags = random_bags(rng, mode, (1, 9, 17, 5, 64), rows.shape[0], d)
                b = Bits(eng, rows, bags)
                _replay(b, mode, 10, f"{tag}_{name}")
                got = _replay(b, mode, 64, f"{tag}_{name}_where", where=where)
                assert (got[3] <= eng.where_count(where)).all()

        check("fresh", rows)
        eng.tombstone(np.arange(0, n, 7))
        check("removed", rows)
        more = rng.standard_normal((333, d), dtype=np.float32)
        eng.append(more)
        check("added", np.concatenate([rows, more]))
    finally:
        eng.close()


def test_an_empty_index_and_no_query():
    eng = HipScanEngine(8, "l2", device=0)
    try:
        raw = np.ones((2, 8), np.float32)
        args = (np.array([-1, -1]), raw, np.array([POS, NEG], np.int32), np.array([0, 2]))
        lab, tiers, values, cnt = eng.search_examples(BEST, *args, 5)
        assert (lab == -1).all() and (tiers == NO_TIER).all() and np.isposinf(values).all() and cnt.tolist() == [0]
        eng.append(np.ones((4, 8), np.float32))
        lab, tiers, values, cnt = eng.search_examples(BEST, np.zeros(0, np.int64), None, np.zeros(0, np.int32), np.array([0]), 5)
        assert lab.shape == (0, 5) and tiers.shape == (0, 5) and values.shape == (0, 5) and cnt.shape == (0,)
        lab, tiers, values, cnt = eng.search_examples(CONTEXT, *args, 5)  # all four rows tie at 0.0: label order
        assert lab.tolist() == [[0, 1, 2, 3, -1]] and cnt.tolist() == [4] and bits_equal(values[0, :4], 0.0)
        eng.tombstone(np.arange(4))
        lab, tiers, values, cnt = eng.search_examples(BEST, *args, 5)
        assert (lab == -1).all() and cnt.tolist() == [0]
    finally:
        eng.close()


def bits_equal(values, x):
    return (_bits(np.asarray(values, np.float64)) == _bits(np.full(len(values), x))).all()


def test_the_c_level_refusals_launch_nothing_and_write_nothing():
    eng, rows, rng = _corpus("l2", 100, 8, 1)
    try:
        lib = _native.load()
        eng.define_attr(INT, "int64")
        eng.last_stats()
        k = 5
        good = dict(mode=BEST, labels=[1, -1, 2], roles=[POS, NEG, POS], offsets=[0, 3], k=k, vectors=np.ones((3, 8), np.float32),
                    where=None, null=None, null_in=None)

        def call(**kw):
            a = {**good, **kw}
            labels = np.asarray(a["labels"], np.int64)
            roles = np.asarray(a["roles"], np.int32)
            offsets = np.asarray(a["offsets"], np.int64)
            nq = a.get("nq", offsets.size - 1)
            kk = max(a["k"], 1)
            outs = [np.full((max(nq, 1), kk), -7, np.int64), np.full((max(nq, 1), kk), -7, np.int32),
                    np.full((max(nq, 1), kk), -7.0), np.full(max(nq, 1), -7, np.int32)]
            ptrs = [None if a["null"] == i else o.ctypes.data for i, o in enumerate(outs)]
            vec = a["vectors"]
            w, keep = eng._where_arg(a["where"])
            ins = {"labels": labels.ctypes.data if labels.size else None, "roles": roles.ctypes.data if roles.size else None,
                   "offsets": offsets.ctypes.data}
            if a["null_in"]:
                ins[a["null_in"]] = None
            rc = lib.mlvdb_search_batch_examples(eng.handle, a["mode"], ins["labels"], None if vec is None else vec.ctypes.data,
                                                 ins["roles"], ins["offsets"], nq, a["k"], 1, w, *ptrs)
            assert all((o == -7).all() for o in outs), "a refused call wrote to its outputs"
            return rc

        INVALID, UNSUPPORTED = 1, 6
        bad_vec = np.ones((3, 8), np.float32)
        bad_vec[1, 3] = np.nan
        refused = {
            "k = 0": (dict(k=0), INVALID),
            "k = 65": (dict(k=65), UNSUPPORTED),
            "65 examples": (dict(labels=[1] * 65, roles=[POS] * 65, offsets=[0, 65], vectors=None), UNSUPPORTED),
            "offsets from 1": (dict(offsets=[1, 3]), INVALID),
            "offsets descend": (dict(offsets=[0, 3, 2]), INVALID),
            "an empty bag": (dict(offsets=[0, 0, 3]), INVALID),
            "label = total": (dict(labels=[1, -1, 100]), INVALID),
            "label = -2": (dict(labels=[1, -1, -2]), INVALID),
            "a raw example without vectors": (dict(vectors=None), INVALID),
            "a non-finite raw vector": (dict(vectors=bad_vec), INVALID),
            "a target in BEST": (dict(roles=[POS, NEG, TARGET]), INVALID),
            "an unknown role": (dict(roles=[POS, NEG, 3]), INVALID),
            "DISCOVER without its target": (dict(mode=DISCOVER, roles=[POS, NEG, POS]), INVALID),
            "DISCOVER with half a pair": (dict(mode=DISCOVER, labels=[1, 2], roles=[TARGET, POS], offsets=[0, 2]), INVALID),
            "DISCOVER with a swapped pair": (dict(mode=DISCOVER, roles=[TARGET, NEG, POS]), INVALID),
            "CONTEXT with a target": (dict(mode=CONTEXT, roles=[TARGET, POS, NEG]), INVALID),
            "CONTEXT with an odd bag": (dict(mode=CONTEXT, roles=[POS, NEG, POS]), INVALID),
            "an unknown mode": (dict(mode=3), INVALID),
            "a negative mode": (dict(mode=-1), INVALID),
            "a bad program": (dict(where=W1(W.EQ, 9, 1)), INVALID),
            "a program whose set range leaves its table": (dict(where=W1(W.IN, INT, 0, 3, (1, 2))), INVALID),
            "nq < 0": (dict(nq=-1), INVALID),
            **{f"null output {i}": (dict(null=i), INVALID) for i in range(4)},
            **{f"null {name}": (dict(null_in=name), INVALID) for name in ("labels", "roles", "offsets")},
        }
        for what, (kw, code) in refused.items():
            assert call(**kw) == code, what
        st = eng.last_stats()
        assert st["scan_launches"] == 0 and st["rows_scanned"] == 0
        with pytest.raises(RuntimeError, match=r"search_batch_examples failed \(6\).*MLVDB_MAX_TOPK"):
            eng.search_examples(BEST, [1], None, [POS], [0, 1], 65)
        bags = random_bags(rng, DISCOVER, (9, 3), 100, 8)
        _replay(Bits(eng, rows, bags), DISCOVER, 64, "after_refusals")  # the handle is as good as before
        assert eng.last_stats()["scan_launches"] >= 1
    finally:
        eng.close()


# ---------------------------------------------------------------- 5. the surface
def test_index_search_examples_and_discover_return_the_oracle_engines_answer():
    rng = np.random.default_rng(31)
    n, d = 400, 12
    rows = rng.standard_normal((n, d)).astype(np.float32)
    vecs = [Vector(values=r, metadata={}) for r in rows]
    device, oracle = Index(space="l2"), Index(space="l2", engine_factory=ExamplesOracleEngine)
    device.add(vecs, "ns")
    oracle.add(vecs, "ns")
    ids = [v.id for v in vecs]
    raw = rng.standard_normal(d).astype(np.float32)
    positive, negative = [[ids[3], raw], [ids[10]]], [[ids[20], ids[21]], []]
    context = [[(ids[1], ids[2]), (raw, ids[4])], [(ids[5], ids[6])]]
    for call in (lambda ix: ix.search_examples(positive, 10, "ns", "l2", negative=negative),
                 lambda ix: ix.search_discover(10, "ns", "l2", target=[ids[7], raw], context=context),
                 lambda ix: ix.search_discover(10, "ns", "l2", context=context)):
        got, want = call(device), call(oracle)
        assert np.array_equal(got.labels, want.labels) and np.array_equal(got.tiers, want.tiers)
        assert np.array_equal(got.counts, want.counts) and np.abs(got.values - want.values).max() <= SCORE_ATOL
        assert [h.vector_id for h in got[0]] == [h.vector_id for h in want[0]]
