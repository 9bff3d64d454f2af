"""Seeded call histories on ONE ``HipScanEngine`` handle from creation to close, against the NumPy model of the whole engine
(tests/history_helpers.py, tests/history_recent_helpers.py; the coverage the committed seed sets reach is asserted without a
GPU in tests/test_history_host.py).
Every answer is compared at once: labels, counts, groups, facet and bin counts exactly, distances by the suite's bars.  A
mismatch leaves history_<tag>.json (the ops up to the failing step) in the mismatch directory of tests/conftest.py and the
arrays beside it, names seed, step and op, and starts nothing more on the device but ``close()``."""
import pytest

from mlvectordb_amd.engine import HipScanEngine
from mlvectordb_amd.multi_device import MultiDeviceEngine
from tests import history_helpers as H
from tests import history_recent_helpers as R

pytestmark = pytest.mark.gpu


def _replay(key, make_engine):
    ops, expected = H.make_history(*key)
    drawn, redrawn = H.redraw_counts(*key)
    print(f"history {H.history_tag(*key)}: {redrawn} of {drawn} drawn queries were redrawn")
    engine = make_engine()
    try:
        stats = H.run_history(engine, ops, expected, H.history_tag(*key))
    finally:
        engine.close()
    assert stats["steps"] == len(ops)


@pytest.mark.parametrize("key", H.SMALL, ids=lambda key: H.history_tag(*key))
def test_small_history_equals_the_model_at_every_step(key):
    """d = 20 / 64 / 128 / 256 / 100: the bf16-shadow widths, the zero-padded int8 shadow and a 256-column row; the corpus stays
    under ~6,000 rows and ``set_strategy`` switches the routes."""
    seed, space, d, _ = key
    _replay(key, lambda: HipScanEngine(d, space, device=0))


@pytest.mark.parametrize("key", H.LARGE, ids=lambda key: H.history_tag(*key))
def test_large_history_crosses_the_threshold_of_auto_both_ways(key):
    """Appends of 12,000 rows until past 32,768 live rows, so that `auto` itself changes route at nq = 12 and 40; tombstones and a
    compaction back below the threshold; growth again."""
    seed, space, d, _ = key
    _replay(key, lambda: HipScanEngine(d, space, device=0))


@pytest.mark.parametrize("key", H.MULTI, ids=lambda key: H.history_tag(*key))
def test_history_through_three_logical_shards_equals_one_model(key):
    """``MultiDeviceEngine`` over three ``HipScanEngine`` shards on device 0, the ops of tests/test_host_fuzz.py."""
    seed, space, d, _ = key
    _replay(key, lambda: MultiDeviceEngine(d, space, [0, 0, 0]))


@pytest.mark.parametrize("key", H.WIDE, ids=lambda key: H.history_tag(*key))
def test_wide_history_equals_the_model_at_every_step(key):
    """The entry families added since the first histories -- ordered, diversified, grouped, by-example and late-interaction
    queries, updates and filtered deletes, list and sparse columns -- on one handle: pools that regrow, are repacked and
    reset, the inner searches on the filter route across mutations, masked calls before unmasked ones."""
    seed, space, d, _ = key
    _replay(key, lambda: HipScanEngine(d, space, device=0))


def test_an_index_outlives_a_destroyed_neighbour_that_used_every_workspace():
    """Engine B is opened first; engine A replays the first wide history -- every family's workspace, regrown rows, columns and
    pools -- and is closed, which frees all of it; then B replays the second one and equals the model at every step.  Answers
    only: the card is shared, so its free memory is not ours to assert on."""
    key_a, key_b = H.WIDE[0], H.WIDE[1]
    ops_a, expected_a = H.make_history(*key_a)
    ops_b, expected_b = H.make_history(*key_b)
    b = HipScanEngine(key_b[2], key_b[1], device=0)
    try:
        a = HipScanEngine(key_a[2], key_a[1], device=0)
        try:
            assert H.run_history(a, ops_a, expected_a, "neighbour_" + H.history_tag(*key_a))["steps"] == len(ops_a)
        finally:
            a.close()
        assert H.run_history(b, ops_b, expected_b, "survivor_" + H.history_tag(*key_b))["steps"] == len(ops_b)
    finally:
        b.close()


@pytest.mark.parametrize("key", H.WIDE_LARGE, ids=lambda key: H.history_tag(*key))
def test_wide_large_history_moves_the_inner_searches_between_the_routes(key):
    """Past 32,768 rows `auto` itself takes the filter route inside search_mmr / search_like / search_grouped and the tag-filtered
    search_each at nq = 12 and 40; a ``tombstone_where`` of about a third of the rows and a compaction bring it back; growth again."""
    seed, space, d, _ = key
    _replay(key, lambda: HipScanEngine(d, space, device=0))


@pytest.mark.parametrize("key", R.RECENT, ids=lambda key: H.history_tag(*key))
def test_recent_history_equals_the_model_at_every_step(key):
    """Binary vectors, geo columns, attribute statistics and hybrid search on one handle with every mutation of the wide wave
    (tests/history_recent_helpers.py): the bits pool regrown, repacked and reset, rows rewritten at another width, hybrid on
    the filter route and at paged depths across compactions, ``geo_nearest`` and ``where_ordered`` in one workspace,
    ``attr_stats`` at a small ``max_groups`` after a large one, masked calls before unmasked ones."""
    seed, space, d, _ = key
    print(f"history {H.history_tag(*key)}: distance bar {R.geo_bar(*key):.3e}")
    _replay(key, lambda: HipScanEngine(d, space, device=0))


def test_an_index_outlives_a_destroyed_neighbour_that_used_the_recent_workspaces():
    """Engine B is opened first; engine A replays the first recent history -- the hybrid, bits, statistics and ordering
    workspaces among the rest -- and is closed, which frees all of it; then B replays the second one and equals the model at
    every step."""
    key_a, key_b = R.RECENT[0], R.RECENT[1]
    ops_a, expected_a = H.make_history(*key_a)
    ops_b, expected_b = H.make_history(*key_b)
    b = HipScanEngine(key_b[2], key_b[1], device=0)
    try:
        a = HipScanEngine(key_a[2], key_a[1], device=0)
        try:
            assert H.run_history(a, ops_a, expected_a, "neighbour_" + H.history_tag(*key_a))["steps"] == len(ops_a)
        finally:
            a.close()
        assert H.run_history(b, ops_b, expected_b, "survivor_" + H.history_tag(*key_b))["steps"] == len(ops_b)
    finally:
        b.close()


@pytest.mark.parametrize("key", R.RECENT_LARGE, ids=lambda key: H.history_tag(*key))
def test_recent_large_history_moves_the_dense_leg_of_hybrid_between_the_routes(key):
    """Past 32,768 rows `auto` itself takes the filter route inside ``search_hybrid`` at nq = 12 and 40 with fetch_dense <= 64;
    fetch_dense = 65 and 1024 on each side; a ``tombstone_where`` of about a third of the rows through a geo box and a
    compaction bring it back; growth again."""
    seed, space, d, _ = key
    print(f"history {H.history_tag(*key)}: distance bar {R.geo_bar(*key):.3e}")
    _replay(key, lambda: HipScanEngine(d, space, device=0))
