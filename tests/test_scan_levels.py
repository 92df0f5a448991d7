"""The single-block scans behind compactions and prefix sums where they take a second trip, and the fused sortedness pass where its
blocks loop and its arrival counters fill (csrc/vdl_ops.hip: k_scan_counts, launch_compact_offsets; csrc/vdl_partition.hip:
launch_prefix_sum, k_sorted_heads_counted).

A compaction tile is 4096 slots.  launch_compact_offsets counts and scans in one launch up to 64 tiles (262 144 slots) and in two
beyond; k_scan_counts takes 8 x 1024 counts per trip and carries their sum into the next, so a second trip needs more than 8192
tiles (33 554 432 slots); launch_prefix_sum scans its block sums with the same kernel.  k_sorted_heads_counted runs at most 2048
blocks: beyond 8 388 608 rows a block takes several tiles and the last block's scan, 8 x 256 counts per trip, takes a second trip;
the blocks' arrivals are gathered on 64 counters (fewer blocks than counters, as many, more).  tests/test_partition_index_cpu.py guards
these constants.  References are numpy statements (tests/level_cases.py), tied to the oracle in tests/test_level_cases_cpu.py."""
import numpy as np
import pytest

import level_cases as lc
from helpers import engine_with
from level_cases import CT

pytestmark = pytest.mark.gpu

TWO_TRIPS = 8192 * CT            # 33 554 432 slots: the last size one trip of k_scan_counts serves


def _run(e, text):
    p = e.parse(text)
    try:
        return p.run(as_numpy=True)["results"]
    finally:
        p.close()


# ---- compaction ---------------------------------------------------------------------------------------------------------------------
def _flags(density, n, rng):
    if density == "all":
        return np.ones(n, np.int8)
    if density == "none in the first trip":
        f = np.zeros(n, np.int8)
        f[TWO_TRIPS:] = 1
        return f
    return (rng.integers(0, 3, n) == 0).astype(np.int8)


def _compaction(n, density):
    rng = np.random.default_rng(n % 100003 + len(density))
    f = _flags(density, n, rng)
    a = rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    text, named = lc.compact_program()
    e = engine_with({"t.f": f, "t.a": a})
    try:
        res = _run(e, text)
    finally:
        e.close()
    slots = np.flatnonzero(f)
    assert np.array_equal(lc.out(res, named["slots"]), slots)
    assert np.array_equal(lc.out(res, named["picked"]), a[slots].astype(np.int64))


@pytest.mark.parametrize("density", ["all", "one in three"])
@pytest.mark.parametrize("n", [64 * CT, 64 * CT + 1])
def test_compaction_in_one_launch_and_in_two(n, density):
    """262 144 slots are 64 tiles, the last size k_compact_count_scan serves (launch_compact_offsets: nb <= kWave); one slot more takes
    k_compact_count and k_scan_counts.  FoldSelect -> Gather -> MaterializeCompact over an int8 flag and an int32 value column."""
    _compaction(n, density)


@pytest.mark.parametrize("density", ["all", "none in the first trip", "one in three"])
@pytest.mark.parametrize("n", [TWO_TRIPS, TWO_TRIPS + 1, TWO_TRIPS + 3 * CT + 17])
def test_compaction_beyond_one_trip_of_the_scan(n, density):
    """8192 tiles fill one trip of k_scan_counts exactly; one slot more, and three tiles and 17 slots more, start a second trip whose
    offsets begin at `carry`, the total of the first.  Every slot selected (the carry is 33 554 432), nothing selected in the first
    trip (the carry is 0 and everything comes from the second), one slot in three."""
    _compaction(n, density)


# ---- launch_prefix_sum ----------------------------------------------------------------------------------------------------------------
def test_foldselect_over_general_runs_beyond_one_trip_of_the_scan():
    """One FoldSelect over general runs (vdl_genexec.h: fold_select_runs) with more than 33 554 432 non-EPS control slots: the run numbers
    are a launch_prefix_sum over the run heads, whose 8192 + block sums take two trips of k_scan_counts; the stable Partition behind
    it runs over as many entries.  Runs of one to a few slots, a stretch of runs of thousands and one run of half a million slots that
    crosses the end of the first trip; a few hundred EPS slots in the control.
    Reference: the numpy statement of the rule (level_cases.general_select_reference), which tests/test_level_cases_cpu.py compares with
    the oracle at 40 000 slots -- the oracle hands its results over as Python lists, minutes at this size."""
    rng = np.random.default_rng(12)
    n = TWO_TRIPS + 3 * CT + 17 + 1000
    heads = rng.random(n) < 0.3
    heads[5_000_000:9_000_000] &= rng.random(4_000_000) < 0.001
    heads[TWO_TRIPS - 300_000:TWO_TRIPS + 200_000] = False
    ctl = (np.cumsum(heads) % 1000).astype(np.int32)
    flags = np.ones(n, np.int8)
    flags[rng.integers(0, n, 500)] = 0
    flags[[0, 63, 64, 4095, 4096, TWO_TRIPS - 1, TWO_TRIPS, n - 1]] = 0
    assert int(flags.sum()) > TWO_TRIPS
    data = rng.integers(0, 3, n).astype(np.int8)
    text, named = lc.general_select_program()
    e = engine_with({"t.c": ctl, "t.f": flags, "t.d": data})
    try:
        res = _run(e, text)
    finally:
        e.close()
    slots, values = lc.general_select_reference(ctl, flags != 0, data)
    assert np.array_equal(lc.out(res, named["hits"]), values)
    assert np.array_equal(lc.out(res, named["offset"]), slots - values)
    assert np.array_equal(lc.out(res, named["data"]), data[values].astype(np.int64))


# ---- the fused sortedness pass --------------------------------------------------------------------------------------------------------
SHAPES = ["distinct", "runs of 7", "one run", "descent at the end", "descent at a multiple of 256", "descent at row 4096 x 1000"]
DOMAIN = 1 << 40                 # five passes as declared: the Partition looks for order first (partition_positions: partition_passes(pcount) > 1)


def _keys(n, shape):
    if shape == "descent at a multiple of 256":
        return lc.sorted_keys(n, "distinct", descent_at=256 * max(n // 512, 1))
    if shape == "descent at row 4096 x 1000":
        return lc.sorted_keys(n, "distinct", descent_at=CT * 1000)
    return lc.sorted_keys(n, shape)


def _group_by(monkeypatch, n, shapes):
    rng = np.random.default_rng(n % 100003)
    vals = rng.integers(-10 ** 9, 10 ** 9, n)
    text, named = lc.group_by_program(DOMAIN)
    for shape in shapes:
        keys = _keys(n, shape)
        ref = lc.group_by_reference(keys, vals)
        e = engine_with({"t.k": keys, "t.v": vals})
        try:
            for off in (False, True):
                if off:
                    monkeypatch.setenv("VDL_NO_DENSE_HEADS", "1")
                else:
                    monkeypatch.delenv("VDL_NO_DENSE_HEADS", raising=False)
                res = _run(e, text)
                bad = [name for name, node in named.items() if not np.array_equal(lc.out(res, node), ref[name])]
                assert not bad, (shape, "VDL_NO_DENSE_HEADS" if off else "as built", bad)
        finally:
            e.close()


@pytest.mark.parametrize("n", [63 * CT, 63 * CT + 1, 64 * CT, 64 * CT + 1, 65 * CT, 65 * CT + 1, 129 * CT + 1])
def test_sortedness_pass_around_its_arrival_counters(n, monkeypatch):
    """GROUP BY over an int64 key without EPS rows and a multi-pass domain: k_sorted_heads_counted with 63, 64, 65, 66 and 130 blocks --
    fewer blocks than arrival counters (groups = gridDim.x, one member each), as many, more (counters with two and three members).
    Keys in order (distinct, runs of 7, one run): the folds take the run heads, the tiles' offsets and the number of groups from the
    pass, so a wrong scan of the tile counts shows in them.  One descent (last row, a multiple of 256 where lane 0 reads its left
    neighbour from memory): the verdict, and the fall-through to the radix passes.  Each also with VDL_NO_DENSE_HEADS=1
    (k_sorted_heads, k_compact_count, k_scan_counts instead of the one launch)."""
    _group_by(monkeypatch, n, SHAPES[:5])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [2048 * CT, 2048 * CT + 1, 4097 * CT + 300])
def test_sortedness_pass_beyond_its_largest_grid(n, shape, monkeypatch):
    """2048 tiles are the largest grid with one tile per block; one row more and 4097 tiles + 300 rows make blocks loop over tiles
    (t += gridDim.x) and the last block's scan carry a total across trips of 2048 counts.  The descent at row 4096 x 1000 sits on a
    tile's first row."""
    _group_by(monkeypatch, n, [shape])
