"""The radix Partition (csrc/vdl_partition.hip) where its look-back uses the upper levels of its tree of status rows.  A tile of a pass
is T = 8192 rows; tile 255 is the first to store a level-2 row (n >= 256 T = 2 097 152 rows) and tile 4095 the first to store a
level-3 row (n >= 4096 T = 33 554 432); from there on the prefix of a tile is made of rows of three and four levels
(fen_prefix_row) and the 30- and 45-row sums of add_rows run.  Levels 3 to 5 of the index arithmetic alone:
tests/test_partition_index_cpu.py.

Every program is the GROUP BY idiom around one Partition (tests/level_cases.py: partition_program) and runs in four forms: as
built, VDL_NO_PACKED_PARTITION=1 (key and slot travel as two words), VDL_PART_WIDE_STATUS=1 (the 64-bit status words and destinations
that a Partition of 2^31 rows would take) and both.  The keys are in random order, so the sortedness check in front of a multi-pass
Partition (vdl_genexec.h: partition_positions) finds a descent and the radix passes run.

Reference: up to 512 T rows a stable argsort of the pivot buckets in numpy, tied to the oracle at 256 T + 1 rows here and at small
sizes in tests/test_level_cases_cpu.py; at level 3 the three O(n) properties that leave one answer (level_cases.stable_partition_error)."""
import numpy as np
import pytest

import level_cases as lc
from helpers import engine_with, oracle_run
from level_cases import T

pytestmark = pytest.mark.gpu

SWITCHES = ("VDL_NO_PACKED_PARTITION", "VDL_PART_WIDE_STATUS", "VDL_NO_SORTED_SHORTCUT", "VDL_NO_SPARSE", "VDL_SPARSE_ALWAYS")
FORMS = ((), ("VDL_NO_PACKED_PARTITION",), ("VDL_PART_WIDE_STATUS",), ("VDL_NO_PACKED_PARTITION", "VDL_PART_WIDE_STATUS"))
PMIN, PCOUNT = 1000, 1 << 30
N1 = 0x111 * T + 777


def switch(monkeypatch, on):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k in on:
        monkeypatch.setenv(k, "1")


def run_forms(monkeypatch, cols, programs, ref, forms=FORMS, also=()):
    """every program (text, named outputs) in every form: each output equals the reference"""
    e = engine_with(cols)
    try:
        for text, named in programs:
            for form in forms:
                switch(monkeypatch, form + tuple(also))
                p = e.parse(text)
                res = p.run(as_numpy=True)["results"]
                bad = lc.mismatches(res, named, ref)
                p.close()
                assert not bad, (form, also, sorted(named), bad)
    finally:
        e.close()


def keys_for(mode, rng, n, pmin=PMIN, pcount=PCOUNT):
    keys = rng.integers(pmin, pmin + pcount, n)
    if mode == "c":                       # below the first pivot (bucket 0, with the keys equal to pmin) and beyond the last (bucket pcount)
        k = max(n // 50, 3)
        keys[rng.integers(0, n, k)] = rng.integers(pmin - 10 ** 6, pmin + 1, k)
        keys[rng.integers(0, n, k)] = rng.integers(pmin + pcount, pmin + pcount + 10 ** 6, k)
        keys[[1, n // 2, n - 2]] = [np.iinfo(np.int64).min + 3, np.iinfo(np.int64).max - 3, pmin]
    return keys


@pytest.mark.parametrize("mode", ["a", "b", "c"])
@pytest.mark.parametrize("n", [256 * T, 256 * T + 1, N1, 0x1FF * T + T - 1, 0x200 * T + 5])
def test_partition_at_level_two(n, mode, monkeypatch):
    """256 to 513 tiles: tile 255 (and 511) stores a level-2 row, later tiles read it; the last tile is full, holds one row, 777, T - 1
    and 5 rows.  Keys uniform over a domain of 2^30 (four passes, packed), no EPS rows, random order.
    (a) the positions are an output: the last pass writes pos[slot] = rank (MODE 2; launch_partition: mode = last ? 2 : 0);
    (b) only Scatters read the Partition and every key lies inside the pivots: partition_positions takes `lazy` and `sorted_keys`, the
        last pass stores the slots -- and the key values -- in rank order (MODE 1);
    (c) as (b) with keys below pmin and beyond pmin + pcount (buckets 0 and pcount): `values_inside` fails, MODE 1 without sorted_keys."""
    rng = np.random.default_rng(n + ord(mode))
    keys = keys_for(mode, rng, n)
    vals = rng.integers(-10 ** 9, 10 ** 9, n)
    cols = lc.partition_cols(keys, vals, rng)
    ref = lc.partition_reference(keys, vals, None, PMIN, PCOUNT)
    program = lc.partition_program(PMIN, PCOUNT, False, positions=(mode == "a"))
    if n == 256 * T + 1:                  # the reference itself, against the oracle
        want = oracle_run(program[0], cols)
        assert not lc.mismatches(want, program[1], ref)
    run_forms(monkeypatch, cols, [program], ref)


def _shape(shape, rng, n):
    """-> (keys, pmin, pcount, switches that the shape needs)"""
    if shape == "every key equal":        # (in order as it stands: only with the shortcut off does it reach the passes, all of its rows in one digit of every pass)
        return np.full(n, PMIN + 123456, np.int64), PMIN, PCOUNT, ("VDL_NO_SORTED_SHORTCUT",)
    if shape == "constant in every aligned 64 rows":
        return np.repeat(rng.integers(PMIN, PMIN + PCOUNT, (n + 63) // 64), 64)[:n], PMIN, PCOUNT, ()
    if shape == "strictly descending":
        return PMIN + 7 + 3 * np.arange(n, dtype=np.int64)[::-1], PMIN, PCOUNT, ()
    if shape == "constant low byte":
        return PMIN + ((rng.integers(0, PCOUNT >> 8, n) << 8) | 0x5A), PMIN, PCOUNT, ()
    if shape == "domain of 200":
        return rng.integers(0, 200, n), 0, 200, ()
    if shape == "domain of 2^38":
        return rng.integers(0, 1 << 38, n), 0, 1 << 38, ()
    if shape == "domain of 2^45":
        return rng.integers(0, 1 << 45, n), 0, 1 << 45, ()
    assert shape == "declared 2^40, keys below 2^10"
    return rng.integers(0, 1 << 10, n), 0, 1 << 40, ()


@pytest.mark.parametrize("shape", ["every key equal", "constant in every aligned 64 rows", "strictly descending", "constant low byte", "domain of 200",
                                   "domain of 2^38", "domain of 2^45", "declared 2^40, keys below 2^10"])
def test_partition_key_shapes_at_level_two(shape, monkeypatch):
    """273 tiles and 777 rows, positions materialised and then read by Scatters only.
    every key equal / constant in every aligned 64 rows: part_count's wave-uniform branch (lane 0 adds the wave's 64 at once), one digit
    holds a whole tile; strictly descending: every tile's rows go to other digits than its predecessor's; constant low byte: the first
    pass moves nothing.  domain of 200: bits <= 8, ONE pass, which is first and last (k_part_pass<FIRST, unpacked, MODE 2>); 2^38: five
    passes; 2^45: 45 + 22 bits do not fit a word (launch_partition: slot_bits = 0), six unpacked passes; declared 2^40 with keys below
    2^10: the sortedness pass reports the largest key and max_bucket cuts five passes to two."""
    rng = np.random.default_rng(len(shape))
    keys, pmin, pcount, also = _shape(shape, rng, N1)
    vals = rng.integers(-10 ** 9, 10 ** 9, N1)
    ref = lc.partition_reference(keys, vals, None, pmin, pcount)
    run_forms(monkeypatch, lc.partition_cols(keys, vals, rng), [lc.partition_program(pmin, pcount, False, True), lc.partition_program(pmin, pcount, False, False)],
              ref, also=also)


@pytest.mark.parametrize("case", ["domain of 200, one row in three EPS", "domain of 200 over 600 tiles, one row in three EPS", "every other row EPS",
                                  "valid rows in the first 10 tiles only"])
def test_partition_with_eps_rows_at_level_two(case, monkeypatch):
    """EPS rows (FoldSelect -> Gather in front): the first pass reads the validity bitmap and takes no full-tile body
    (k_part_pass: !(FIRST && in.valid)), the later passes learn the number of rows from the device (n_dev) and the blocks beyond it
    return at once.  A domain of 200 (one pass) with one row in three EPS, over 273 tiles and 777 rows and over 600 tiles; 600 tiles with
    every other row EPS (the later passes run on 300 tiles, still level 2); 600 tiles with valid rows in the first 10 only.  Each as
    the engine chooses -- a selection may be partitioned as its compacted entries, which are fewer tiles -- and with VDL_NO_SPARSE as a
    dense vector with a bitmap over all of its tiles."""
    rng = np.random.default_rng(len(case))
    n = N1 if case == "domain of 200, one row in three EPS" else 600 * T
    pmin, pcount = (0, 200) if case.startswith("domain") else (PMIN, PCOUNT)
    keys = keys_for("a", rng, n, pmin, pcount)
    vals = rng.integers(-10 ** 9, 10 ** 9, n)
    if case.startswith("domain"):
        flags = rng.integers(0, 3, n) != 0
    elif case.startswith("every other"):
        flags = np.arange(n) % 2 == 0
    else:
        flags = (rng.integers(0, 10, n) < 7) & (np.arange(n) < 10 * T)
    ref = lc.partition_reference(keys, vals, flags, pmin, pcount)
    cols = lc.partition_cols(keys, vals, rng, flags)
    programs = [lc.partition_program(pmin, pcount, True, True), lc.partition_program(pmin, pcount, True, False)]
    run_forms(monkeypatch, cols, programs, ref)
    run_forms(monkeypatch, cols, programs[:1], ref, also=("VDL_NO_SPARSE",))


# ---- level 3 -----------------------------------------------------------------------------------------------------------------------
def _level_three(monkeypatch, n, keys, vals, flags, positions):
    """as built: the properties that make the positions the stable partition, then every output from the order they imply; then
    VDL_PART_WIDE_STATUS=1: the same arrays again"""
    rng = np.random.default_rng(3)
    bucket = lc.buckets(keys, 0, PCOUNT)
    text, named = lc.partition_program(0, PCOUNT, flags is not None, positions, sorted_rows=not positions)
    e = engine_with(lc.partition_cols(keys, vals, rng, flags))
    try:
        switch(monkeypatch, ())
        p = e.parse(text)
        res = p.run(as_numpy=True)["results"]
        first = {name: lc.out(res, node) for name, node in named.items()}
        p.close()
        if positions:
            slots = first.get(lc.SLOTS)
            err = lc.stable_partition_error(bucket, flags, pos=first[lc.POS], slots=slots)
            assert err is None, err
            order = np.empty(len(first[lc.POS]), np.int64)
            order[first[lc.POS]] = np.arange(n) if slots is None else slots
        else:                                                      # the value column is the row number: scattered, it IS the order
            order = first[lc.SVAL]
            err = lc.stable_partition_error(bucket, flags, order=order)
            assert err is None, err
        ref = lc.outputs_from_order(keys, vals, order)
        del bucket, order
        bad = [name for name in named if name in ref and not np.array_equal(first[name], ref[name])]
        assert not bad, bad
        del ref
        switch(monkeypatch, ("VDL_PART_WIDE_STATUS",))
        p = e.parse(text)
        res = p.run(as_numpy=True)["results"]
        bad = [name for name, node in named.items() if not np.array_equal(lc.out(res, node), first[name])]
        p.close()
        assert not bad, ("VDL_PART_WIDE_STATUS", bad)
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["a", "b"])
def test_partition_at_level_three(mode, monkeypatch):
    """4097 tiles and 5 rows, keys uniform in 2^30 in random order: tile 4095 stores the first level-3 row and tile 4096 reads it.
    (a) positions materialised (MODE 2); (b) read by Scatters only, keys inside the pivots (MODE 1 with sorted_keys)."""
    n = 4097 * T + 5
    rng = np.random.default_rng(40 + ord(mode))
    keys = rng.integers(0, PCOUNT, n)
    vals = rng.integers(-10 ** 9, 10 ** 9, n) if mode == "a" else np.arange(n, dtype=np.int64)
    _level_three(monkeypatch, n, keys, vals, None, positions=(mode == "a"))


def test_partition_with_eps_rows_at_level_three(monkeypatch):
    """4700 tiles with one row in eight EPS: 4112 tiles of valid rows, so the later passes reach level 3 as well while the blocks
    beyond n_dev return early; the FoldSelect in front compacts over 9400 tiles of 4096 rows, two trips of k_scan_counts."""
    n = 4700 * T
    rng = np.random.default_rng(47)
    keys = rng.integers(0, PCOUNT, n)
    vals = rng.integers(-10 ** 9, 10 ** 9, n)
    _level_three(monkeypatch, n, keys, vals, np.arange(n) % 8 != 3, positions=True)
