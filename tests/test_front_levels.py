"""The one-pass fused front (csrc/vdl_mscan_body.h: project_front_body) where its look-back uses the upper levels of its tree.  A batch
is FRONT_BATCH x T = 4 x 2048 = 8192 rows; the tree is of fan-out 16 over batches (csrc/vdl_front_index.h).  Batch 15 is the first to
store a level-1 node and batch 16 the first to read one (17 batches, 131 073 rows); batch 255 stores the first level-2 node, batch 256
reads it (257 batches, 2 097 153 rows); batch 4095 stores the first level-3 node, batch 4096 reads it (4097 batches, 33 554 433 rows).
Levels 4 to 6 and the prefix walk's second trip: tests/test_front_index_cpu.py, on the host.

The programs, the survivor patterns -- functions of the batch number, so that a node missing from or doubled in a prefix moves
survivors visibly --, the numpy reference and the comparison are tests/front_cases.py; tests/test_front_cases_cpu.py ties the
reference to the oracle and shows what the comparison rejects.  Every case asserts that the plan has its fused front, that EVERY output
equals the reference -- the front's own vectors (row ids, f.k, f.v, d.g[f.k] of the survivors in row order) value for value -- and that
the run's timings name the front with numpy's number of survivors.

How long the output vectors are (vdl_engine.cpp: run_projection).  A plan's first run takes the whole table's length when
n x 8 x (outputs + 1) <= 2^28 bytes and else counts first (capacity 0: nothing is fetched or written) and runs again with the exact
number.  The number of outputs is read from each plan's description (front_cases.front_output_columns) and the path asserted from it
before the run.  Program A's front has 2 output columns beside the row ids (24 bytes a row: the whole table up to 11 184 810 rows), program B's
3 (32 bytes: 8 388 608 rows): levels 1 and 2 take the whole table, level 3 (33.5 M rows) counts first.  From the second run on the
capacity is min(n, m + m / 8 + 4096) for the m survivors seen last time; a run that finds more repeats the pass with the exact number."""
import numpy as np
import pytest

import front_cases as fc
from front_cases import B, T
from helpers import engine_with

pytestmark = pytest.mark.gpu

FIRST_RUN_BYTES = 1 << 28              # (tests/test_front_cases_cpu.py guards it)


def counts_first(n, outputs):
    return n * 8 * (outputs + 1) > FIRST_RUN_BYTES


def later_capacity(n, m):
    return min(n, m + m // 8 + 4096)


def check(p, named, ref, n, what):
    r = p.run(as_numpy=True)
    got = fc.outputs(r["results"], named)
    del r["results"]
    bad = fc.front_mismatches(got, ref)
    assert not bad, (what, bad, {name: (len(got[name]), len(ref[name])) for name in bad})
    assert fc.kept_note(r["timings"], len(ref[fc.ROWS]), n), (what, sorted(r["timings"]))


def run_patterns(size, dimension_filter, jit, patterns, first_run_counts):
    """a fresh plan per pattern (a first run each), every output against the reference.  first_run_counts: whether, by the number of
    output columns the plan's description shows and the table's length, such a first run counts first (capacity 0, then the exact
    number) or takes the whole table's length as its capacity"""
    n = fc.rows_of(*size)
    text, named = fc.front_program(dimension_filter)
    e = None
    try:
        for pattern in patterns:
            cols = fc.fact_columns(fc.pattern_mask(pattern, n), dimension_filter, seed=len(pattern))
            if e is None:
                e = engine_with(cols)
            else:
                for name in ("f.a", "f.k", "f.v"):
                    e.upload(name, cols[name])
            ref = fc.front_reference(cols, dimension_filter)
            p = e.parse(text)
            if jit:
                p.set_jit(True)
            d = p.describe()
            assert "fused front" in d
            assert fc.front_output_columns(d) == (3 if dimension_filter else 2), d
            assert counts_first(n, fc.front_output_columns(d)) == first_run_counts, (size, fc.front_output_columns(d))
            check(p, named, ref, n, (size, pattern))
            p.close()
            del ref, cols
    finally:
        if e is not None:
            e.close()


# one count of each level also with a partial last tile (+1 row, +T-1 rows) and one with a last batch of 1, 2 and 3 tiles
LEVEL_ONE = [(15, 0, 0), (16, 0, 0), (17, 0, 0), (17, 0, 1), (17, 0, T - 1), (16, 1, 0), (16, 2, 0), (16, 3, 0)]
LEVEL_TWO = [(255, 0, 0), (256, 0, 0), (257, 0, 0), (0x111, 0, 0), (257, 0, 1), (257, 0, T - 1), (256, 1, 0), (256, 2, 0), (256, 3, 0)]
LEVEL_THREE = [(4095, 0, 0), (4096, 0, 0), (4097, 0, 0), (0x1111, 0, 0), (4097, 0, 1), (4097, 0, T - 1)]


@pytest.mark.parametrize("jit", [False, True], ids=["precompiled", "specialised"])
@pytest.mark.parametrize("dimension_filter", [False, True], ids=["A", "B"])
@pytest.mark.parametrize("size", LEVEL_ONE, ids=str)
def test_front_at_level_one(size, dimension_filter, jit):
    """15, 16 and 17 batches (batch 16 reads the level-1 node of batches 0 .. 15), 17 with a partial last tile, 16 with a last batch of
    1, 2 and 3 tiles; every pattern, each as the first run of a fresh plan (capacity: the whole table)"""
    run_patterns(size, dimension_filter, jit, fc.PATTERNS, first_run_counts=False)


@pytest.mark.parametrize("jit", [False, True], ids=["precompiled", "specialised"])
@pytest.mark.parametrize("dimension_filter", [False, True], ids=["A", "B"])
@pytest.mark.parametrize("size", LEVEL_TWO, ids=str)
def test_front_at_level_two(size, dimension_filter, jit):
    """255, 256, 257 and 0x111 batches (batch 256 reads the level-2 node of batches 0 .. 255; batch 0x110 one node of each of levels 2, 1
    and none of level 0, batch 0x111 one of each), 257 with a partial last tile, 256 with a last batch of 1, 2 and 3 tiles; every
    pattern, each as the first run of a fresh plan (capacity: the whole table)"""
    run_patterns(size, dimension_filter, jit, fc.PATTERNS, first_run_counts=False)


@pytest.mark.parametrize("pattern", ["signature", "isolated", "full head"])
@pytest.mark.parametrize("size", LEVEL_THREE, ids=str)
def test_front_at_level_three(size, pattern):
    """4095, 4096, 4097 and 0x1111 batches (batch 4096 reads the level-3 node of batches 0 .. 4095), 4097 with a partial last tile;
    program A, precompiled, the first run of a fresh plan: it counts first with capacity 0 and runs again with the exact number"""
    run_patterns(size, False, False, [pattern], first_run_counts=True)


def test_front_at_level_three_with_every_row_kept():
    """4097 batches and 5 rows, every row survives: node values reach n, every batch overflows the carry area"""
    run_patterns((4097, 0, 5), False, False, ["all"], first_run_counts=True)


def test_front_at_level_three_specialised():
    run_patterns((4097, 0, 5), False, True, ["signature"], first_run_counts=True)


# ---- the guessed capacity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batches", [257, 4097])
def test_front_guesses_its_capacity_from_the_last_run_across_levels(batches):
    """One plan over data that changes under it: `signature` (the first run), `all` (the guess of m / 8 + 4096 more is short: the pass is
    repeated with the exact number), `none`, `isolated`, `signature` again (at 4097 batches the guess from `isolated`'s few rows is short again)."""
    n = fc.rows_of(batches, 0, 5)
    text, named = fc.front_program(False)
    cols = fc.fact_columns(fc.pattern_mask("signature", n), False)
    e = engine_with(cols)
    try:
        p = e.parse(text)
        assert "fused front" in p.describe()
        assert counts_first(n, fc.front_output_columns(p.describe())) == (batches == 4097)      # (the first run's path)
        seen = None
        for pattern in ("signature", "all", "none", "isolated", "signature"):
            mask = fc.pattern_mask(pattern, n)
            cols["f.a"] = fc.fact_a(mask, False)
            m = int(mask.sum())
            if pattern == "all" or (pattern == "signature" and seen is not None and batches == 4097):
                assert m > later_capacity(n, seen), "this run was to find its guess short"
            del mask
            e.upload("f.a", cols["f.a"])
            ref = fc.front_reference(cols, False)
            check(p, named, ref, n, pattern)
            del ref
            seen = m
    finally:
        e.close()


def _exactly(n, total, last):
    """a mask with `total` survivors of which the last batch holds `last` (its first rows), the others spread evenly over the batches before it"""
    start = (fc.batches_of(n) - 1) * B
    mask = np.zeros(n, bool)
    mask[start:start + last] = True
    mask[np.linspace(0, start - 1, total - last).astype(np.int64)] = True
    assert int(mask.sum()) == total and int(mask[start:].sum()) == last
    return mask


@pytest.mark.parametrize("over,last", [(0, 3), (1, 1), (1, 5)], ids=["m equals the capacity", "one above: the last batch begins at the capacity", "one above: the last batch crosses the capacity"])
def test_front_at_the_edge_of_its_guessed_capacity(over, last):
    """257 batches.  After a run that kept m0 rows the capacity is c = m0 + m0 / 8 + 4096.  A run that keeps exactly c rows fits; one
    that keeps c + 1 is repeated -- with the last batch holding the one row beyond (its offset IS the capacity: `off < out_cap` fails)
    or five rows of which the last is beyond (`off + k >= out_cap` stops that one lane)."""
    n = fc.rows_of(257, 0, 5)
    text, named = fc.front_program(False)
    mask = fc.pattern_mask("signature", n)
    cols = fc.fact_columns(mask, False)
    e = engine_with(cols)
    try:
        p = e.parse(text)
        check(p, named, fc.front_reference(cols, False), n, "first run")
        cap = later_capacity(n, int(mask.sum()))
        assert cap < (fc.batches_of(n) - 1) * B // 2                # (room to spread the survivors without two on one row)
        cols["f.a"] = fc.fact_a(_exactly(n, cap + over, last), False)
        e.upload("f.a", cols["f.a"])
        ref = fc.front_reference(cols, False)
        assert len(ref[fc.ROWS]) == cap + over
        check(p, named, ref, n, "second run")
    finally:
        e.close()


# ---- the kernel's other instantiations -----------------------------------------------------------------------------------------------
def _variant(extra_filters, extra_takes, shifted):
    n = fc.rows_of(257, 0, 5)
    mask = fc.pattern_mask("signature", n)
    cols = dict(fc.fact_columns(mask, False), **fc.variant_columns(n, extra_filters, extra_takes))
    text, named = fc.front_program(False, extra_filters, extra_takes)
    ref = fc.front_reference(cols, False, extra_takes)
    keep = []
    if shifted:
        import torch
        import mplan2vdl_amd as m

        e = m.Engine(device=0)
        for name, v in cols.items():
            t = torch.from_numpy(np.concatenate((v[:1], v))).cuda()
            keep.append(t)
            e.register_tensor(name, t[1:])                          # shifted by one element: misaligned for the 2-row loads
    else:
        e = engine_with(cols)
    try:
        p = e.parse(text)
        d = p.describe()
        assert "fused front" in d
        check(p, named, ref, n, (extra_filters, extra_takes, shifted))
        return d
    finally:
        e.close()


def test_front_over_misaligned_columns_at_level_two():
    """columns registered as torch tensors shifted by one element: the instantiation without vector loads (VEC = false)"""
    _variant(0, 0, True)


@pytest.mark.parametrize("extra_filters,deciding", [(5, 6), (9, 10)])
def test_front_with_more_deciding_columns_at_level_two(extra_filters, deciding):
    """5 - 8 and 9 - 12 deciding columns (further int8 columns with range filters that every row passes): NCS = 8 and 12"""
    d = _variant(extra_filters, 0, False)
    assert fc.front_column_counts(d)[0] == deciding, d


def test_front_with_more_take_side_columns_at_level_two():
    """more than 12 columns on the take side (4 deciding ones, f.k, f.v and 7 further fact columns that are outputs -- a front hands over
    at most kMaxProjOuts = 10 vectors --): NCS = 4, NCT = kMaxVCols"""
    d = _variant(3, 7, False)
    assert fc.front_column_counts(d) == (4, 13), d
