"""The engine at the ends of int64: the directed programs of tests/int64_edge_cases.py (values near +-2^63, positions at and
beyond 2^31 / 2^32, sums that wrap) through the engine as planned, with fusion off and under every executor switch that bears
on the family.  The engine's results must equal the Python model's (tests/vdl_model.py), and so must the oracle's: all three
bit for bit, no tolerances.  Sizes are the smallest at which the kernels' units come into play: 1, 65, 4097 (one more than a
compaction tile), 8193 (one more than a Partition tile), 4351 where a wide-load kernel needs 4096 rows and a tail."""
import numpy as np
import pytest

import int64_edge_cases as cases
import mplan2vdl_amd as m
from mplan2vdl_amd import _lib
import vdl_model as model
from helpers import check_against_oracle, engine_with, oracle_run
from test_int64_edges_cpu import pool_program, same
from vdl_model import I64_MAX, I64_MIN

pytestmark = pytest.mark.gpu

SPARSE = ["VDL_NO_SPARSE", "VDL_SPARSE_ALWAYS"]
EXPR = ["VDL_NO_EXPR_FUSION", "VDL_NO_PRED_FUSION", "VDL_NO_SPARSE_EXPR"]
FILTER = ["VDL_NO_FILTER_FUSION", "VDL_NO_WIDE_FILTER"]
GROUP = ["VDL_NO_SORTED_SHORTCUT", "VDL_NO_GROUP_BATCH", "VDL_NO_PACKED_PARTITION", "VDL_NO_DENSE_HEADS"]
SIZES = [1, 65, 4097]


def run_everywhere(monkeypatch, name, built, switches=(), jit=False, images=False):
    """model == oracle, then one engine: as planned, without fusion, under each switch (and, for fused scans, specialised /
    without the columns' images).  Returns the timing labels of the run as planned."""
    text, cols = built
    want = model.run(text, cols)
    same(name, text, cols, oracle_run(text, cols), want)
    e = engine_with(cols)
    labels = None
    try:
        if images:
            for k in cols:
                e.encode(k)
        modes = [("planned", None), ("unfused", None)] + [(s, s) for s in switches]
        modes += [("specialised", None), ("specialised_rtb", None)] if jit else []
        modes += [("no_images", None)] if images else []
        for mode, env in modes:
            if env:
                monkeypatch.setenv(env, "1")
            e.set_column_images(mode != "no_images")
            p = e.parse(text)
            p.set_fusion(mode != "unfused")
            if mode.startswith("specialised"):
                p.set_jit(True, runtime_bounds=mode.endswith("rtb"))
            try:
                out = p.run()
                if labels is None:
                    labels = list(out["timings"])
                p.close()
                # (the switch is still in force: the report names it and its traced reruns run under it)
                check_against_oracle("int64_edges_%s" % mode, name, text, cols, out["results"], want)
            except AssertionError as exc:
                if mode.startswith("specialised") or images:
                    raise AssertionError("mode %s: the report's traced reruns use the precompiled scans with the images on, so they need "
                                         "not show what this run showed\n%s" % (mode, exc)) from exc
                raise
            finally:
                if env:
                    monkeypatch.delenv(env)
    finally:
        e.close()
    return labels


# ---- a. element-wise operators ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", list(cases.DTYPES))
@pytest.mark.parametrize("n", SIZES)
def test_elementwise_operators(monkeypatch, n, width):
    run_everywhere(monkeypatch, "elementwise_%s_n%d" % (width, n), cases.elementwise(n, width), ["VDL_NO_EXPR_FUSION"])


# ---- b. fused expression trees -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "selection"])
@pytest.mark.parametrize("n", SIZES)
def test_expression_trees_at_every_height_and_past_the_limits(monkeypatch, n, sparse):
    run_everywhere(monkeypatch, "expr_chains_%d_n%d" % (sparse, n), cases.expr_chains(n, sparse), EXPR + SPARSE)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "selection"])
def test_trees_past_a_limit_of_the_fused_kernel_are_split(monkeypatch, capfd, sparse):
    """The values of the trees one past a limit are checked above; this checks that they were split at all, from the executor's
    own account (VDL_TRACE_FORMS: one `split:` line whenever a tree does not fit one kernel and a side of it is run first).
    Every limit that a tree can pass is passed: 13 leaves and depth 9.  The third limit, 48 instructions, cannot be: a tree of L
    leaves holds 2L - 1 instructions, 23 at the most within 12 leaves, and the >= / != idioms only shorten the program -- the
    26-leaf tree of 51 instructions is cut on its leaves as it grows, long before."""
    import re

    text, cols = cases.expr_chains(65, sparse)
    monkeypatch.setenv("VDL_TRACE_FORMS", "1")
    if sparse:
        monkeypatch.setenv("VDL_SPARSE_ALWAYS", "1")
    e = engine_with(cols)
    try:
        capfd.readouterr()
        got = e.run_vdl(text, fuse=False)["results"]
        err = capfd.readouterr().err
    finally:
        e.close()
    check_against_oracle("int64_edges_split", "expr_chains_%d" % sparse, text, cols, got, model.run(text, cols))
    splits = [tuple(int(x) for x in g) for g in re.findall(r"split: (\d+) leaves, (\d+) instructions, depth (\d+) do not fit", err)]
    assert any("entries of a selection" in ln for ln in err.splitlines() if "split:" in ln) == sparse, err[-3000:]
    assert any(lv == 13 and d <= 8 for lv, ins, d in splits), splits              # the leaf limit alone
    assert any(d == 9 and lv <= 12 for lv, ins, d in splits), splits              # the depth limit alone
    assert len(splits) >= 3, splits                                               # ... and the 26-leaf tree, cut as it grows
    assert all(lv > 12 or d > 8 for lv, ins, d in splits), splits                 # and nothing within the limits was split


# ---- c. predicates and filters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_predicate_chains_between_pool_columns(monkeypatch, n):
    run_everywhere(monkeypatch, "predicates_n%d" % n, cases.predicates(n), EXPR + SPARSE + FILTER)


@pytest.mark.parametrize("n", SIZES)
def test_column_filters_with_bounds_at_both_ends(monkeypatch, n):
    run_everywhere(monkeypatch, "column_filters_n%d" % n, cases.column_filters(n), FILTER + SPARSE + ["VDL_NO_PRED_FUSION"])


def test_wide_int32_filter_with_bounds_outside_int32(monkeypatch):
    run_everywhere(monkeypatch, "wide_i32_filters", cases.wide_i32_filters(4351), FILTER + SPARSE)


# ---- d. positions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["i32", "i64"])
@pytest.mark.parametrize("n", SIZES)
def test_positions_outside_the_source(monkeypatch, n, width):
    run_everywhere(monkeypatch, "positions_%s_n%d" % (width, n), cases.positions(n, width), SPARSE + FILTER + ["VDL_NO_RANKED_GATHER"])


@pytest.mark.parametrize("width", ["i32", "i64"])
def test_join_filter_with_foreign_keys_outside_the_dimension(monkeypatch, width):
    run_everywhere(monkeypatch, "join_filter_%s" % width, cases.join_filter(4351, width), SPARSE + FILTER, jit=True)


@pytest.mark.parametrize("n", SIZES)
def test_like_offsets_outside_the_heap(monkeypatch, n):
    run_everywhere(monkeypatch, "like_offsets_n%d" % n, cases.like_offsets(n), SPARSE)


# ---- e. folds ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("holes", ["none", "data", "control", "both"])
@pytest.mark.parametrize("n", SIZES)
def test_folds_over_pool_data_and_pool_controls(monkeypatch, n, holes):
    run_everywhere(monkeypatch, "folds_%s_n%d" % (holes, n), cases.folds(n, holes), SPARSE + ["VDL_NO_GROUP_BATCH", "VDL_NO_DENSE_HEADS"])


# ---- f. Partition ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pmin", cases.PMINS)
@pytest.mark.parametrize("shape", ["shuffled", "sorted", "eps"])
@pytest.mark.parametrize("n", [1, 65, 8193])
def test_partition_by_pivots_at_both_ends(monkeypatch, n, shape, pmin):
    run_everywhere(monkeypatch, "partition_%s_pmin%d_n%d" % (shape, pmin, n), cases.partitions(n, shape, pmin), GROUP + SPARSE)


# ---- g. Semisort -------------------------------------------------------------------------------------------------------------------------------
SPANS = [(0, 5), (255, -255), (256, I64_MIN), (1 << 40, -(1 << 39)), ((1 << 62) - 1, -(1 << 61)), ((1 << 62) - 1, I64_MAX - (1 << 62) + 1)]


@pytest.mark.parametrize("span,low", SPANS)
@pytest.mark.parametrize("n", [1, 65, 8193])
def test_semisort_over_spans_up_to_the_limit(monkeypatch, n, span, low):
    for holes in ("none", "some"):
        run_everywhere(monkeypatch, "semisort_span%d_low%d_%s_n%d" % (span, low, holes, n), cases.semisort(n, span, low, holes), ["VDL_NO_PACKED_PARTITION"])


def test_semisort_of_nothing_and_past_the_limit(monkeypatch):
    for n in (1, 65, 8193):
        run_everywhere(monkeypatch, "semisort_all_eps_n%d" % n, cases.semisort(n, 3, 0, "all"))
    for span, low in ((1 << 62, -(1 << 61)), ((1 << 63) - 1, I64_MIN), ((1 << 64) - 1, I64_MIN)):
        text, cols = cases.semisort(65, span, low, "none")
        same("semisort_span%d_low%d" % (span, low), text, cols, oracle_run(text, cols), model.run(text, cols))
        e = engine_with(cols)
        try:
            with pytest.raises(m.VdlError, match="wider than 2\\^62") as err:
                e.run_vdl(text)
            assert err.value.code == _lib.VDL_ERR_UNSUPPORTED
        finally:
            e.close()


# ---- h. fused scans: a column against a column ----------------------------------------------------------------------------------------------------
def abandoned(labels):
    return [k for k in labels if k.startswith("fusedPlanAbandoned")]


@pytest.mark.parametrize("grouped", [False, True], ids=["global", "grouped"])
@pytest.mark.parametrize("form", ["gt", "lt", "ge"])
@pytest.mark.parametrize("width", ["i32", "i64"])
def test_scans_that_compare_two_columns(monkeypatch, width, form, grouped):
    """the fused scan (precompiled, specialised, bounds at run time, images on and off) reads the difference of two columns for its
    sign: over int32 operands the wrap-around difference, over int64 operands the saturated one -- never given up"""
    for n in (65, 4097):
        labels = run_everywhere(monkeypatch, "compare_scan_%s_%s_%d_n%d" % (width, form, grouped, n), cases.compare_scan(n, width, form, grouped),
                                ["VDL_NO_GROUP_BATCH"], jit=True, images=True)
        assert not abandoned(labels), labels


@pytest.mark.parametrize("width", ["i32", "i64"])
def test_fronts_and_dimension_scans_that_compare_two_columns(monkeypatch, width):
    for n in (65, 4097):
        labels = run_everywhere(monkeypatch, "compare_front_%s_n%d" % (width, n), cases.compare_front(n, width), SPARSE, jit=True, images=True)
        assert not abandoned(labels), labels
        labels = run_everywhere(monkeypatch, "compare_dimension_%s_n%d" % (width, n), cases.compare_dimension(n, width), SPARSE, jit=True, images=True)
        assert not abandoned(labels), labels


@pytest.mark.parametrize("grouped", [False, True], ids=["global", "grouped"])
def test_min_and_max_over_nothing_but_their_identities(monkeypatch, grouped):
    for n in (1, 65, 4097):
        labels = run_everywhere(monkeypatch, "identity_aggregates_%d_n%d" % (grouped, n), cases.identity_aggregates(n, grouped), ["VDL_NO_GROUP_BATCH"], jit=True)
        assert not [k for k in labels if k.startswith("fusedPlanAbandoned")], labels


# ---- the generator of test_random_programs over pool columns ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "VDL_SPARSE_ALWAYS", "VDL_NO_SPARSE"])
def test_random_programs_over_pool_columns(monkeypatch, mode):
    if mode:
        monkeypatch.setenv(mode, "1")
    for seed in range(24):
        text, cols = pool_program(seed, 10 + seed % 30)
        want = model.run(text, cols)
        same("pool_program seed %d" % seed, text, cols, oracle_run(text, cols), want)
        e = engine_with(cols)
        got = e.run_vdl(text)["results"]
        e.close()
        check_against_oracle("pool_programs_%s" % (mode or "default"), seed, text, cols, got, want)
