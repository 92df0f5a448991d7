"""Lookup images on the GPU (Engine.set_lookup_images): a dimension column looked up through a join index is read from its byte image
in every scan role -- aggregate scans in the eager, staged and queue forms, both sides of a fused front, dimension and semi-join
scans, sharded runs -- with the oracle's answers bit for bit on the same bytes, switch on and off, precompiled and specialised.
Plan.lookup_columns() must name the image wherever the switch is on and nothing (== {}) where it is off: a run that fell back to
the catalog column does not pass.  The directed programs and their catalogs are tests/test_lookup_images_cpu.py's."""
import os
import re

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import catalog, datagen, frontend, shard_rows
from conftest import ROOT, golden
from helpers import check_against_oracle, oracle_run, run_ranks
from test_lookup_images_cpu import MUST_LOOK_UP, PLANS, affine_cols, affine_program, chain_cols, chain_program
from test_scan_forms import SUFFIX

pytestmark = pytest.mark.gpu

META = os.path.join(ROOT, "tests", "golden", "tpch10noorder")
_want = {}


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one code-object cache for the module: a scan compiles once across the cases that share its source"""
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


def oracle_of(key, text, cols):
    """the expected result, computed once per (program, catalog) and non-empty"""
    if key not in _want:
        _want[key] = oracle_run(text, cols)
        assert any(len(list(v.values())[0]) for v in _want[key].values()), key
    return _want[key]


def encoded_engine(cols):
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
    return e


def run_mode(e, text, mode):
    """(results, note, lookup columns, image columns) of one run: "off" precompiled, "on" specialised, (u, late) a pinned form"""
    p = e.parse(text)
    if mode == "on":
        p.set_jit(True)
    elif mode != "off":
        p.set_jit(True, tune=True)
    got = p.run()["results"]
    out = got, p.jit_note(), p.lookup_columns(), p.image_columns()
    p.close()
    return out


# ---- 1. the Q14 shape ------------------------------------------------------------------------------------------------------------
Q14_ROWS = 30011
BAD = [-1, 1000, 2 ** 31 + 3, 2 ** 32 + 1]                      # join indices outside part's 1000 rows: those rows are EPS either way
Q14_MODES = {"precompiled": "off", "specialised": "on", "eager": (2, 0), "staged": (2, 1), "queue": (2, 3)}


def q14_cols(bad):
    cols = datagen.q14_tables(Q14_ROWS)
    assert len(cols["part.p_type"]) == 1000
    if bad:
        idx = cols["lineitem.lineitem_part"].copy()
        at = np.arange(0, len(idx), 997)
        idx[at] = np.array(BAD, np.int64)[np.arange(len(at)) % len(BAD)]
        cols["lineitem.lineitem_part"] = idx
    return cols


@pytest.mark.parametrize("bad", [False, True], ids=["in_range", "bad_indices"])
@pytest.mark.parametrize("mode", list(Q14_MODES))
def test_q14_reads_p_type_through_a_two_byte_narrowing(mode, bad, jit_cache, monkeypatch):
    """part.p_type is the source of the LIKE table -- a raw use -- and its image is a pure narrowing, which may stand in for it"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    form = Q14_MODES[mode]
    if isinstance(form, tuple):
        monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % form)
        monkeypatch.setenv("VDL_JIT_ASSUME_SELECTIVITY", "0.3")       # (every filter counts as selective: the staged and queue forms exist)
    text, cols = golden("q14.vdl"), q14_cols(bad)
    want = oracle_of(("q14", bad), text, cols)
    e = encoded_engine(cols)
    assert e.image_info("part.p_type") == (2, 0, 1)
    streamed = None
    for on in (True, False):
        e.set_lookup_images(on)
        got, note, lookups, images = run_mode(e, text, form)
        assert got == want, (mode, bad, on, note)
        assert lookups == ({"scan0": {"part.p_type": 2}} if on else {}), (on, lookups)
        assert "part.p_type" not in images.get("scan0", {}) and (streamed is None or images == streamed), images
        streamed = images
        if isinstance(form, tuple):
            chosen = re.findall(r"scan 0 tuned:[^;]*-> (k_mscan_specialised<\d+,(\d+),[^>]*>)", note)
            assert len(chosen) == 1 and int(chosen[0][1]) == form[0] and chosen[0][0].endswith(SUFFIX[form[1]] + ">"), (mode, note)
            assert (",limg" in chosen[0][0]) == on, (on, note)
        elif form == "on":
            assert "not specialised" not in note and (",limg" in note) == on, (on, note)
    e.close()


# ---- 2. an affine target under a filter and as a factor; 3. dimension sizes --------------------------------------------------------
@pytest.mark.parametrize("variant,emax", [("global", 200), ("global", 127), ("grouped", 200), ("keyed", 200)])
def test_affine_target_under_a_filter_and_as_a_wrapping_factor(variant, emax, jit_cache, monkeypatch):
    """u.x = 7 + 1000 e: the range filter's bounds are no multiples of 1000 and the upper one lies beyond the image's range, the
    SUM factor's multiplier is 2^61 + 5.  The ingest pass stores e as a SIGNED byte, so e in 0 .. 200 takes 2 bytes (scale 1000,
    base 7) and e in 0 .. 127 takes 1: both are run, each read at the width Engine.image_info reports.  "keyed": the looked-up value
    is also a component of the group key, so the affine image may not stand in for it and no lookup is listed.  (The other raw use of
    an aggregate scan, the column of a FIRST aggregate, cannot be a lookup: the planner takes only table columns there.)"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    text, cols = affine_program(variant), affine_cols(emax=emax)
    want = oracle_of(("affine", variant, emax), text, cols)
    e = encoded_engine(cols)
    width = 1 if emax <= 127 else 2
    assert e.image_info("u.x") == (width, 7, 1000)
    scans = 2 if variant == "global" else 1
    for on in (True, False):
        e.set_lookup_images(on)
        for mode in ("off", "on"):
            got, note, lookups, images = run_mode(e, text, mode)
            check_against_oracle("lookup_affine_%s_%d_%s_%s" % (variant, emax, on, mode), 0, text, cols, got, want)
            if on and variant != "keyed":
                assert lookups == {"scan%d" % s: {"u.x": width} for s in range(scans)}, lookups
            else:
                assert lookups == {}, lookups
            assert all("u.x" not in v for v in images.values()), images
            if mode == "on":
                assert "not specialised" not in note and (",limg" in note) == bool(lookups), note
    e.close()


@pytest.mark.parametrize("nu", [1, 63, 64, 65, 1000])
def test_dimension_sizes_around_the_image_padding(nu, jit_cache, monkeypatch):
    """the global form over dimensions of 1, 63, 64, 65 and 1000 rows; the join index reaches one row below and two beyond the table"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    text, cols = affine_program("global"), affine_cols(nu=nu)
    assert cols["t.t_u"].min() == -1 and cols["t.t_u"].max() == nu + 1
    want = oracle_of(("sizes", nu), text, cols)
    e = encoded_engine(cols)
    width = e.image_info("u.x")[0]
    assert width in (1, 2)
    for on in (True, False):
        e.set_lookup_images(on)
        for mode in ("off", "on"):
            got, note, lookups, _ = run_mode(e, text, mode)
            assert got == want, (nu, on, mode, note)
            assert lookups == ({"scan0": {"u.x": width}, "scan1": {"u.x": width}} if on else {}), lookups
    e.close()


# ---- 4. the Q3 front ---------------------------------------------------------------------------------------------------------------
Q3_ORDERS = 20011


@pytest.mark.parametrize("steps", [False, True], ids=["bytes", "steps"])
def test_q3_front_takes_the_orders_columns_through_their_images(steps):
    text = golden("q3.vdl")
    e = m.Engine(device=0)
    keep = datagen.register_q3_columns(e, Q3_ORDERS, steps=steps)
    cols = {k: e.download(k) for k in datagen.Q3_COLUMNS}
    want = oracle_of(("q3",), text, cols)
    for on in (True, False):
        e.set_lookup_images(on)
        for mode in ("off", "on"):
            got, note, lookups, images = run_mode(e, text, mode)
            assert got == want, (steps, on, mode, note)
            if on:
                take = lookups.get("front.take", {})
                assert take.get("orders.o_orderdate") == 2 and take.get("orders.o_shippriority") == 1, lookups
            else:
                assert lookups == {}, lookups
            assert all(not c.startswith("orders.") for c in images.get("front.take", {})), images
            if mode == "on":
                front = [x for x in note.split("; ") if x.startswith("front: ")]
                assert front and "not specialised" not in front[0] and (",limg" in front[0]) == on and (",stp" in front[0]) == steps, note
    e.close()
    del keep

    # the order date as an affine image of scale 1000: the take side decodes a key operand and an output exactly
    cols = dict(cols)
    cols["orders.o_orderdate"] = cols["orders.o_orderdate"].astype(np.int64) * 1000 + 7
    cols["orders.o_shippriority"] = cols["orders.o_shippriority"].astype(np.int64) * 1000 + 7
    scaled, n = re.subn(r"^15,RangeV,val,728732,", "15,RangeV,val,728732007,", text, flags=re.M)
    scaled, k = re.subn(r"^80,RangeV,val,727563,", "80,RangeV,val,727563007,", scaled, flags=re.M)
    assert n == 1 and k == 1
    want = oracle_of(("q3", "scaled"), scaled, cols)
    e = encoded_engine(cols)
    if steps:
        e.encode_steps("lineitem.lineitem_orders")
    w, base, scale = e.image_info("orders.o_orderdate")
    assert w == 2 and scale == 1000 and base == int(cols["orders.o_orderdate"].min()), (w, base, scale)
    for on in (True, False):
        e.set_lookup_images(on)
        for mode in ("off", "on"):
            got, note, lookups, _ = run_mode(e, scaled, mode)
            assert got == want, (steps, on, mode, note)
            assert (lookups.get("front.take", {}).get("orders.o_orderdate") == 2) == on and (on or lookups == {}), lookups
    e.close()


# ---- 5. lookup chains and every compiled plan ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PLANS)
def test_every_compiled_plan_under_lookup_images(n):
    cfg = frontend.load_metadata(META)
    text = frontend.compile_plan(open(os.path.join(META, "%02d.sql.mplan" % n)).read(), cfg)
    cols = catalog.synth_columns(META, cfg, text, scale=1e-3, seed=7)
    want = oracle_of(("plan", n), text, cols)
    e = encoded_engine(cols)
    for on in (True, False):
        e.set_lookup_images(on)
        for mode in ("off", "on"):
            got, note, lookups, _ = run_mode(e, text, mode)
            assert got == want, (n, on, mode, note, lookups)
            if not on:
                assert lookups == {}, lookups
            elif n in MUST_LOOK_UP:
                assert lookups, (n, mode, note)
            for col, w in lookup_targets_of(lookups).items():
                assert e.image_info(col)[0] == w, (col, w)
    e.close()


def lookup_targets_of(roles):
    got = {}
    for v in roles.values():
        got.update(v)
    return got


def test_lookup_chain_through_a_decoded_source():
    """t.t_u -> u.u_w (an image of base 40000, scale 1: the source of a further lookup, decoded after its own) -> w.z (scale 1000:
    encoded where the select side checks its range, decoded where the take side hands it over)"""
    text, cols = chain_program(), chain_cols()
    want = oracle_of(("chain",), text, cols)
    e = encoded_engine(cols)
    assert e.image_info("u.u_w") == (2, 40000, 1) and e.image_info("w.z") == (1, 7, 1000)
    for on in (True, False):
        e.set_lookup_images(on)
        for mode in ("off", "on"):
            got, note, lookups, _ = run_mode(e, text, mode)
            check_against_oracle("lookup_chain_%s_%s" % (on, mode), 0, text, cols, got, want)
            both = {"u.u_w": 2, "w.z": 1}
            assert lookups == ({"front.select": both, "front.take": both} if on else {}), lookups
            if mode == "on":
                assert "not specialised" not in note and (",limg" in note) == on, note
    e.close()


# ---- 6. sharded runs ---------------------------------------------------------------------------------------------------------------
def test_q3_as_three_co_partitioned_shards_looks_its_own_orders_slice_up():
    text = golden("q3.vdl")
    e = m.Engine(device=0)
    keep = datagen.register_q3_columns(e, Q3_ORDERS)
    want = oracle_of(("q3",), text, {k: e.download(k) for k in datagen.Q3_COLUMNS})
    e.close()
    del keep
    world, n_li = 3, 4 * Q3_ORDERS

    def work(rank, rv):
        lo, hi = shard_rows(n_li, rank, world)
        e = m.Engine(device=0)
        keep = datagen.register_q3_columns(e, Q3_ORDERS, (lo, hi), copartition=True)
        e.set_lookup_images(True)
        e.comm_init_host(rank, world, *rv.transport(rank))
        p = e.parse(text)
        p.set_sharded_table("lineitem")
        p.set_row_offset(lo)
        res = p.run_sharded()["results"]
        lookups, base = p.lookup_columns(), e.image_info("orders.o_orderdate")
        p.close()
        e.close()
        del keep
        return res, lookups, base

    parts = run_ranks(world, work, timeout=600)
    got = {k: {name: sum((part[0][k][name] for part in parts), []) for name in v} for k, v in want.items()}
    assert got == want
    for res, lookups, image in parts:
        take = lookups.get("front.take", {})
        assert take.get("orders.o_orderdate") == 2 and take.get("orders.o_shippriority") == 1, lookups
        assert image[0] == 2 and image[1] != 0                   # (every slice's image has its own base)


def test_q14_as_two_row_range_shards_through_the_fold_route():
    text, cols = golden("q14.vdl"), q14_cols(False)
    want = oracle_of(("q14", False), text, cols)
    world = 2
    li = [k for k in cols if k.startswith("lineitem.")]

    def work(rank, rv):
        lo, hi = shard_rows(Q14_ROWS, rank, world)
        e = encoded_engine({k: (v[lo:hi] if k in li else v) for k, v in cols.items()})
        e.set_lookup_images(True)
        e.comm_init_host(rank, world, *rv.transport(rank))
        p = e.parse(text)
        p.set_sharded_table("lineitem")
        p.set_row_offset(lo)
        route = p.sharded_route()
        res = p.run_sharded()["results"]
        lookups = p.lookup_columns()
        p.close()
        e.close()
        return route, res, lookups

    for route, res, lookups in run_ranks(world, work, timeout=600):
        assert route == ("fold", True)
        assert res == want
        assert lookups == {"scan0": {"part.p_type": 2}}, lookups


# ---- 7. the switch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["off", "on"])
def test_one_plan_follows_the_switch_and_column_images_win(mode, jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    monkeypatch.delenv("VDL_LOOKUP_IMAGES", raising=False)
    text, cols = affine_program("global"), affine_cols()
    want = oracle_of(("affine", "global", 200), text, cols)
    e = encoded_engine(cols)
    p = e.parse(text)
    if mode == "on":
        p.set_jit(True)
    both = {"scan0": {"u.x": 2}, "scan1": {"u.x": 2}}
    assert p.run()["results"] == want and p.lookup_columns() == {}           # off by default
    for on in (True, False, True):
        e.set_lookup_images(on)
        assert p.run()["results"] == want, on
        assert p.lookup_columns() == (both if on else {}), (on, p.lookup_columns())
        if mode == "on":
            assert (",limg" in p.jit_note()) == on, p.jit_note()
    e.set_column_images(False)                                               # ... under which the switch is ignored
    assert p.run()["results"] == want
    assert p.lookup_columns() == {} and p.image_columns() == {}
    e.set_column_images(True)
    assert p.run()["results"] == want and p.lookup_columns() == both
    p.close()
    e.close()
