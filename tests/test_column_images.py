"""Frame-of-reference column images on the GPU (csrc/vdl_column_image.h, vdl_image.hip, bind_scan): aggregate scans that read
the narrow images instead of the catalog columns give the oracle's answers bit for bit -- Q6, Q1, every compiled TPC-H plan and
random fused programs, with images on and off, precompiled and specialised, one GPU and sharded -- and the census of a staged
scan over images counts the lines of the image widths."""
import os

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import catalog, datagen, frontend
from conftest import ROOT
from helpers import check_against_oracle, oracle_run, run_ranks

pytestmark = pytest.mark.gpu

META = os.path.join(ROOT, "tests", "golden", "tpch10noorder")
PLANS = [1, 3, 4, 5, 6, 9, 10, 11, 12, 14, 15, 16, 18, 19, 20]


def golden(name):
    return open(os.path.join(ROOT, "tests", "golden", name)).read()


def encoded_engine(cols):
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
    return e


def runs_three_ways(e, text, jit_modes=("off", "on")):
    """results with images on under each jit mode, then with images off"""
    out = []
    for images in (True, False):
        e.set_column_images(images)
        for mode in jit_modes:
            p = e.parse(text)
            if mode != "off":
                p.set_jit(True, tune=mode == "tune")
            out.append((images, mode, p.run()["results"], p.jit_note()))
            p.close()
    e.set_column_images(True)
    return out


@pytest.mark.parametrize("query", ["q6", "q1"])
def test_generated_columns_carry_images_and_queries_match_the_oracle(query):
    n = 300007
    names = datagen.Q6_COLUMNS if query == "q6" else datagen.Q1_COLUMNS
    text = golden(query + ".vdl")
    e = m.Engine(device=0)
    for name in names:
        e.generate(datagen.LINEITEM[name], 0, n)
    assert e.image_info("lineitem.l_shipdate") == (2, 727564, 1)
    assert e.image_info("lineitem.l_discount") == (1, 0, 1)
    assert e.image_info("lineitem.l_quantity") == (1, 100, 100)
    assert e.image_info("lineitem.l_extendedprice") == (4, 0, 1)
    cols = {k: e.download(k) for k in names}                   # the catalog columns stay as generated
    for k, v in cols.items():
        assert v.dtype == datagen.LINEITEM[k].dtype and np.array_equal(v, datagen.generate(datagen.LINEITEM[k], 0, n))
    want = oracle_run(text, cols)
    for images, mode, got, note in runs_three_ways(e, text, ("off", "on", "tune")):
        assert got == want, (images, mode, note)
        if mode != "off" and "k_mscan_specialised" in note:
            assert (",img" in note) == images, note
    e.close()


@pytest.mark.parametrize("n", PLANS)
def test_every_compiled_plan_over_images_matches_the_oracle(n):
    cfg = frontend.load_metadata(META)
    text = frontend.compile_plan(open(os.path.join(META, "%02d.sql.mplan" % n)).read(), cfg)
    cols = catalog.synth_columns(META, cfg, text, scale=1e-3, seed=7)
    want = oracle_run(text, cols)
    e = encoded_engine(cols)
    for images, mode, got, note in runs_three_ways(e, text):
        assert got == want, (n, images, mode, note)
    e.close()


def test_random_fused_programs_over_images_match_the_oracle():
    from test_random_fused import Gen
    for seed in range(120):
        text, cols = Gen(seed).build()
        want = oracle_run(text, cols)
        e = encoded_engine(cols)
        for images, mode, got, note in runs_three_ways(e, text):
            check_against_oracle("random_fused_images_%s_%s" % (images, mode), seed, text, cols, got, want)
        e.close()


@pytest.mark.parametrize("case", ["shaped", "wide"])
def test_columns_of_every_shape_round_trip_through_their_images(case):
    """the random fused programs over columns of other shapes: negative values under a power-of-ten scale (an affine image, its
    filters rewritten with negative offsets), a single value, a scale only some rows share, values that do not narrow"""
    from test_random_fused import Gen
    widths = []
    for seed in range(40):
        text, cols = Gen(seed).build()
        n = len(cols["t.a"])
        rng = np.random.default_rng(seed)
        cols["t.a"] = (rng.integers(-60, 60, n) * 10 ** 6 - 5).astype(np.int64)
        cols["t.b"] = np.full(n, 17, dtype=np.int32)
        cols["t.c"] = (rng.integers(0, 40, n) * 100 + (np.arange(n) % 97 == 0) * 3).astype(np.int64) if case == "shaped" else \
            rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
        want = oracle_run(text, cols)
        e = encoded_engine(cols)
        widths.append(tuple(e.image_info("t." + c) for c in "abc"))
        for k, v in cols.items():
            assert np.array_equal(e.download(k), v)
        for images, mode, got, note in runs_three_ways(e, text):
            check_against_oracle("image_shapes_%s_%s_%s" % (case, images, mode), seed, text, cols, got, want)
        e.close()
    for (a, b, c) in widths:
        assert a[0] == 1 and a[2] == 10 ** 6                     # affine: (v - min) / 10^6
        assert b == (1, 0, 1)
        if case == "shaped":
            assert c[0] == 2 and c[2] == 1                       # (the 3s break the scale of 100: a pure narrowing)
        else:
            assert c[0] == 0


@pytest.mark.parametrize("late", [1, 4])
def test_scan_traffic_over_images_counts_the_image_lines(late, monkeypatch):
    """the census of a staged scan over images: the eager images in full plus 128 B per line of a late image in which a row was
    still in -- a numpy count over the image widths (128 rows of a 1-byte image per line, 32 of the 4-byte one)"""
    monkeypatch.setenv("VDL_JIT_U", "2")
    monkeypatch.setenv("VDL_JIT_LATE", str(late))
    text = golden("q6.vdl")
    n = 1024 * 301
    e = m.Engine(device=0)
    for name in datagen.Q6_COLUMNS:
        e.generate(datagen.LINEITEM[name], 0, n)
    cols = {k: e.download(k) for k in datagen.Q6_COLUMNS}
    p = e.parse(text)
    p.set_jit(True)
    assert p.run()["results"] == oracle_run(text, cols)
    moved, detail = p.scan_traffic()
    e.close()
    d, disc, q, x = (cols["lineitem." + c] for c in ("l_shipdate", "l_discount", "l_quantity", "l_extendedprice"))
    lines = lambda alive, per: int(alive.reshape(-1, per).any(axis=1).sum())
    a0 = (d >= 728294) & (d <= 728658)
    a1 = a0 & (disc >= 5) & (disc <= 7)
    a2 = a1 & (q < 2400)
    if late == 4:                                                # every filter image with the tile (2 + 1 + 1 B), the price late
        want = 4 * n + 128 * lines(a2, 32)
    else:                                                        # the date with the tile, discount, quantity, price late in that order
        want = 2 * n + 128 * (lines(a0, 128) + lines(a1, 128) + lines(a2, 32))
    assert moved == want, (moved, want, detail)


def test_eight_generated_shards_fold_over_their_own_images():
    """the sharded fold route: every rank generates its rows (and their image) and the merged answer is the whole table's"""
    text = golden("q6.vdl")
    world, n = 8, 400009
    whole = {k: datagen.generate(datagen.LINEITEM[k], 0, n) for k in datagen.Q6_COLUMNS}
    want = oracle_run(text, whole)

    def work(rank, rv):
        r0, r1 = m.shard_rows(n, rank, world)
        e = m.Engine(device=0)
        for k in datagen.Q6_COLUMNS:
            e.generate(datagen.LINEITEM[k], r0, r1 - r0)
        assert e.image_info("lineitem.l_quantity")[0] == 1
        e.comm_init_host(rank, world, *rv.transport(rank))
        p = e.parse(text)
        p.set_row_offset(r0)
        p.set_jit(True)
        res = [p.run_sharded()["results"]]
        e.set_column_images(False)
        res.append(p.run_sharded()["results"])
        e.close()
        return res

    for got in run_ranks(world, work, timeout=600):
        assert got == [want, want]
