"""Column images read by the scans with derived columns (csrc/vdl_bind.cpp, project_front_body, project_select_body): fused fronts,
dimension scans and semi-join scans over encoded columns give the oracle's answers bit for bit -- Q3 over the columns the benchmark
registers, every compiled TPC-H plan, random front / join / semi-join programs over columns shaped to break a wrong decode, sharded
runs, the pipe end (`vdlrun --encode`) -- with images on and off, precompiled and specialised, and Plan.image_columns() names what
each scan role read from an image."""
import json
import os
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import catalog, datagen, frontend, resolve, shard_rows
from mplan2vdl_amd._lib import parse_image_columns
from conftest import ROOT, golden
from helpers import check_against_oracle, oracle_run, run_ranks

pytestmark = pytest.mark.gpu

META = os.path.join(ROOT, "tests", "golden", "tpch10noorder")
PLANS = [1, 3, 4, 5, 6, 9, 10, 11, 12, 14, 15, 16, 18, 19, 20]
VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
SIDE_ROLES = ("front.", "dim", "semi")


def compiled(n):
    cfg = frontend.load_metadata(META)
    return cfg, frontend.compile_plan(open(os.path.join(META, "%02d.sql.mplan" % n)).read(), cfg)


def encoded_engine(cols):
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
    return e


def runs_both_ways(e, text, jit_modes=("off", "on")):
    """[(images, jit mode, results, jit note, image columns)] with images on, then off"""
    out = []
    for images in (True, False):
        e.set_column_images(images)
        for mode in jit_modes:
            p = e.parse(text)
            if mode == "on":
                p.set_jit(True)
            out.append((images, mode, p.run()["results"], p.jit_note(), p.image_columns()))
            p.close()
    e.set_column_images(True)
    return out


def side_columns(roles):
    """{column: width} over the front / dimension / semi-join roles"""
    got = {}
    for role, cols in roles.items():
        if role.startswith(SIDE_ROLES):
            got.update(cols)
    return got


def test_image_column_lists_parse():
    assert parse_image_columns("") == {}
    assert parse_image_columns("dim2: orders.o_orderdate:2; front.select: lineitem.l_shipdate:2 lineitem.lineitem_orders:4") == {
        "dim2": {"orders.o_orderdate": 2}, "front.select": {"lineitem.l_shipdate": 2, "lineitem.lineitem_orders": 4}}


def test_q3_front_reads_the_registered_columns_through_their_images():
    n_orders = 20011
    text = golden("q3.vdl")
    e = m.Engine(device=0)
    keep = datagen.register_q3_columns(e, n_orders)
    cols = {k: e.download(k) for k in datagen.Q3_COLUMNS}
    want = oracle_run(text, cols)
    assert any(len(list(v.values())[0]) for v in want.values())
    names = ("lineitem.l_shipdate", "lineitem.lineitem_orders", "lineitem.l_discount", "lineitem.l_extendedprice")
    for name in names:
        assert e.image_info(name)[0] in (1, 2, 4), name
    for images, mode, got, note, roles in runs_both_ways(e, text):
        assert got == want, (images, mode, note, roles)
        if not images:
            assert roles == {}, roles
        else:
            front = {}
            for role in ("front.select", "front.take"):
                front.update(roles.get(role, {}))
            for name in names:
                assert front.get(name) == e.image_info(name)[0], (name, roles)
            assert roles["front.select"].get("lineitem.lineitem_orders") == e.image_info("lineitem.lineitem_orders")[0], roles
            assert any(r.startswith("dim") and any(c.startswith("orders.") for c in v) for r, v in roles.items()), roles
        if mode == "on":
            line = [x for x in note.split("; ") if x.startswith("front: ")]
            assert line and "not specialised" not in line[0], note
            assert (",img>" in line[0]) == images, note
    e.close()
    del keep


def test_q3_over_an_offset_join_index_and_scaled_prices():
    """a lineitem slice whose join index starts far from 0 (an affine image: base != 0, 2 bytes) with a few indices past the
    orders table (those rows are EPS), prices with a decimal scale (an affine image of scale 1000 or more: the take side decodes the revenue
    term's operands), and a shipdate filter whose bounds lie outside the image's range on one side"""
    n_orders = 70001
    tabs = datagen.q3_tables(n_orders)
    r0, r1 = 4 * 40000, 4 * 52000
    cols = {k: (v[r0:r1].copy() if k.startswith("lineitem.") else v) for k, v in tabs.items() if k in datagen.Q3_COLUMNS}
    idx = cols["lineitem.lineitem_orders"]
    idx[::997] = n_orders + 5
    cols["lineitem.l_extendedprice"] = cols["lineitem.l_extendedprice"].astype(np.int64) * 1000
    cols["lineitem.l_shipdate"] = cols["lineitem.l_shipdate"] + 40 * (np.arange(len(idx)) % 2)
    text = golden("q3.vdl")
    want = oracle_run(text, cols)
    e = encoded_engine(cols)
    w, base, scale = e.image_info("lineitem.lineitem_orders")
    assert w == 2 and base == 40000 and scale == 1, (w, base, scale)
    w, base, scale = e.image_info("lineitem.l_extendedprice")
    assert w == 4 and scale >= 1000 and base != 0, (w, base, scale)
    for images, mode, got, note, roles in runs_both_ways(e, text):
        assert got == want, (images, mode, note, roles)
        if images:
            assert "lineitem.lineitem_orders" in roles.get("front.select", {}), roles
            assert "lineitem.l_extendedprice" in roles.get("front.take", {}), roles
    e.close()


@pytest.mark.parametrize("n", PLANS)
def test_every_compiled_plan_over_encoded_columns(n):
    cfg, text = compiled(n)
    cols = catalog.synth_columns(META, cfg, text, scale=1e-3, seed=7)
    want = oracle_run(text, cols)
    e = encoded_engine(cols)
    p = e.parse(text)
    d = p.describe()
    p.close()
    for images, mode, got, note, roles in runs_both_ways(e, text):
        assert got == want, (n, images, mode, note, roles)
        if not images:
            assert roles == {}, roles
        elif "\nfused front:" in d:
            assert side_columns(roles), (n, d, roles)
    e.close()


def shaped(cols, seed):
    """the generators' integer columns moved to where a wrong decode shows: the first column scaled by 10^6 and shifted negative (an
    affine image of 1 byte), the second negative (a 1- or 2-byte pure narrowing of negative values), and one column whose range
    is too wide to narrow next to them (no image)"""
    rng = np.random.default_rng(seed)
    out = dict(cols)
    names = [k for k in sorted(cols) if not k.endswith("pkey") and cols[k].dtype.kind == "i" and len(cols[k])]
    tables = {}
    for k in names:
        tables.setdefault(k.split(".")[0], []).append(k)
    for t, ks in tables.items():
        plain = [k for k in ks if cols[k].min() >= -200 and cols[k].max() <= 200]
        if plain:
            k = plain[0]
            out[k] = (cols[k].astype(np.int64) * 10 ** 6 - 5)
        if len(plain) > 1:
            k = plain[1]
            out[k] = cols[k].astype(np.int64) - 300
        if len(plain) > 2:
            k = plain[2]
            v = cols[k].astype(np.int64).copy()
            v[rng.integers(0, len(v), 2)] = [-(1 << 40), 1 << 40]
            out[k] = v
    return out


def random_generators():
    from test_random_conditions import FrontGen
    from test_random_joins import Gen as JoinGen
    from test_random_semijoins import Gen as SemiGen
    return [("front", FrontGen), ("join", JoinGen), ("semi", SemiGen), ("semi_front", lambda s: SemiGen(s, sparse_domain=True))]


@pytest.mark.parametrize("kind", ["front", "join", "semi", "semi_front"])
@pytest.mark.parametrize("shape", ["as_generated", "shaped"])
def test_random_programs_over_encoded_columns(kind, shape):
    gen = dict(random_generators())[kind]
    read = 0
    for seed in range(36):
        text, cols = gen(seed).build()
        if shape == "shaped":
            cols = shaped(cols, seed)
        want = oracle_run(text, cols)
        e = encoded_engine(cols)
        for images, mode, got, note, roles in runs_both_ways(e, text, ("off", "on") if seed % 6 == 0 else ("off",)):
            check_against_oracle("front_images_%s_%s_%s_%s" % (kind, shape, images, mode), seed, text, cols, got, want)
            if images:
                read += bool(side_columns(roles))
            else:
                assert roles == {}, roles
        e.close()
    assert read > 0


def test_q3_as_co_partitioned_shards_each_with_its_own_images():
    text = golden("q3.vdl")
    n_orders = 30011
    n_li = 4 * n_orders
    e = m.Engine(device=0)
    keep = datagen.register_q3_columns(e, n_orders)
    want = e.run_vdl(text)["results"]
    cols = {k: e.download(k) for k in datagen.Q3_COLUMNS}
    assert want == oracle_run(text, cols)
    e.close()
    del keep

    for world, copart in ((4, True), (8, False)):
        def work(rank, rv):
            lo, hi = shard_rows(n_li, rank, world)
            e = m.Engine(device=0)
            keep = datagen.register_q3_columns(e, n_orders, (lo, hi), copartition=copart)
            e.comm_init_host(rank, world, *rv.transport(rank))
            p = e.parse(text)
            p.set_sharded_table("lineitem")
            p.set_row_offset(lo)
            res = [p.run_sharded()["results"]]
            roles = p.image_columns()
            e.set_column_images(False)
            res.append(p.run_sharded()["results"])
            off = p.image_columns()
            p.close()
            e.close()
            del keep
            return res, roles, off

        parts = run_ranks(world, work, timeout=600)
        for j in range(2):
            got = {k: {name: sum((part[0][j][k][name] for part in parts), []) for name in v} for k, v in want.items()}
            assert got == want, (world, copart, j)
        for res, roles, off in parts:
            assert side_columns(roles), roles
            assert off == {}, off


@pytest.mark.parametrize("plan_no", [15, 16])
def test_front_route_plans_over_encoded_shards(plan_no):
    """Q15 / Q16 sharded by lineitem rows, every rank's columns encoded: the ranks' answers are the whole table's"""
    cfg, text = compiled(plan_no)
    cols = catalog.synth_columns(META, cfg, text, scale=1e-3, seed=7)
    want = oracle_run(text, cols)
    world = 2
    li = [k for k in cols if k.startswith("lineitem.") and not k.endswith(".heap")]
    n = len(cols[li[0]]) if li else 0

    def work(rank, rv):
        lo, hi = shard_rows(n, rank, world)
        e = encoded_engine({k: (v[lo:hi] if k in li else v) for k, v in cols.items()})
        e.comm_init_host(rank, world, *rv.transport(rank))
        p = e.parse(text)
        p.set_sharded_table("lineitem")
        p.set_row_offset(lo)
        whole = p.sharded_route()[1]
        res = p.run_sharded()["results"]
        e.close()
        return whole, res

    parts = run_ranks(world, work, timeout=600)
    if parts[0][0]:
        for whole, res in parts:
            assert res == want
    else:
        got = {k: {name: sum((part[1][k][name] for part in parts), []) for name in v} for k, v in want.items()}
        assert got == want


def pipe(text, args):
    r = subprocess.run([VDLRUN] + args, input=text.encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads(r.stdout.decode()), r.stderr.decode()


@pytest.mark.parametrize("plan", [3, 4, 10])
def test_vdlrun_encode_reads_images_and_answers_the_same(tmp_path, plan):
    cfg, text = compiled(plan)
    text = "\n".join(ln.split(";;")[0].rstrip() for ln in text.splitlines()) + "\n"
    cols = catalog.synth_columns(META, cfg, text, scale=1e-3, seed=5)
    coldir = str(tmp_path / "cols")
    catalog.export_columns(cols, coldir)
    want = oracle_run(text, cols)
    dictionary = resolve.load_dictionary(os.path.join(META, "dictionary.csv"))
    replies = {}
    for flags in ([], ["--encode"], ["--jit"], ["--jit", "--encode"]):
        reply, err = pipe(text, ["--data", coldir] + flags)
        assert reply["results"] == want, flags
        assert set(reply) == {"results", "timings"}
        resolve.decode(reply, dictionary)
        lines = [ln for ln in err.splitlines() if ln.startswith("vdlrun: images: ")]
        if "--encode" in flags:
            assert len(lines) == 1, err
            roles = parse_image_columns(lines[0][len("vdlrun: images: "):])
            assert side_columns(roles), (plan, roles)
        else:
            assert not lines, err
        replies[tuple(flags)] = reply["results"]
    assert len({json.dumps(v, sort_keys=True) for v in replies.values()}) == 1


def test_vdlrun_rows_encode_keeps_its_reply():
    """--rows: the generated lineitem, encoded again; Q1's grouped scan reads the images either way, the line names them"""
    text = golden("q1.vdl")
    plain, err0 = pipe(text, ["--rows", "50000"])
    enc, err1 = pipe(text, ["--rows", "50000", "--encode"])
    assert plain["results"] == enc["results"]
    assert "vdlrun: images: " not in err0
    line = [ln for ln in err1.splitlines() if ln.startswith("vdlrun: images: ")]
    assert len(line) == 1 and "lineitem.l_shipdate:2" in line[0], err1


def test_front_rebinds_when_images_or_columns_change():
    n_orders = 9001
    text = golden("q3.vdl")
    e = m.Engine(device=0)
    keep = datagen.register_q3_columns(e, n_orders)
    cols = {k: e.download(k) for k in datagen.Q3_COLUMNS}
    want = oracle_run(text, cols)
    for mode in ("off", "on"):
        p = e.parse(text)
        if mode == "on":
            p.set_jit(True)
        e.set_column_images(True)
        assert p.run()["results"] == want
        assert "lineitem.l_discount" in p.image_columns().get("front.take", {})
        e.set_column_images(False)
        assert p.run()["results"] == want
        assert p.image_columns() == {}
        if mode == "on":
            assert ",img>" not in p.jit_note(), p.jit_note()
        e.set_column_images(True)
        e.drop("lineitem.l_discount")
        e.upload("lineitem.l_discount", cols["lineitem.l_discount"])
        assert p.run()["results"] == want
        roles = p.image_columns()
        assert "lineitem.l_discount" not in roles.get("front.take", {}) and "lineitem.lineitem_orders" in roles.get("front.select", {}), roles
        e.encode("lineitem.l_discount")
        assert p.run()["results"] == want
        assert "lineitem.l_discount" in p.image_columns().get("front.take", {})
        if mode == "on":
            assert ",img>" in p.jit_note(), p.jit_note()
        p.close()
    e.close()
    del keep
