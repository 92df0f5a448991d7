"""Step images (vdl_column_image.h Steps; vdl.h "step images"): a join index that never decreases and steps by at most 1 kept as a
base, one bit per row and one anchor per 64 rows, built by k_image_steps and decoded with the tile by the fused front, dimension
scans and semi-join scans.  The image against numpy at the group and tile edges, columns that do not qualify, Q3 through it with
every switch both ways, the decode's edges (partial tile, carried and fetched survivors), every compiled plan, two ranks, the
pipe end."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import catalog, datagen, frontend, shard_rows
from mplan2vdl_amd._lib import parse_step_columns
from conftest import ROOT, golden
from helpers import oracle_run, run_ranks

pytestmark = pytest.mark.gpu

META = os.path.join(ROOT, "tests", "golden", "tpch10noorder")
PLANS = [1, 3, 4, 5, 6, 9, 10, 11, 12, 14, 15, 16, 18, 19, 20]          # tests/test_front_images.py::PLANS
VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
JOIN_INDEX = "lineitem.lineitem_orders"


def body_constant(pattern):
    text = open(os.path.join(ROOT, "mplan2vdl_amd", "csrc", "vdl_mscan_body.h")).read()
    return int(re.search(pattern, text).group(1))


# the tile of the projection scans and the front's carry area, from the kernels' own header
T = body_constant(r"constexpr int kMsBlock = (\d+);") * 2 * body_constant(r"#define VDL_PROJ_U (\d+)")
FRONT_CARRY = body_constant(r"constexpr int kFrontCarry = (\d+);")
FRONT_BATCH = body_constant(r"#define VDL_FRONT_BATCH (\d+)")
assert T % 64 == 0 and T >= 128


def popcount64(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype="<u8").view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64)


def decode(base, heads, anchors, n):
    """v[r] = base + anchor[r >> 6] + popcount(heads[r >> 6] & (~0 >> (63 - (r & 63)))), as include/vdl.h states it"""
    r = np.arange(n, dtype=np.int64)
    mask = np.uint64(0xFFFFFFFFFFFFFFFF) >> (np.uint64(63) - (r & 63).astype(np.uint64))
    return base + anchors[r >> 6].astype(np.int64) + popcount64(heads[r >> 6] & mask)


def step_rows(n, steps_at):
    return sorted({r for r in steps_at if 1 <= r < n})


def step_column(n, base, steps_at, dtype):
    """starts at `base`, goes up by 1 at every row of `steps_at` (rows 1 .. n - 1)"""
    up = np.zeros(n, dtype=np.int64)
    up[step_rows(n, steps_at)] = 1
    return (base + np.cumsum(up)).astype(dtype)


# ---- 1. the image against numpy ------------------------------------------------------------------------------------------
BASES = {2: -3000, 4: 70000, 8: (1 << 40) + 5}


@pytest.mark.parametrize("width", [2, 4, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 4 * T + 65])
def test_image_against_numpy(n, width):
    dtype, base = {2: np.int16, 4: np.int32, 8: np.int64}[width], BASES[width]
    shapes = {"t.equal": [], "t.every": range(1, n), "t.edges": [64, T, n - 1], "t.mixed": [r for r in range(1, n) if r % 4 == 0 or r % 67 == 66]}
    e = m.Engine(device=0)
    for name, at in shapes.items():
        col = step_column(n, base, at, dtype)
        assert col[0] == base and int(col[-1]) == base + len(step_rows(n, at))
        e.upload(name, col)
        e.encode_steps(name)
        assert e.steps_info(name) == (True, base, (n + 63) // 64), (name, e.steps_info(name))
        heads, anchors = e.download_steps(name)
        assert len(heads) == len(anchors) == (n + 63) // 64
        assert np.array_equal(decode(base, heads, anchors, n), col.astype(np.int64)), name
        # ... and the layout itself: bit i of word g <=> row 64 g + i differs from the row before; the anchor is the row before the group
        want_bits = np.zeros(len(heads) * 64, dtype=np.uint8)
        want_bits[1:n] = col[1:] != col[:-1]
        assert np.array_equal(np.unpackbits(heads.view(np.uint8), bitorder="little"), want_bits), name
        g = np.arange(1, len(heads))
        assert anchors[0] == 0 and np.array_equal(anchors[1:].astype(np.int64), col.astype(np.int64)[64 * g - 1] - base), name
        assert np.array_equal(e.download(name), col)                       # the column itself is untouched
    if n > 1:
        assert popcount64(e.download_steps("t.equal")[0]).sum() == 0
        assert popcount64(e.download_steps("t.every")[0]).sum() == n - 1
    # re-registration and drop take the image along; an encode of the byte image leaves it alone
    e.encode("t.every")
    assert e.steps_info("t.every")[0]
    e.upload("t.every", step_column(n, base, [], dtype))
    assert e.steps_info("t.every") == (False, 0, 0)
    e.drop("t.equal")
    with pytest.raises(m.VdlError):
        e.steps_info("t.equal")
    e.close()


# ---- 2. columns that do not qualify --------------------------------------------------------------------------------------
def q3_host_catalog(n_orders):
    return {k: v for k, v in datagen.q3_tables(n_orders).items() if k in datagen.Q3_COLUMNS}


def spoiled(kind, idx, idx_max):
    idx = idx.copy()
    if kind == "one_decrease":
        idx[101] = idx[100] - 1                            # (rows 100 .. 103 are one order: 101 falls back to the order before)
    elif kind == "one_step_of_2":
        idx[200:] += 1                                     # rows 199 -> 200 start a new order anyway: now two further
    else:                                                  # a step of 2 exactly across a group boundary
        assert kind == "step_of_2_across_groups"
        idx[64:] += 1
        assert idx[64] - idx[63] == 2
    return np.minimum(idx, idx_max)                        # (the shifted tail stays inside the orders table, and non-decreasing)


@pytest.mark.parametrize("kind", ["one_decrease", "one_step_of_2", "step_of_2_across_groups"])
def test_columns_that_do_not_qualify_get_no_image(kind):
    n_orders = 701
    cols = q3_host_catalog(n_orders)
    cols[JOIN_INDEX] = spoiled(kind, cols[JOIN_INDEX], n_orders - 1)
    d = np.diff(cols[JOIN_INDEX])
    assert ((d < 0) | (d > 1)).sum() == 1 and 0 <= cols[JOIN_INDEX].min() and cols[JOIN_INDEX].max() == n_orders - 1 and len(d) + 1 > T
    text = golden("q3.vdl")
    want = oracle_run(text, cols)
    assert any(len(list(v.values())[0]) for v in want.values())
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
    e.encode_steps(JOIN_INDEX)                             # VDL_OK whether or not the column qualifies (an error would raise)
    assert e.steps_info(JOIN_INDEX) == (False, 0, 0)
    for jit in (False, True):
        p = e.parse(text)
        p.set_jit(jit)
        assert p.run()["results"] == want, (kind, jit)
        assert p.step_columns() == {}, p.step_columns()
        assert ",stp" not in p.jit_note()
        p.close()
    e.close()


# ---- 3. Q3 through the step image ----------------------------------------------------------------------------------------
def test_q3_through_the_step_image():
    text = golden("q3.vdl")
    e = m.Engine(device=0)
    keep = datagen.register_q3_columns(e, 20011, steps=True)
    cols = {k: e.download(k) for k in datagen.Q3_COLUMNS}
    want = oracle_run(text, cols)
    assert any(len(list(v.values())[0]) for v in want.values())
    assert e.steps_info(JOIN_INDEX) == (True, 0, (4 * 20011 + 63) // 64)
    today = {}                                             # image_columns() without step images, by (images, jit)
    for steps in (False, True):
        e.set_step_images(steps)
        for images in (True, False):
            e.set_column_images(images)
            for jit in (False, True):
                p = e.parse(text)
                p.set_jit(jit)
                got = p.run()["results"]
                note, roles, stepped = p.jit_note(), p.image_columns(), p.step_columns()
                p.close()
                assert got == want, (steps, images, jit, note)
                if not steps:
                    today[(images, jit)] = roles
                    assert stepped == {} and ",stp" not in note, (stepped, note)
                elif images:
                    assert JOIN_INDEX in stepped["front.select"] and JOIN_INDEX in stepped.get("front.take", []), stepped
                    assert JOIN_INDEX not in roles.get("front.select", {}) and JOIN_INDEX not in roles.get("front.take", {}), roles
                    # every other column is read as it is today
                    assert {r: {k: w for k, w in c.items() if k != JOIN_INDEX} for r, c in today[(images, jit)].items()} == roles, (roles, today)
                    if jit:
                        line = [x for x in note.split("; ") if x.startswith("front: ")]
                        assert line and "not specialised" not in line[0] and ",img,stp>" in line[0], note
                else:
                    assert stepped == {} and roles == today[(images, jit)] == {}, (stepped, roles)
                    assert ",stp" not in note, note
    e.set_column_images(True)
    e.close()
    del keep


# ---- 4. edges of the decode ----------------------------------------------------------------------------------------------
EDGE_N = 4 * T + 65


@pytest.fixture(scope="module")
def edge_catalog():
    """n = 4 T + 65 lineitems (a partial last tile; not a multiple of 64) cut out of the Q3 catalog from a row in the middle of an
    order, the orders table whole: the join index starts at 700.  Every order and customer passes, so the ship date alone decides."""
    r0, n_orders = 4 * 700 + 2, 4000
    tabs = datagen.q3_tables(n_orders)
    cols = {k: (v[r0:r0 + EDGE_N].copy() if k.startswith("lineitem.") else v.copy()) for k, v in tabs.items() if k in datagen.Q3_COLUMNS}
    assert len(cols[JOIN_INDEX]) == EDGE_N and cols[JOIN_INDEX][0] == 700 and EDGE_N % 64 != 0
    cols["orders.o_orderdate"][:] = 728000                 # < date '1995-03-15' (728732)
    cols["customer.c_mktsegment"][:] = 16                  # 'BUILDING'
    return cols


def edge_case(cols, surviving_rows):
    out = dict(cols)
    ship = np.full(EDGE_N, 728000, dtype=cols["lineitem.l_shipdate"].dtype)
    ship[surviving_rows] = 729000                          # > 728732
    out["lineitem.l_shipdate"] = ship
    return out


@pytest.mark.parametrize("case", ["six_rows", "every_row"])
def test_edges_of_the_decode(edge_catalog, case):
    rows = [0, 63, 64, T - 1, T, EDGE_N - 1] if case == "six_rows" else np.arange(EDGE_N)
    cols = edge_case(edge_catalog, rows)
    text = golden("q3.vdl")
    want = oracle_run(text, cols)
    orders = np.unique(cols[JOIN_INDEX][rows])
    assert len(orders) and all(len(list(v.values())[0]) == len(orders) for v in want.values())      # one group per surviving order
    if case == "every_row":
        assert FRONT_BATCH * T > FRONT_CARRY               # a batch's survivors overflow the carry area: the rest is fetched per survivor
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
    e.encode_steps(JOIN_INDEX)
    assert e.steps_info(JOIN_INDEX) == (True, 700, (EDGE_N + 63) // 64)
    for jit in (False, True):
        p = e.parse(text)
        p.set_jit(jit)
        assert p.run()["results"] == want, (case, jit, p.jit_note())
        stepped = p.step_columns()
        assert JOIN_INDEX in stepped.get("front.select", []) and JOIN_INDEX in stepped.get("front.take", []), stepped
        if jit:
            assert ",stp" in p.jit_note(), p.jit_note()
        p.close()
    e.close()


# ---- 5. every compiled plan ----------------------------------------------------------------------------------------------
def compiled(n):
    cfg = frontend.load_metadata(META)
    return cfg, frontend.compile_plan(open(os.path.join(META, "%02d.sql.mplan" % n)).read(), cfg)


def run_plan_over_step_images(n, cols):
    """{jit: step_columns()} after the plan ran, results checked against the oracle, with every column encoded both ways"""
    _, text = compiled(n)
    want = oracle_run(text, cols)
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
        e.encode_steps(k)
    out = {}
    for jit in (False, True):
        p = e.parse(text)
        p.set_jit(jit)
        assert p.run()["results"] == want, (n, jit, p.jit_note())
        out[jit] = p.step_columns()
        p.close()
    e.close()
    return out


def synth(n):
    cfg, text = compiled(n)
    return catalog.synth_columns(META, cfg, text, scale=5e-4, seed=3, clustered=(JOIN_INDEX,))


@pytest.mark.parametrize("n", PLANS)
def test_every_compiled_plan_with_step_images_tried_on_every_column(n):
    stepped = run_plan_over_step_images(n, synth(n))
    if n in (12, 14):                                      # aggregate scans bind no step image
        assert stepped == {False: {}, True: {}}, stepped


def names_the_join_index(stepped):
    return all(any(JOIN_INDEX in cols for cols in roles.values()) for roles in stepped.values())


@pytest.mark.parametrize("n", [3, 5, 10])
def test_q3_q5_q10_report_the_join_index(n):
    """the synthetic catalogs' clustered join index holds every order and goes up by 0 or 1 from row to row, as a lineitem written
    order by order does: it qualifies, and Q3, Q5 and Q10 read it through its step image, precompiled and specialised"""
    cols = synth(n)
    d = np.diff(cols[JOIN_INDEX])
    assert d.min() == 0 and d.max() == 1, np.bincount(d).tolist()
    stepped = run_plan_over_step_images(n, cols)
    assert names_the_join_index(stepped), stepped


# ---- 6. two ranks over the host transport --------------------------------------------------------------------------------
def test_two_co_partitioned_ranks_each_with_its_own_step_image():
    text = golden("q3.vdl")
    n_orders, world = 30011, 2
    n_li = 4 * n_orders
    e = m.Engine(device=0)
    keep = datagen.register_q3_columns(e, n_orders)
    want = e.run_vdl(text)["results"]
    assert any(len(list(v.values())[0]) for v in want.values())
    e.close()
    del keep

    def work(rank, rv):
        lo, hi = shard_rows(n_li, rank, world)
        e = m.Engine(device=0)
        keep = datagen.register_q3_columns(e, n_orders, (lo, hi), copartition=True, steps=True)
        info = e.steps_info(JOIN_INDEX)
        e.comm_init_host(rank, world, *rv.transport(rank))
        p = e.parse(text)
        p.set_sharded_table("lineitem")
        p.set_row_offset(lo)
        res = p.run_sharded()["results"]
        stepped = p.step_columns()
        p.close()
        e.close()
        del keep
        return res, stepped, info, hi - lo

    parts = run_ranks(world, work, timeout=600)
    got = {k: {name: sum((part[0][k][name] for part in parts), []) for name in v} for k, v in want.items()}
    assert got == want
    for res, stepped, info, rows in parts:
        assert info == (True, 0, (rows + 63) // 64), info                  # a rebased index: every rank's starts at 0
        assert JOIN_INDEX in stepped.get("front.select", []), stepped


# ---- 7. the environment variable -----------------------------------------------------------------------------------------
def test_the_environment_variable_reaches_vdlrun_encode(tmp_path):
    """VDL_STEP_IMAGES=1 makes vdl_encode_column try a step image, so `vdlrun --encode` reads Q3's join index through one and says
    so.  (--data: `--rows` generates lineitem's own columns only, and Q3 needs orders and customer.)"""
    text = "\n".join(ln.split(";;")[0].rstrip() for ln in golden("q3.vdl").splitlines()) + "\n"
    cols = q3_host_catalog(3001)
    coldir = str(tmp_path / "cols")
    catalog.export_columns(cols, coldir)
    want = oracle_run(text, cols)
    env = {k: v for k, v in os.environ.items() if k != "VDL_STEP_IMAGES"}

    def pipe(flags, extra_env):
        r = subprocess.run([VDLRUN, "--data", coldir] + flags, input=text.encode(), capture_output=True, timeout=600, env=dict(env, **extra_env))
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        assert json.loads(r.stdout.decode())["results"] == want, (flags, extra_env)
        return [ln[len("vdlrun: step images: "):] for ln in r.stderr.decode().splitlines() if ln.startswith("vdlrun: step images: ")]

    lines = pipe(["--encode"], {"VDL_STEP_IMAGES": "1"})
    assert len(lines) == 1 and JOIN_INDEX in parse_step_columns(lines[0]).get("front.select", []), lines
    assert pipe(["--encode"], {}) == []
    lines = pipe(["--encode-steps"], {})
    assert len(lines) == 1 and JOIN_INDEX in parse_step_columns(lines[0]).get("front.select", []), lines
