"""ORDER BY / LIMIT applied on the device (vdl_plan_set_order).  The reference of every check is numpy's lexsort -- keys as signed
int64, key by key, each ascending or descending, ties by the row's position -- over the columns of the SAME plan run without an
order and over the oracle's columns; the ordered run must agree with both on every output column, exactly."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib, datagen, resolve
from conftest import ROOT
from helpers import engine_with, lineitem, oracle_run, prog
from helpers import run_ranks
from test_comm_gpu import lineitem_shards
from test_random_programs import Gen
from test_tpch_plans import META, program_and_columns

pytestmark = pytest.mark.gpu

VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
TOP_MAX, BOUNDARY = 4096, 4096            # kOrdTopMax, kOrdBoundary (vdl_kernels.h): limits up to TOP_MAX select, the selection stops at <= BOUNDARY rows
COMPACT_TILE, ORDER_TILE = 4096, 2048     # compact_tile(): rows per block of the compaction kernels; kOrdTile: rows per block and turn of the order kernels


def golden(name):
    return open(os.path.join(ROOT, "tests", "golden", name)).read()


def host(v):
    if type(v).__name__ == "DeviceValues":
        import torch
        return torch.as_tensor(v, device="cuda:0").cpu().numpy().astype(np.int64)
    return np.asarray(v, dtype=np.int64)


def columns(results):
    """{tmpN: {".name": values}} -> ([tmpN...], {tmpN: name}, {tmpN: int64 array}) in program order"""
    tmps = list(results)
    return tmps, {t: next(iter(results[t]))[1:] for t in tmps}, {t: host(next(iter(results[t].values()))) for t in tmps}


def expected(results, keys, limit):
    """The issue's order over the unordered results: np.lexsort((position, +-k_K, .., +-k_1))[:L] applied to every column.
    (~k reverses the signed order of k and exists for INT64_MIN.)"""
    keys = [(k, False) if isinstance(k, str) else k for k in keys]
    tmps, names, cols = columns(results)
    by = dict((names[t], t) for t in reversed(tmps))
    by.update((t, t) for t in tmps)
    m_rows = len(cols[tmps[0]])
    assert all(len(cols[t]) == m_rows for t in tmps)
    ks = [~cols[by[f]] if d else cols[by[f]] for f, d in keys]
    order = np.lexsort(tuple([np.arange(m_rows, dtype=np.int64)] + ks[::-1])) if ks else np.arange(m_rows)
    if limit > 0:
        order = order[:limit]
    return {t: cols[t][order] for t in tmps}, m_rows


def check_ordered(plan, unordered, oracle_results, keys, limit, path=None):
    plan.set_order(keys, limit=limit)
    res = plan.run(as_numpy=True)
    note = plan.order_note()
    _, _, got = columns(res["results"])
    want, m_rows = expected(unordered, keys, limit)
    rows = min(limit, m_rows) if limit > 0 else m_rows
    assert list(got) == list(want)
    for t in want:
        assert len(got[t]) == rows, (t, len(got[t]), rows, note)          # exactly min(L, m) values leave the engine
        assert np.array_equal(got[t], want[t]), (t, keys, limit, note)
    if oracle_results is not None:
        want2, m2 = expected(oracle_results, keys, limit)
        assert m2 == m_rows
        for t in want2:
            assert np.array_equal(got[t], want2[t]), ("oracle", t, keys, limit, note)
    assert "timeInMicrosecondsForOrder" in res["timings"]
    assert note.split()[0] in ("host", "topn", "sort") and ("m=%d" % m_rows) in note.split() and ("rows=%d" % rows) in note.split(), note
    if path:
        assert note.split()[0] == path, note
    if note.startswith("topn"):
        f = dict(x.split("=") for x in note.split()[1:])
        if f["digits_used_up"] == "0":
            assert int(f["candidates"]) <= limit + BOUNDARY, note
    return res, note


# ---- TPC-H Q3 ---------------------------------------------------------------------------------------------------------------------

REV, DATE, PRIO, OKEY = "revenue", "o_orderdate__orders__o_orderdate", "o_shippriority__orders__o_shippriority", "l_orderkey__lineitem__l_orderkey"
Q3_ORACLE = {}


def q3_oracle(n_orders):
    if n_orders not in Q3_ORACLE:
        Q3_ORACLE[n_orders] = oracle_run(golden("q3.vdl"), datagen.q3_tables(n_orders))
    return Q3_ORACLE[n_orders]


@pytest.mark.parametrize("fusion", [True, False])
@pytest.mark.parametrize("images", [True, False])
@pytest.mark.parametrize("n_orders", [2000, 50000, 1500000])
def test_q3_ordered_and_cut_on_the_device(n_orders, images, fusion):
    text = golden("q3.vdl")
    e = engine_with(datagen.q3_tables(n_orders))
    if images:
        for name in list(datagen.q3_tables(1)):
            e.encode(name)
    e.set_column_images(images)
    p = e.parse(text)
    p.set_fusion(fusion)
    plain = p.run(as_numpy=True)
    want = q3_oracle(n_orders)
    _, _, cols = columns(plain["results"])
    _, _, ocols = columns(want)
    m_rows = len(cols["tmp110"])
    assert m_rows > 100 and all(np.array_equal(cols[t], ocols[t]) for t in ocols)
    assert len(np.unique(cols["tmp120"])) == 1                       # o_shippriority is constant: a key the selection skips whole
    assert len(np.unique(cols["tmp115"])) < m_rows or m_rows < 200   # dates tie
    sel = "topn"
    check_ordered(p, plain["results"], want, [(REV, True), (DATE, False)], 10, sel)
    check_ordered(p, plain["results"], want, [(DATE, True), PRIO, REV], 100, sel)
    check_ordered(p, plain["results"], want, [("tmp110", True), ("tmp115", False)], TOP_MAX, "topn")
    check_ordered(p, plain["results"], want, [(REV, True), (DATE, False)], TOP_MAX + 1, "sort")
    check_ordered(p, plain["results"], want, [(DATE, True), PRIO, REV], 0, "sort")
    check_ordered(p, plain["results"], want, [(OKEY, True)], 0, "sort")
    check_ordered(p, plain["results"], want, [], 7)                  # no keys: the first rows in program order
    # with device outputs the 65536 rule applies to the ordered, cut outputs
    p.set_device_outputs(True)
    res, _ = check_ordered(p, plain["results"], want, [(DATE, True), PRIO, REV], 100, sel)
    assert all(type(next(iter(v.values()))).__name__ == "ndarray" for v in res["results"].values())
    res, _ = check_ordered(p, plain["results"], want, [(REV, True), (DATE, False)], 0, "sort")
    kind = "DeviceValues" if m_rows >= 65536 else "ndarray"
    assert all(type(next(iter(v.values()))).__name__ == kind for v in res["results"].values()), m_rows
    if n_orders == 1500000:
        assert m_rows >= 65536                                       # the full order of the large case does stay in HBM
    p.set_device_outputs(False)
    # cleared: byte-identical results and the same timing labels as a fresh plan
    p.set_order([])
    again = p.run(as_numpy=True)
    fresh_plan = e.parse(text)
    fresh_plan.set_fusion(fusion)
    fresh = fresh_plan.run(as_numpy=True)
    assert p.order_note() == ""
    assert list(again["results"]) == list(fresh["results"]) and sorted(again["timings"]) == sorted(fresh["timings"])
    assert "timeInMicrosecondsForOrder" not in again["timings"]
    for t in fresh["results"]:
        a, b = host(next(iter(again["results"][t].values()))), host(next(iter(fresh["results"][t].values())))
        assert a.tobytes() == b.tobytes() == cols[t].tobytes()
    e.close()


# ---- fused plans: outputs built on the host ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fusion", [True, False])
def test_q1_and_q6_take_the_host_path_when_fused(fusion):
    n = datagen.LINEITEM_ROWS["sf0.01"]
    cols = lineitem(datagen.Q1_COLUMNS, n)
    e = engine_with(cols)
    q1 = golden("q1.vdl")
    want = oracle_run(q1, cols)
    p = e.parse(q1)
    p.set_fusion(fusion)
    plain = p.run(as_numpy=True)
    names = [next(iter(v))[1:] for v in plain["results"].values()]
    flag, status = [x for x in names if x.startswith("l_returnflag")][0], [x for x in names if x.startswith("l_linestatus")][0]
    path = "host" if fusion else None
    check_ordered(p, plain["results"], want, [(flag, True), (status, False)], 0, path)
    check_ordered(p, plain["results"], want, [(flag, True), (status, False)], 1, path)
    check_ordered(p, plain["results"], want, [(status, True), (flag, True)], 3, path)
    q6 = golden("q6.vdl")
    want6 = oracle_run(q6, {k: cols[k] for k in datagen.Q6_COLUMNS})
    p6 = e.parse(q6)
    p6.set_fusion(fusion)
    plain6 = p6.run(as_numpy=True)
    check_ordered(p6, plain6["results"], want6, [("revenue", True)], 1, path)
    check_ordered(p6, plain6["results"], want6, [], 1, path)
    e.close()


# ---- Q10 and Q18 out of the front end, with their SQL's own ORDER BY and LIMIT ---------------------------------------------------------

@pytest.mark.parametrize("n,keys,limit", [(10, [("revenue", True)], 20),                                     # order by revenue desc limit 20
                                          (18, [("o_totalprice", True), ("o_orderdate", False)], 100)])      # order by o_totalprice desc, o_orderdate limit 100
@pytest.mark.parametrize("scale,seed", [(1e-3, 7), (5e-3, 3)])
def test_q10_and_q18_with_their_own_order_and_limit(n, keys, limit, scale, seed):
    from mplan2vdl_amd import frontend
    text, cols = program_and_columns(frontend.load_metadata(META), n, scale, seed)
    want = oracle_run(text, cols)
    e = engine_with(cols)
    p = e.parse(text)
    plain = p.run(as_numpy=True)
    names = [next(iter(v))[1:] for v in plain["results"].values()]
    full = [([x for x in names if x == f or x.startswith(f + "__")][0], d) for f, d in keys]       # the output's full field name
    assert len(next(iter(plain["results"].values())).popitem()[1]) > 0
    plain = p.run(as_numpy=True)
    check_ordered(p, plain["results"], want, full, limit)
    check_ordered(p, plain["results"], want, full, 0)
    e.close()


# ---- single-table programs: FoldSelect + MaterializeCompact of three columns --------------------------------------------------------------

def filter_program(gen_seed=1):
    """Load a, b, c, f; keep the rows where f != 0 (the filter idiom of test_random_programs.Gen: Gather(x, FoldSelect(RangeV 0 1 f, f)));
    outputs ka, kb, kc."""
    g = Gen.__new__(Gen)
    g.lines, g.nid = [], 0
    v = {c: g.project(g.emit("Load,t.%s" % c), c) for c in "abcf"}
    sel = g.emit("FoldSelect,val,Id %d,val,Id %d,val" % (g.rangev(0, v["f"], 1), v["f"]))
    for c in "abc":
        g.emit("MaterializeCompact,Id %d" % g.emit("Project,k%s,Id %d,val" % (c, g.gather(v[c], sel))))
    return prog(*g.lines)


def key_column(rng, kind, n):
    if kind == "few":
        return rng.integers(-2, 2, n, dtype=np.int64)
    if kind == "full":
        x = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        if n >= 4:
            x[:4] = [I64_MIN, I64_MAX, -1, 0]
        return x
    if kind == "constant":
        return np.full(n, -7, np.int64)
    return rng.integers(-10**9, 10**9, n, dtype=np.int64)


SIZES = [1, ORDER_TILE - 1, ORDER_TILE, ORDER_TILE + 1, COMPACT_TILE - 1, COMPACT_TILE, COMPACT_TILE + 1, 2 * BOUNDARY + 1, 70001]


@pytest.mark.parametrize("kinds", [("few", "full", "mid"), ("full", "few", "constant"), ("constant", "few", "full"), ("few", "few", "few"),
                                   ("mid", "constant", "few")])
@pytest.mark.parametrize("n", SIZES)
def test_filtered_columns_ordered_at_tile_edges(n, kinds):
    rng = np.random.default_rng(n * 31 + len("".join(kinds)))
    text = filter_program()
    for keep in ("all", "most", "none"):
        cols = {"t.%s" % c: key_column(rng, k, n) for c, k in zip("abc", kinds)}
        cols["t.f"] = np.ones(n, np.int64) if keep == "all" else (rng.integers(0, 8, n) > 0).astype(np.int64) if keep == "most" else np.zeros(n, np.int64)
        want = oracle_run(text, cols)
        e = engine_with(cols)
        p = e.parse(text)
        plain = p.run(as_numpy=True)
        for limit in (1, 7, TOP_MAX):
            for keys in ([("ka", False), ("kb", True), ("kc", False)], [("kc", True), ("ka", True)], [("kb", False)]):
                _, note = check_ordered(p, plain["results"], want, keys, limit)
                if keep != "none" and n > 1:
                    assert note.startswith("topn"), note
        check_ordered(p, plain["results"], want, [("ka", True), ("kb", False), ("kc", True)], 0)
        check_ordered(p, plain["results"], want, [("kb", True)], TOP_MAX + 1)
        e.close()


def test_selection_adversaries():
    text = filter_program()
    n = 1000003
    rng = np.random.default_rng(5)
    # every row equal on every key: the digits are used up at once, the answer is the first L positions
    cols = {"t.a": np.full(n, 5, np.int64), "t.b": np.full(n, I64_MIN, np.int64), "t.c": np.arange(n, dtype=np.int64), "t.f": np.ones(n, np.int64)}
    e = engine_with(cols)
    p = e.parse(text)
    plain = p.run(as_numpy=True)
    for limit in (1, 10, TOP_MAX):
        res, note = check_ordered(p, plain["results"], None, [("ka", True), ("kb", False)], limit, "topn")
        assert "digits_used_up=1" in note and "rounds=0" in note, note
        assert np.array_equal(host(res["results"]["tmp19"][".kc"]), np.arange(limit))
    check_ordered(p, plain["results"], None, [("ka", True), ("kb", False)], 0, "sort")
    e.close()
    # keys equal except in the lowest bit of the LAST key
    low = rng.integers(0, 2, n, dtype=np.int64)
    for base in (0, I64_MAX - 1, I64_MIN):
        cols = {"t.a": np.full(n, -3, np.int64), "t.b": np.full(n, I64_MAX, np.int64), "t.c": base + low, "t.f": np.ones(n, np.int64)}
        e = engine_with(cols)
        p = e.parse(text)
        plain = p.run(as_numpy=True)
        for desc in (False, True):
            _, note = check_ordered(p, plain["results"], None, [("ka", False), ("kb", True), ("kc", desc)], 10, "topn")
            assert "digits_used_up=1" in note and "rounds=1" in note, note
            check_ordered(p, plain["results"], None, [("ka", False), ("kb", True), ("kc", desc)], TOP_MAX, "topn")
        e.close()
    # a hot digit, round after round: all rows but two share the leading 43 bits, so the first rounds find (nearly) every row in one bin
    c = rng.integers(0, 1 << 20, n, dtype=np.int64)
    c[123], c[77] = 1 << 62, -(1 << 62)
    cols = {"t.a": c, "t.b": rng.integers(0, 3, n, dtype=np.int64), "t.c": np.arange(n, dtype=np.int64)[::-1].copy(), "t.f": np.ones(n, np.int64)}
    e = engine_with(cols)
    p = e.parse(text)
    plain = p.run(as_numpy=True)
    for desc in (False, True):
        for limit in (1, 2, 10, TOP_MAX):
            _, note = check_ordered(p, plain["results"], None, [("ka", desc), ("kb", not desc)], limit, "topn")
            if limit > 2:
                assert int(dict(x.split("=") for x in note.split()[1:])["rounds"]) >= 4, note
    check_ordered(p, plain["results"], None, [("ka", True), ("kb", False)], 0, "sort")           # a range beyond 2^62: sorted as two halves
    e.close()
    # fewer rows than the limit
    cols = {"t.a": key_column(rng, "full", 37), "t.b": key_column(rng, "few", 37), "t.c": key_column(rng, "mid", 37), "t.f": np.ones(37, np.int64)}
    e = engine_with(cols)
    p = e.parse(text)
    plain = p.run(as_numpy=True)
    res, _ = check_ordered(p, plain["results"], oracle_run(text, cols), [("ka", True), ("kb", False)], 100, "topn")
    assert len(host(res["results"]["tmp19"][".kc"])) == 37
    e.close()
    # a first key of four values (each on a quarter of the rows, far more than the selection's stop), a constant second key -- skipped
    # whole -- and a third that decides: the selection walks through the skipped key and reaches the third
    cols = {"t.a": rng.integers(0, 4, n, dtype=np.int64), "t.b": np.full(n, 9, np.int64), "t.c": key_column(rng, "full", n), "t.f": np.ones(n, np.int64)}
    e = engine_with(cols)
    p = e.parse(text)
    plain = p.run(as_numpy=True)
    for desc in (False, True):
        _, note = check_ordered(p, plain["results"], None, [("ka", desc), ("kb", True), ("kc", not desc)], 100, "topn")
        f = dict(x.split("=") for x in note.split()[1:])
        assert f["digits_used_up"] == "0" and int(f["rounds"]) >= 2 and int(f["candidates"]) <= 100 + BOUNDARY, note
    e.close()


def test_outputs_of_different_lengths_are_refused_with_their_names():
    g = Gen.__new__(Gen)
    g.lines, g.nid = [], 0
    a = g.project(g.emit("Load,t.a"), "a")
    f = g.project(g.emit("Load,t.f"), "f")
    sel = g.emit("FoldSelect,val,Id %d,val,Id %d,val" % (g.rangev(0, f, 1), f))
    g.emit("MaterializeCompact,Id %d" % g.emit("Project,filtered,Id %d,val" % g.gather(a, sel)))
    g.emit("MaterializeCompact,Id %d" % g.emit("Project,whole,Id %d,val" % a))
    text = prog(*g.lines)
    e = engine_with({"t.a": np.arange(100, dtype=np.int64), "t.f": (np.arange(100) % 2).astype(np.int64)})
    p = e.parse(text)
    p.set_order([("whole", True)], limit=3)
    with pytest.raises(m.VdlError) as ei:
        p.run()
    assert ei.value.code == _lib.VDL_ERR_SHAPE
    assert "filtered" in str(ei.value) and "whole" in str(ei.value) and "50" in str(ei.value) and "100" in str(ei.value)
    p.set_order([])
    assert [len(next(iter(v.values()))) for v in p.run()["results"].values()] == [50, 100]
    e.close()


# ---- sharded runs refuse; the CLI end to end -----------------------------------------------------------------------------------------------

def test_run_sharded_refuses_an_ordered_plan():
    text = golden("q6.vdl")
    cols = lineitem(datagen.Q6_COLUMNS, 5000)
    shards = lineitem_shards(cols, 1)

    def work(rank, rv):
        r0, mine = shards[rank]
        e = engine_with(mine)
        e.comm_init_host(rank, 1, *rv.transport(rank))
        p = e.parse(text)
        p.set_order([("revenue", True)], limit=1)
        with pytest.raises(m.VdlError) as ei:
            p.run_sharded()
        assert ei.value.code == _lib.VDL_ERR_UNSUPPORTED and "disjoint result rows" in str(ei.value) and "not built" in str(ei.value)
        p.set_order([])
        res = p.run_sharded()["results"]
        e.close()
        return res

    assert run_ranks(1, work)[0] == oracle_run(text, cols)


LINEITEM_FILTER = prog(
    "1,Load,lineitem.l_quantity", "2,Project,val,Id 1,l_quantity", "3,RangeV,val,4900,Id 2,0", "4,Greater,val,Id 2,val,Id 3,val",
    "5,RangeV,val,0,Id 4,1", "6,FoldSelect,val,Id 5,val,Id 4,val",
    "7,Load,lineitem.l_extendedprice", "8,Project,val,Id 7,l_extendedprice", "9,Gather,Id 8,Id 6,val",
    "10,Project,l_extendedprice__lineitem__l_extendedprice,Id 9,val", "11,MaterializeCompact,Id 10",
    "12,Load,lineitem.l_shipdate", "13,Project,val,Id 12,l_shipdate", "14,Gather,Id 13,Id 6,val",
    "15,Project,l_shipdate__lineitem__l_shipdate,Id 14,val", "16,MaterializeCompact,Id 15",
    "17,Load,lineitem.l_returnflag", "18,Project,val,Id 17,l_returnflag", "19,Gather,Id 18,Id 6,val",
    "20,Project,l_returnflag__lineitem__l_returnflag,Id 19,val", "21,MaterializeCompact,Id 20")


@pytest.mark.parametrize("rows", [60175, 600000])
def test_vdlrun_order_by_and_limit_through_resolve(rows):
    cols = lineitem(["lineitem.l_quantity", "lineitem.l_extendedprice", "lineitem.l_shipdate", "lineitem.l_returnflag"], rows)
    want = oracle_run(LINEITEM_FILTER, cols)
    keys = [("l_shipdate__lineitem__l_shipdate", True), ("l_extendedprice__lineitem__l_extendedprice", False)]
    cut, m_rows = expected(want, keys, 10)
    assert m_rows > 10
    r = subprocess.run([VDLRUN, "--rows", str(rows), "--order-by", "l_shipdate__lineitem__l_shipdate:desc,tmp11:asc", "--limit", "10"],
                       input=LINEITEM_FILTER.encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    reply = json.load(io.BytesIO(r.stdout))
    assert list(reply["results"]) == ["tmp11", "tmp16", "tmp21"]
    for t, entry in reply["results"].items():
        (k, v), = entry.items()
        assert k.startswith(".") and all(isinstance(x, int) for x in v) and v == cut[t].tolist()
    assert "timeInMicrosecondsForOrder" in reply["timings"]
    names, decoded = resolve.decode(reply, resolve.load_dictionary(os.path.join(META, "dictionary.csv")))
    assert len(names) == 3 and len(decoded) == 10 and all(len(row) == 3 for row in decoded)
    raw = {k: v for k, v in zip(names, zip(*decoded))}
    date = [k for k in raw if "l_shipdate" in k][0]
    assert list(raw[date]) == cut["tmp16"].tolist()                   # dates have no dictionary: they come through as they are, in order
    # the CLI's refusal with --gpus
    r = subprocess.run([VDLRUN, "--gpus", "2", "--rows", str(rows), "--order-by", "tmp11", "--limit", "10"], input=LINEITEM_FILTER.encode(),
                       capture_output=True, timeout=120)
    assert r.returncode != 0 and b"disjoint result rows" in r.stderr
