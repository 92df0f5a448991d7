"""ORDER BY / LIMIT in sharded runs (vdl_plan_set_order_sharded).  Ranks are threads of the test, one context each on device 0, meeting
in the host transport (helpers.run_ranks).  The expected answer everywhere: np.lexsort over the keys with the position in the
UNSHARDED oracle result as the last key, cut to the limit -- the rule of tests/test_order.py -- and every rank must hold exactly that
in every output."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib, catalog, datagen, frontend, shard_rows
from conftest import ROOT, golden
from helpers import engine_with, lineitem, make_heap, oracle_run, prog, run_ranks
from test_comm_gpu import META, lineitem_shards, table_shards
from test_order import LINEITEM_FILTER, columns, expected
from test_order_cpu import program_outputs

pytestmark = pytest.mark.gpu

VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
N_DEV = torch.cuda.device_count()            # (does not initialise the GPU in this process)
REV, DATE = "revenue", "o_orderdate__orders__o_orderdate"


def as_columns(results):
    return columns(results)[2]


def ordered_ranks(text, shards, world, table, orders, fuse=True):
    """Every rank runs `text` once per (keys, limit) of `orders` with the merged order switched on; returns per rank a list of
    (columns, order note, timing labels), or the VdlError the rank raised for that order."""
    def work(rank, rv):
        r0, cols = shards[rank]
        e = engine_with(cols)
        e.comm_init_host(rank, world, *rv.transport(rank))
        p = e.parse(text)
        p.set_fusion(fuse)
        if table:
            p.set_sharded_table(table)
        p.set_row_offset(r0)
        out = []
        for keys, limit in orders:
            p.set_order(keys, limit=limit, sharded=True)
            try:
                res = p.run_sharded(as_numpy=True)
                out.append((as_columns(res["results"]), p.order_note(), sorted(res["timings"])))
            except m.VdlError as exc:
                out.append(exc)
        route = p.sharded_route()
        e.close()
        return route, out

    return run_ranks(world, work, timeout=120)


def check_every_rank(got, want_results, orders, world, route):
    for rank_route, per_order in got:
        assert rank_route == (route, True)
        for (keys, limit), entry in zip(orders, per_order):
            assert not isinstance(entry, Exception), entry
            cols, note, labels = entry
            want, m_rows = expected(want_results, [k[:2] if not isinstance(k, str) else k for k in keys], limit)
            rows = min(limit, m_rows) if limit > 0 else m_rows
            assert list(cols) == list(want)
            for t in want:
                assert len(cols[t]) == rows and np.array_equal(cols[t], want[t]), (t, keys, limit, note)
            if route == "exchange":
                tail = re.search(r" \| merge world=(\d+) candidates=(\d+) rows=(\d+)$", note)
                assert tail and int(tail.group(1)) == world and int(tail.group(3)) == rows and rows <= int(tail.group(2)) <= world * 4096, note
                assert "timeInMicrosecondsForOrderMerge" in labels and "timeInMicrosecondsForOrder" in labels, labels


# ---- the exchange route: TPC-H Q3 -----------------------------------------------------------------------------------------------

Q3 = {}


def q3():
    if not Q3:
        cfg = frontend.load_metadata(META)
        Q3["text"] = frontend.compile_plan(open(os.path.join(META, "03.sql.mplan")).read(), cfg)
        Q3["cols"] = catalog.synth_columns(META, cfg, Q3["text"], scale=6e-4, seed=3)
        Q3["want"] = oracle_run(Q3["text"], Q3["cols"])
    return Q3["text"], Q3["cols"], Q3["want"]


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_q3_merges_the_ranks_first_rows_on_the_exchange_route(world):
    text, cols, want = q3()
    total = len(next(iter(as_columns(want).values())))
    assert total > 10                                      # the cut is real
    keys = [(REV, True), (DATE, False)]
    assert total > 5 * 64                                  # ... also where every rank of five cuts its own run at the limit
    orders = [(keys, 1), (keys, 10), (keys, 64), (keys, 4096), (keys, total + 7), ([], 5), ([(DATE, True)], 10)]
    got = ordered_ranks(text, lineitem_shards(cols, world), world, "lineitem", orders)
    check_every_rank(got, want, orders, world, "exchange")


# ---- a GROUP BY written for the route: one result row per key, in key order; t and total are functions of the key ---------------------

ND = 2048
GROUP_BY = prog(
    "1,Load,f.k", "2,Project,val,Id 1,k", "3,Load,f.v", "4,Project,val,Id 3,v", "5,Load,f.t", "6,Project,val,Id 5,t",
    "7,RangeC,val,0,%d,1" % ND, "8,Partition,val,Id 2,val,Id 7,val", "9,RangeV,val,0,Id 2,1",
    "10,Scatter,Id 2,Id 9,val,Id 8,val", "11,Scatter,Id 4,Id 9,val,Id 8,val", "12,Scatter,Id 6,Id 9,val,Id 8,val",
    "13,FoldSum,val,Id 10,val,Id 11,val", "14,FoldChoose,val,Id 10,val,Id 12,val", "15,FoldChoose,val,Id 10,val,Id 10,val",
    "16,Project,total,Id 13,val", "17,MaterializeCompact,Id 16", "18,Project,t,Id 14,val", "19,MaterializeCompact,Id 18",
    "20,Project,k,Id 15,val", "21,MaterializeCompact,Id 20")


def group_columns(rng, keys, t_of_key):
    """rows in random order; f.t is a function of the key, so the group's chosen t does not depend on which row comes first"""
    k = rng.permutation(np.asarray(keys, dtype=np.int64))
    return {"f.k": k, "f.v": rng.integers(-50, 50, size=len(k)).astype(np.int64), "f.t": np.asarray(t_of_key, dtype=np.int64)[k]}


@pytest.mark.parametrize("fuse,route", [(False, "exchange"), (True, "fold")])
@pytest.mark.parametrize("distinct", [1, 3])
def test_ties_come_out_in_unsharded_program_order_across_the_ranks(distinct, fuse, route):
    """Statement by statement the GROUP BY exchanges its rows and the ranks' first rows are merged; fused it is a dense-domain grouped
    scan whose words are merged, and every rank orders the whole answer."""
    rng = np.random.default_rng(40 + distinct)
    keys = rng.integers(0, 600, size=5000)
    cols = group_columns(rng, keys, np.arange(ND) % distinct + 5)
    want = oracle_run(GROUP_BY, cols)
    n_groups = len(np.unique(keys))
    assert len(as_columns(want)["tmp19"]) == n_groups > 3 * 64 and len(np.unique(as_columns(want)["tmp19"])) == distinct
    orders = [([("t", False)], 64), ([("t", True)], 64), ([("t", True), ("k", True)], 64)]
    got = ordered_ranks(GROUP_BY, table_shards(cols, 3, "f"), 3, "f", orders, fuse=fuse)
    check_every_rank(got, want, orders, 3, route)
    first = got[0][1][0][0]
    if distinct == 1:
        assert first["tmp21"].tolist() == sorted(np.unique(keys))[:64]          # all keys equal: the first 64 groups as they stand


def test_a_rank_without_result_rows_and_a_rank_with_fewer_than_the_limit():
    """Three ranks; the cut of the key domain follows the population: keys 0, 1 (one row each) and 2 (3000 rows) go to rank 0, nothing
    has its middle in rank 1's share, key 3 (2000 rows) and a hundred small groups go to rank 2."""
    rng = np.random.default_rng(9)
    keys = [0, 1] + [2] * 3000 + [3] * 2000 + [k for k in range(10, 110) for _ in range(10)]
    cols = group_columns(rng, keys, (np.arange(ND) * 7919) % 13)
    want = oracle_run(GROUP_BY, cols)
    orders = [([("t", True), ("total", False)], 10), ([("total", False)], 10), ([("k", True)], 10)]
    got = ordered_ranks(GROUP_BY, table_shards(cols, 3, "f"), 3, "f", orders, fuse=False)
    check_every_rank(got, want, orders, 3, "exchange")
    local = [int(re.match(r"topn m=(\d+) ", per_order[0][1]).group(1)) for _, per_order in got]
    assert local == [3, 0, 101], local


def test_every_rank_cuts_its_run_at_a_limit_of_4096():
    """About 20 000 groups over three ranks: every rank holds more than 4096 result rows, so L_r = limit = 4096 < m_r everywhere and
    k_ord_merge ranks 3 x 4096 candidates in runs of full length; t has a thousand values, so most comparisons go to the second key."""
    nd = 20000
    text = GROUP_BY.replace("7,RangeC,val,0,%d,1" % ND, "7,RangeC,val,0,%d,1" % nd)
    rng = np.random.default_rng(77)
    keys = np.concatenate([np.arange(nd), rng.integers(0, nd, size=40000)])
    cols = group_columns(rng, keys, rng.integers(0, 1000, size=nd))
    want = oracle_run(text, cols)
    assert len(as_columns(want)["tmp19"]) == nd
    orders = [([("t", True), ("total", False)], 4096), ([("t", False)], 3000)]
    got = ordered_ranks(text, table_shards(cols, 3, "f"), 3, "f", orders, fuse=False)
    check_every_rank(got, want, orders, 3, "exchange")
    for _, per_order in got:
        note = per_order[0][1]
        assert int(re.match(r"topn m=(\d+) ", note).group(1)) > 4096 and note.endswith("| merge world=3 candidates=12288 rows=4096"), note


@pytest.mark.parametrize("descending", [False, True])
def test_keys_at_both_ends_of_int64(descending):
    rng = np.random.default_rng(3 + descending)
    t = rng.integers(-5, 5, size=ND).astype(np.int64)
    t[rng.choice(400, size=60, replace=False)] = rng.choice(np.array([I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1], dtype=np.int64), size=60)
    cols = group_columns(rng, rng.integers(0, 400, size=4000), t)
    want = oracle_run(GROUP_BY, cols)
    seen = as_columns(want)["tmp19"]
    assert I64_MIN in seen and I64_MAX in seen
    orders = [([("t", descending)], 10), ([("t", descending), ("k", not descending)], 100)]
    got = ordered_ranks(GROUP_BY, table_shards(cols, 2, "f"), 2, "f", orders, fuse=False)
    check_every_rank(got, want, orders, 2, "exchange")


# ---- text keys ----------------------------------------------------------------------------------------------------------------------

def text_case(rng, bad_key=None):
    """t = the code of the key's name in a heap of a few hundred strings written in non-alphabetical order"""
    names = ["%s%03d" % ("zyxwvutsrq"[i % 10] * (1 + i % 4), (i * 37) % 311) for i in range(311)]
    assert names != sorted(names)
    heap, where = make_heap(names)
    code_of_key = np.array([where[names[k % len(names)]] for k in range(ND)], dtype=np.int64)
    if bad_key is not None:
        code_of_key[bad_key] += 1                             # inside a string: names no string of the heap
    keys = rng.integers(0, 500, size=4000)
    if bad_key is not None:
        keys[:3] = bad_key
    cols = group_columns(rng, keys, code_of_key)
    cols["d.name.heap"] = heap
    cols["f.name.heap"] = heap
    text_of_code = {where[s]: s.encode() for s in names}
    return cols, text_of_code


def test_a_text_key_over_a_replicated_heap_and_the_refusal_of_a_sharded_one():
    rng = np.random.default_rng(21)
    cols, text_of_code = text_case(rng)
    want = oracle_run(GROUP_BY, {k: v for k, v in cols.items() if not k.endswith(".heap")})
    res = as_columns(want)
    # the host order by decoded bytes: ranks of the strings take the codes' place, the position decides ties
    rank_of = {s: r for r, s in enumerate(sorted(set(text_of_code.values())))}
    by_text = np.array([rank_of[text_of_code[int(c)]] for c in res["tmp19"]], dtype=np.int64)
    orders = [([("t", False, "d.name.heap")], 10), ([("t", True, "d.name.heap"), ("total", False)], 100), ([("t", False, "f.name.heap")], 10)]
    got = ordered_ranks(GROUP_BY, table_shards(cols, 2, "f"), 2, "f", orders, fuse=False)
    pos = np.arange(len(by_text))
    for route, per_order in got:
        assert route == ("exchange", True)
        a, b, refused = per_order
        order = np.lexsort((pos, by_text))[:10]
        for t in res:
            assert np.array_equal(a[0][t], res[t][order]), (t, a[1])
        assert " text_keys=1 | merge world=2 " in a[1], a[1]
        order = np.lexsort((pos, res["tmp17"], ~by_text))[:100]
        for t in res:
            assert np.array_equal(b[0][t], res[t][order]), (t, b[1])
        assert isinstance(refused, m.VdlError) and refused.code == _lib.VDL_ERR_UNSUPPORTED, refused
    own = [str(per_order[2]) for _, per_order in got]
    assert any("f.name.heap" in msg and "'t'" in msg for msg in own), own          # key and heap are named ...
    assert all("f.name.heap" in msg or "failed on rank" in msg for msg in own), own   # ... and no rank went on alone


def test_a_failure_in_one_ranks_order_step_reaches_every_rank():
    """Only rank 1's result rows hold a code that names no string (the last key of the domain lies in the upper key range): its order
    step fails with VDL_ERR_SHAPE; both ranks raise, neither waits in the gather, and the next run on the same communicator works."""
    rng = np.random.default_rng(22)
    cols, _ = text_case(rng, bad_key=499)
    want = oracle_run(GROUP_BY, {k: v for k, v in cols.items() if not k.endswith(".heap")})
    orders = [([("t", False, "d.name.heap")], 10), ([("total", True)], 10)]
    got = ordered_ranks(GROUP_BY, table_shards(cols, 2, "f"), 2, "f", orders, fuse=False)
    failures = [per_order[0] for _, per_order in got]
    assert all(isinstance(f, m.VdlError) for f in failures), failures
    assert failures[1].code == _lib.VDL_ERR_SHAPE and "d.name.heap" in str(failures[1]), failures[1]
    assert failures[0].code == _lib.VDL_ERR_UNSUPPORTED and "on rank 1" in str(failures[0]), failures[0]
    cut, _ = expected(want, [("total", True)], 10)
    for _, per_order in got:
        assert not isinstance(per_order[1], Exception), per_order[1]
        for t in cut:
            assert np.array_equal(per_order[1][0][t], cut[t])


# ---- routes where every rank holds the whole answer ---------------------------------------------------------------------------------

@pytest.mark.parametrize("query", ["q6", "q1"])
def test_fold_plans_order_the_merged_answer_on_every_rank_also_pipelined(query):
    text = golden(query + ".vdl")
    names = datagen.Q6_COLUMNS if query == "q6" else datagen.Q1_COLUMNS
    n = 100003
    whole = lineitem(names, n)
    want = oracle_run(text, whole)
    outs = program_outputs(text)
    keys = [(outs[-1][1], True), (outs[0][0], False)] if query == "q1" else [("revenue", True)]
    limit = 3 if query == "q1" else 1
    cut, m_rows = expected(want, keys, limit)
    assert m_rows >= limit
    shards = [(lo, {k: v[lo:hi] for k, v in whole.items()}) for lo, hi in (shard_rows(n, r, 2) for r in range(2))]

    def work(rank, rv):
        r0, cols = shards[rank]
        e = engine_with(cols)
        e.comm_init_host(rank, 2, *rv.transport(rank))
        p = e.parse(text)
        p.set_row_offset(r0)
        p.set_order(keys, limit=limit, sharded=True)
        assert p.sharded_route() == ("fold", True)
        res = [as_columns(p.run_sharded(as_numpy=True)["results"])]
        note = p.order_note()
        for k in range(3):                                           # begin / end with two slots: the order is applied in `end`
            p.run_sharded_begin(k & 1)
            if k:
                res.append(as_columns(p.run_sharded_end(1 - (k & 1))["results"]))
        res.append(as_columns(p.run_sharded_end(0)["results"]))
        e.close()
        return res, note

    for res, note in run_ranks(2, work, timeout=120):
        assert len(res) == 4 and note.startswith("host m=%d rows=%d" % (m_rows, limit)), note
        for got in res:
            assert list(got) == list(cut)
            for t in cut:
                assert np.array_equal(got[t], cut[t]), (t, note)


def test_the_front_route_orders_the_whole_answer_on_every_rank():
    cfg = frontend.load_metadata(META)
    text = frontend.compile_plan(open(os.path.join(META, "16.sql.mplan")).read(), cfg)
    cols = catalog.synth_columns(META, cfg, text, scale=2e-3, seed=3)
    want = oracle_run(text, cols)
    tmps = list(want)
    assert len(as_columns(want)[tmps[0]]) > 7
    orders = [([(tmps[-1], True), (tmps[0], False)], 7), ([(tmps[0], True)], 0)]
    got = ordered_ranks(text, table_shards(cols, 2, "partsupp"), 2, "partsupp", orders)
    check_every_rank(got, want, orders, 2, "front")


# ---- the CLI (RCCL: one process per GPU) -------------------------------------------------------------------------------------------------

def gpus(world):
    return pytest.param(world, marks=pytest.mark.skipif(N_DEV < world, reason="needs %d GPUs (this box has %d)" % (world, N_DEV)))


@pytest.mark.parametrize("world", [gpus(1), gpus(2)])
def test_vdlrun_order_sharded_prints_the_one_gpu_answer_once(world):
    """The filter program of tests/test_order.py has no Partition: a whole-answer route.  stdout's results = the one-GPU vdlrun's."""
    order = ["--rows", "60175", "--order-by", "l_shipdate__lineitem__l_shipdate:desc,tmp11:asc", "--limit", "10"]
    one = subprocess.run([VDLRUN] + order, input=LINEITEM_FILTER.encode(), capture_output=True, timeout=300)
    assert one.returncode == 0, one.stderr.decode()[-2000:]
    many = subprocess.run([VDLRUN, "--gpus", str(world), "--order-sharded"] + order, input=LINEITEM_FILTER.encode(), capture_output=True, timeout=300)
    assert many.returncode == 0, many.stderr.decode()[-2000:]
    a, b = json.load(io.BytesIO(one.stdout)), json.load(io.BytesIO(many.stdout))
    assert b["results"] == a["results"] and all(len(next(iter(v.values()))) == 10 for v in b["results"].values())


@pytest.mark.parametrize("world", [gpus(1), gpus(2)])
def test_vdlrun_merges_q3_over_rccl(tmp_path, world):
    """The exchange route through RCCL: Q3 from exported column files, lineitem sharded, the ranks' first rows merged on the device."""
    text, cols, want = q3()
    coldir = str(tmp_path / "cols")
    catalog.export_columns(cols, coldir)
    r = subprocess.run([VDLRUN, "--gpus", str(world), "--shard", "lineitem", "--data", coldir, "--order-sharded", "--order-by",
                        REV + ":desc," + DATE + ":asc", "--limit", "10"], input=text.encode(), capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    reply = json.load(io.BytesIO(r.stdout))
    cut, _ = expected(want, [(REV, True), (DATE, False)], 10)
    assert {t: next(iter(v.values())) for t, v in reply["results"].items()} == {t: v.tolist() for t, v in cut.items()}
    assert "timeInMicrosecondsForOrderMerge" in reply["timings"]
