#!/usr/bin/env python3
"""What ORDER BY / LIMIT on the device is worth on TPC-H Q3: three ways to end the same query, alternating in one process.

    python tools/order_bench.py [n_orders ...] [--repeats R] [--only-ordered]        default: 15000000 (SF10) 150000000 (SF100)

  (a) unordered, results to the host      -- 4 x m values over PCIe (the path of a plan with no order set)
  (b) unordered, results left in HBM      -- vdl_plan_set_device_outputs
  (c) revenue desc, o_orderdate, limit 10 -- vdl_plan_set_order: 4 x 10 values leave the device
Each is vdl_run alone (Plan.execute: the outputs stay in the plan), wall time around it with the device idle before and after.
Prints ms per query for each (median, min, max over the repeats), the order step's timeInMicrosecondsForOrder, the order note,
and checks (c)'s ten rows against np.lexsort over (b)'s columns.  --only-ordered runs (c) alone (for a kernel trace)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import mplan2vdl_amd as m
from mplan2vdl_amd import catalog, datagen, frontend

args = sys.argv[1:]
repeats = int(args[args.index("--repeats") + 1]) if "--repeats" in args else 9
only_ordered = "--only-ordered" in args
sizes = [int(a) for k, a in enumerate(args) if a.isdigit() and (k == 0 or args[k - 1] != "--repeats")] or [15000000, 150000000]
KEYS = [("revenue", True), ("o_orderdate__orders__o_orderdate", False)]


def q3_text(n_orders):
    text = open(os.path.join(ROOT, "tests", "golden", "q3.vdl")).read()
    if n_orders > 15000000:          # the fixture was compiled against the SF10 catalog; larger data needs the program for its own bounds
        meta = os.path.join(ROOT, "tests", "golden", "tpch10noorder")
        factor = -(-n_orders // 15000000)
        text = frontend.compile_plan(open(os.path.join(meta, "03.sql.mplan")).read(), catalog.tpch_scaled_config(frontend.load_metadata(meta), factor))
    return text


def once(plan):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan.execute()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host(v):
    return torch.as_tensor(v, device="cuda:0").cpu().numpy() if type(v).__name__ == "DeviceValues" else np.asarray(v)


for n_orders in sizes:
    torch.cuda.set_device(0)
    e = m.Engine(0)
    e.use_torch_stream()
    keep = datagen.register_q3_columns(e, n_orders, device="cuda:0")
    text = q3_text(n_orders)
    plans = {}
    if not only_ordered:
        plans["a: unordered, to the host"] = e.parse(text)
        plans["b: unordered, left in HBM"] = e.parse(text)
        plans["b: unordered, left in HBM"].set_device_outputs(True)
    plans["c: revenue desc, o_orderdate, limit 10"] = e.parse(text)
    plans["c: revenue desc, o_orderdate, limit 10"].set_order(KEYS, limit=10)
    ms = {k: [] for k in plans}
    order_us = []
    for p in plans.values():          # warm: pools, pinned buffers, bindings
        once(p); once(p)
    for _ in range(repeats):          # alternating: a drift of the machine falls on all three alike
        for k, p in plans.items():
            ms[k].append(once(p))
            if k.startswith("c"):
                order_us.append(p.collect(as_numpy=True)["timings"]["timeInMicrosecondsForOrder"])
    print("Q3, %d orders (%d lineitems), %d alternating repeats" % (n_orders, 4 * n_orders, repeats))
    for k, v in ms.items():
        print("  (%s)  median %8.3f ms   min %8.3f   max %8.3f" % (k, float(np.median(v)), min(v), max(v)))
    pc = plans["c: revenue desc, o_orderdate, limit 10"]
    print("  order step: timeInMicrosecondsForOrder median %d us (min %d, max %d); note: %s" % (int(np.median(order_us)), min(order_us), max(order_us), pc.order_note()))
    if not only_ordered:
        got = {t: host(next(iter(v.values()))) for t, v in pc.collect(as_numpy=True)["results"].items()}
        pb = plans["b: unordered, left in HBM"]
        pb.execute()
        full = {t: host(next(iter(v.values()))) for t, v in pb.collect(as_numpy=True)["results"].items()}
        rows = len(full["tmp110"])
        order = np.lexsort((np.arange(rows), full["tmp115"], ~full["tmp110"]))[:10]
        ok = all(np.array_equal(got[t], full[t][order]) for t in full)
        print("  result rows %d -> %d; (c) equals np.lexsort over (b)'s columns: %s" % (rows, len(got["tmp110"]), ok))
        if not ok:
            sys.exit(1)
    for p in plans.values():
        p.close()
    e.close()
    del keep
    torch.cuda.empty_cache()
