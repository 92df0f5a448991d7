#!/usr/bin/env python3
"""ORDER BY / LIMIT in a sharded run of TPC-H Q3 (the sharded leg beside tools/order_bench.py): lineitem as W shards, ranks = threads
of this process with one context each on device 0, meeting in an in-process host transport.

    python tools/order_sharded_bench.py [n_orders] [--world W] [--repeats R] [--unordered-only]      default: 15000000 (SF10), W = 8

Three runs of vdl_run_sharded over the same data, alternating:
  (u) unordered                                -- every rank ends with its slice: 4 x m_r values to the host
  (c10)   revenue desc, o_orderdate, limit 10   -- vdl_plan_set_order_sharded: local top-N, one gather, k_ord_merge; 4 x 10 values
  (c4096) the same order, limit 4096
Reported: the wall time of rank 0 around the call (all ranks start together at a barrier and meet in the collectives), the local order
step (timeInMicrosecondsForOrder) and staging + merge (timeInMicrosecondsForOrderMerge) as the largest over the ranks, and the bytes
each rank copies to the host.  EIGHT CONTEXTS ON ONE DEVICE MEASURE THE KERNELS AND THE HOST PATH, NOT THE INTERCONNECT: the collectives
are memcpys through pinned memory and the ranks share the device's queues.  No multi-GPU timing of this exists yet.
--unordered-only runs (u) alone: the leg that must cost what it cost before (run it against a build of the parent commit too)."""
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import mplan2vdl_amd as m
from mplan2vdl_amd import datagen

args = sys.argv[1:]


def option(name, default):
    return int(args[args.index(name) + 1]) if name in args else default


world, repeats = option("--world", 8), option("--repeats", 9)
unordered_only = "--unordered-only" in args
sizes = [int(a) for k, a in enumerate(args) if a.isdigit() and (k == 0 or not args[k - 1].startswith("--"))] or [15000000]
n_orders = sizes[0]
KEYS = [("revenue", True), ("o_orderdate__orders__o_orderdate", False)]
LEGS = ["u"] if unordered_only else ["u", "c10", "c4096"]


class Rendezvous:
    """the collectives of the host transport among the threads of this process"""

    def __init__(self, n):
        self.n, self.barrier, self.slots = n, threading.Barrier(n), [None] * n

    def transport(self, rank):
        def all_gather(send):
            self.slots[rank] = send
            self.barrier.wait()
            out = list(self.slots)
            self.barrier.wait()
            return out

        def all_to_all(pieces):
            self.slots[rank] = pieces
            self.barrier.wait()
            out = [self.slots[src][rank] for src in range(self.n)]
            self.barrier.wait()
            return out

        return all_gather, all_to_all


rv = Rendezvous(world)
text = open(os.path.join(ROOT, "tests", "golden", "q3.vdl")).read()
n_li = 4 * n_orders
report = [None] * world
errors = []


def rank_body(rank):
    try:
        torch.cuda.set_device(0)
        e = m.Engine(0)
        r0, r1 = m.shard_rows(n_li, rank, world)
        keep = datagen.register_q3_columns(e, n_orders, (r0, r1), device="cuda:0", copartition=True)
        e.comm_init_host(rank, world, *rv.transport(rank))
        plans = {}
        for leg in LEGS:
            p = e.parse(text)
            p.set_sharded_table("lineitem")
            p.set_row_offset(r0)
            if leg != "u":
                p.set_order(KEYS, limit=int(leg[1:]), sharded=True)
            plans[leg] = p
        ms = {leg: [] for leg in LEGS}
        step = {leg: {"timeInMicrosecondsForOrder": [], "timeInMicrosecondsForOrderMerge": []} for leg in LEGS}
        for turn in range(2 + repeats):                     # two warm turns: pools, pinned buffers, bindings
            for leg in LEGS:                                # alternating: a drift of the machine falls on all legs alike
                torch.cuda.synchronize()
                rv.barrier.wait()
                t0 = time.perf_counter()
                plans[leg].execute_sharded()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if turn >= 2:
                    ms[leg].append(dt)
                    timings = plans[leg].collect(as_numpy=True)["timings"]
                    for label in step[leg]:
                        if label in timings:
                            step[leg][label].append(timings[label])
        results = {leg: {t: np.asarray(next(iter(v.values()))) for t, v in plans[leg].collect(as_numpy=True)["results"].items()} for leg in LEGS}
        notes = {leg: plans[leg].order_note() for leg in LEGS}
        report[rank] = (ms, step, results, notes)
        for p in plans.values():
            p.close()
        e.close()
        del keep
    except BaseException as exc:          # noqa: BLE001
        errors.append(exc)
        rv.barrier.abort()


threads = [threading.Thread(target=rank_body, args=(r,)) for r in range(world)]
for t in threads:
    t.start()
for t in threads:
    t.join()
if errors:
    raise errors[0]

print("Q3, %d orders (%d lineitems) as %d shards on one device through the host transport, %d alternating repeats" % (n_orders, n_li, world, repeats))
print("  (eight contexts on one device measure the kernels and the host path, not the interconnect; no multi-GPU timing of this exists yet)")
names = {"u": "u: unordered, every rank its slice", "c10": "c10: revenue desc, o_orderdate, limit 10", "c4096": "c4096: revenue desc, o_orderdate, limit 4096"}
full = {t: np.concatenate([report[r][2]["u"][t] for r in range(world)]) for t in report[0][2]["u"]}
rows = len(full["tmp110"])
for leg in LEGS:
    v = report[0][0][leg]
    per_rank = [8 * sum(len(c) for c in report[r][2][leg].values()) for r in range(world)]
    print("  (%s)  rank 0 wall: median %8.3f ms   min %8.3f   max %8.3f   bytes to the host per rank: min %d  max %d" %
          (names[leg], float(np.median(v)), min(v), max(v), min(per_rank), max(per_rank)))
    if leg != "u":
        for label in ("timeInMicrosecondsForOrder", "timeInMicrosecondsForOrderMerge"):
            worst = [max(report[r][1][leg][label][k] for r in range(world)) for k in range(repeats)]
            print("      %s, largest over the ranks: median %d us (min %d, max %d)" % (label, int(np.median(worst)), min(worst), max(worst)))
        print("      rank 0's note: %s" % report[0][3][leg])
        limit = int(leg[1:])
        order = np.lexsort((np.arange(rows), full["tmp115"], ~full["tmp110"]))[:limit]
        ok = all(np.array_equal(report[r][2][leg][t], full[t][order]) for r in range(world) for t in full)
        print("      result rows %d -> %d on every rank; equals np.lexsort over the concatenated unordered slices: %s" % (rows, min(limit, rows), ok))
        if not ok:
            sys.exit(1)
