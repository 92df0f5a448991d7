#!/usr/bin/env python3
"""What lookup images are worth on the two join workloads that are short of their lookups: TPC-H Q14 (a fused join scan that looks
part.p_type up through lineitem_part) and Q3 (a fused front whose take side fetches o_orderdate / o_shippriority line by isolated line).

    python tools/lookup_bench.py --query q14|q3 [--rows N] [--repeats R] [--legs ab|off|on] [--jit tune|on|off] [--out FILE]

--rows: lineitem rows (default SF100: 600 037 902 lineitems and 20 M parts for Q14; 600 M lineitems, 150 M orders for Q3).
Two legs, alternating in one process: (off) the default -- lookups read the catalog columns -- and (on) Engine.set_lookup_images.
Each leg has a context and a plan of its own over the same generated columns (same seed), so that flipping the switch never
re-binds or re-tunes a plan between timed runs; Q14's part.p_type is encoded in both (datagen.register_q14_columns(lookup_images=True)),
and only the switch differs.  Wall time around each run with the device idle before and after, medians of R (default 9) with
min .. max; the scan kernel's own time (HIP events, Q14) beside it.  The legs' answers must be equal.
--legs off | on runs one leg alone: `off` is what a tree without the switch can run (the parent commit, as a process of its own),
and one leg per process is what a counters-only `rocprofv3 --pmc FETCH_SIZE -- python tools/lookup_bench.py --legs on ...` wants
(FETCH_SIZE x 2 of the scan kernel is the one figure that includes the dimension-side lines; vdl_plan_scan_traffic counts
fact-table lines only)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import mplan2vdl_amd as m
from mplan2vdl_amd import datagen

args = sys.argv[1:]


def opt(name, default):
    return args[args.index(name) + 1] if name in args else default


query = opt("--query", "q14")
rows = int(opt("--rows", datagen.LINEITEM_ROWS["sf100"]))
repeats = int(opt("--repeats", 9))
legs = {"ab": ["off", "on"], "off": ["off"], "on": ["on"]}[opt("--legs", "ab")]
jit = opt("--jit", "tune")
out_path = opt("--out", None)
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, got


def stats(v, unit="ms"):
    return "median %9.3f %s   min %9.3f   max %9.3f" % (float(np.median(v)), unit, min(v), max(v))


def host(values):
    if hasattr(values, "__cuda_array_interface__"):
        return torch.as_tensor(values, device="cuda").cpu().numpy()
    return np.asarray(values, dtype=np.int64).reshape(-1)


class Leg:
    """one context with the switch on or off, the workload's columns generated in it, one plan"""

    def __init__(self, on):
        self.on = on
        self.e = m.Engine(0)
        if on:
            self.e.set_lookup_images(True)          # (a tree without the switch runs --legs off and never gets here)
        if query == "q14":
            try:
                self.keep = datagen.register_q14_columns(self.e, rows, lookup_images=True)
            except TypeError:                       # the parent commit's generator: no parameter, p_type not encoded
                self.keep = datagen.register_q14_columns(self.e, rows)
            text = open(os.path.join(ROOT, "tests", "golden", "q14.vdl")).read()
        else:
            import bench
            self.keep = datagen.register_q3_columns(self.e, rows // 4)
            text = bench.q3_program(rows // 4)
        self.p = self.e.parse(text)
        self.p.set_profiling(True)
        if jit != "off":
            self.p.set_jit(True, tune=(jit == "tune" and query == "q14"))
        if query == "q3":
            self.p.set_device_outputs(True)
        self.wall, self.kernel, self.timings = [], [], {}

    def run(self):
        if query == "q14":
            r = self.p.run()
            self.timings = r["timings"]
            return r["results"]
        self.p.execute()
        return None

    def answer(self):
        if query == "q14":
            return self.p.run()["results"]
        res = self.p.collect()
        self.timings = res["timings"]
        return {k: {f: host(x).tolist() for f, x in v.items()} for k, v in res["results"].items()}

    def lookups(self):
        return self.p.lookup_columns() if hasattr(self.p, "lookup_columns") else "(this tree has no lookup images)"


torch.cuda.set_device(0)
say("lookup_bench: %s, %d lineitem rows, legs %s, jit %s, %d repeats" % (query, rows, "+".join(legs), jit, repeats))
L = {name: Leg(name == "on") for name in legs}
for name, leg in L.items():
    for _ in range(3):                              # warm: builds, tunes, sizes the front's outputs
        leg.run()
    torch.cuda.synchronize()
for _ in range(repeats):
    for name, leg in L.items():                     # alternating
        ms, _ = once(leg.run)
        leg.wall.append(ms)
        if query == "q14":
            leg.kernel.append(leg.p.scan_stats()[2])
answers = {name: leg.answer() for name, leg in L.items()}
if len(L) == 2:
    assert answers["off"] == answers["on"], "the legs' answers differ"
    say("answers of the two legs are equal")
first = next(iter(answers.values()))
say("answer: %s" % {k: {f: (x if len(x) <= 4 else "%d rows, sum %d" % (len(x), int(np.asarray(x, dtype=np.int64).sum()))) for f, x in v.items()} for k, v in first.items()})
for name, leg in L.items():
    say("leg %-3s wall    %s" % (name, stats(leg.wall)))
    if leg.kernel:
        say("leg %-3s kernel  %s" % (name, stats(leg.kernel, "us")))
    say("leg %-3s lookup columns: %s" % (name, leg.lookups()))
    say("leg %-3s timings: %s" % (name, {k.replace("timeInMicrosecondsFor", ""): round(v, 1) for k, v in leg.timings.items()}))
    say("leg %-3s kernels: %s" % (name, leg.p.jit_note()[:900]))
if len(L) == 2:
    a, b = float(np.median(L["off"].wall)), float(np.median(L["on"].wall))
    say("on / off (median wall): %.3f" % (b / a))
    if L["off"].kernel:
        say("on / off (median kernel): %.3f" % (float(np.median(L["on"].kernel)) / float(np.median(L["off"].kernel))))
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
for leg in L.values():
    leg.p.close()
    leg.e.close()
