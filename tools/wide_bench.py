#!/usr/bin/env python3
"""What wide sums cost: Q6 and Q1 over the generator's lineitem, tuned specialised scans, with the switch off
and in mode 1 -- and, with --parent DIR, against a build of the parent commit (DIR holds that commit's mplan2vdl_amd package with its
libvdl.so built) -- taken as ALTERNATING FRESH PROCESSES, `--repeats` per side: every process generates the columns, tunes its scan at
one untimed query, warms up and times `--steps` queries.  Reported per query and side: the median over the processes of each
process's median kernel time (HIP events around the scan and its finish step) and wall time per query, with min .. max; the bytes one
launch moves (vdl_plan_scan_traffic), which must be equal on all sides; the ratios to the parent (or to the switch-off side).  Mode 1
also reports the largest sum_charge of Q1 as a fraction of INT64_MAX.

--wrap-rows N: Q1 at N rows, where the generator's data really wraps: once in mode 2 (the run must fail with VDL_ERR_OVERFLOW) and once
in mode 1 (the exact values).  A child that fails ends the whole measurement: nothing more is started on the device.

    python tools/wide_bench.py --sf sf100 --repeats 3 --steps 20 --parent /path/to/parent/tree --out profiles/r20/wide_bench.txt

--sharded: the sharded leg (DESIGN.md section 5.17 "Sharded runs") instead: every process opens a ONE-RANK RCCL communicator and steps
through vdl_run_sharded_begin / _end over two slots, query k + 1 begun before query k is collected; a step is one begin plus the
collection of the query before it, timed on the host.  Five sides: the parent's plain sharded step (with --parent), this tree's with
the switch off -- the same path, so the two must agree within the spread of the repeats --, this tree's wide sharded step (mode 1 with
vdl_plan_set_wide_sums_sharded), one vdl_run_sharded call per query in mode 1, and vdl_run in mode 1 on the same rows.  Against
vdl_run the single call shows what the wider block, the merge kernel and the second copy cost with nothing hidden, and the pipelined
step what is left of it once the copy-out runs behind the next scan.  One rank on one device: no multi-GPU timing is taken.

    python tools/wide_bench.py --sharded --rows 75004738 --repeats 3 --steps 40 --parent /path/to/parent/tree --out profiles/r21/wide_sharded.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MAX = (1 << 63) - 1


def child(args):
    root = os.path.abspath(args.root or ROOT)
    sys.path.insert(0, root)
    import mplan2vdl_amd as m
    from mplan2vdl_amd import datagen

    rows = args.rows or datagen.LINEITEM_ROWS[args.sf]
    eng = m.Engine(device=0)
    for name in (datagen.Q6_COLUMNS if args.query == "q6" else datagen.Q1_COLUMNS):
        eng.generate(datagen.LINEITEM[name], 0, rows)
    plan = eng.parse(open(os.path.join(ROOT, "tests", "golden", args.query + ".vdl")).read())
    plan.set_profiling(True)
    plan.set_jit(True, tune=True)
    if args.mode and args.leg.startswith("sharded"):
        plan.set_wide_sums(args.mode, sharded=True)
    elif args.mode:
        plan.set_wide_sums(args.mode)                          # (never called on the parent's package: it has no such switch)
    out = {"query": args.query, "mode": args.mode, "rows": rows, "root": root}
    if args.leg.startswith("sharded"):
        return sharded_child(args, eng, plan, out)
    try:
        res = plan.run()                                       # builds, tunes
    except m.VdlError as exc:
        out.update({"error_code": exc.code, "message": str(exc)})
        print(json.dumps(out))
        return 0
    for _ in range(args.warmup):
        plan.execute()
    scan, wall = [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        plan.execute()                                         # (returns with the outputs assembled: the device is idle again)
        wall.append((time.perf_counter() - t0) * 1e6)
        scan.append(plan.scan_stats()[2])
    moved, detail = plan.scan_traffic()
    fields = {name[1:]: [int(x) for x in vals] for f in res["results"].values() for name, vals in f.items()}
    out.update({"scan_us": scan, "wall_us": wall, "bytes_moved": moved, "traffic": detail, "kernel": [k for k in res["timings"] if "FusedScan_" in k],
                "jit_note": plan.jit_note(), "wide_note": plan.wide_note() if args.mode else "", "results": fields})
    print(json.dumps(out))
    eng.close()
    return 0


def sharded_child(args, eng, plan, out):
    """the pipelined sharded step on a one-rank RCCL communicator: begin(k), then collect k - 1"""
    import mplan2vdl_amd as m

    eng.comm_init_rccl(0, 1, eng.comm_unique_id())
    try:
        res = plan.run_sharded()                               # builds, tunes
    except m.VdlError as exc:
        out.update({"error_code": exc.code, "message": str(exc)})
        print(json.dumps(out))
        return 0
    L, c, h = eng._L, eng._c, plan._h
    if args.leg == "sharded1":                                 # one vdl_run_sharded per step: local phase, merge and finalisation, nothing overlapped
        for _ in range(args.warmup):
            eng._check(L.vdl_run_sharded(c, h))
        wall = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            eng._check(L.vdl_run_sharded(c, h))
            wall.append((time.perf_counter() - t0) * 1e6)
        fields = {name[1:]: [int(x) for x in vals] for f in res["results"].values() for name, vals in f.items()}
        out.update({"scan_us": [plan.scan_stats()[2]], "wall_us": wall, "bytes_moved": 0, "traffic": "", "kernel": [k for k in plan.collect()["timings"] if "FusedScan_" in k],
                    "jit_note": plan.jit_note(), "wide_note": plan.wide_note() if args.mode else "", "results": fields})
        print(json.dumps(out))
        eng.close()
        return 0

    def step(k):                                               # (the C calls alone: converting the outputs to Python is no part of a step)
        eng._check(L.vdl_run_sharded_begin(c, h, k & 1))
        if k:
            eng._check(L.vdl_run_sharded_end(c, h, 1 - (k & 1)))

    for k in range(args.warmup + 1):
        step(k)
    wall = []
    for k in range(args.warmup + 1, args.warmup + 1 + args.steps):
        t0 = time.perf_counter()
        step(k)
        wall.append((time.perf_counter() - t0) * 1e6)
    eng._check(L.vdl_run_sharded_end(c, h, (args.warmup + args.steps) & 1))
    last = plan.collect()
    fields = {name[1:]: [int(x) for x in vals] for f in res["results"].values() for name, vals in f.items()}
    same = {name[1:]: [int(x) for x in vals] for f in last["results"].values() for name, vals in f.items()} == fields
    out.update({"scan_us": [plan.scan_stats()[2]], "wall_us": wall, "bytes_moved": 0, "traffic": "", "kernel": [k for k in last["timings"] if "FusedScan_" in k],
                "jit_note": plan.jit_note(), "wide_note": plan.wide_note() if args.mode else "", "results": fields, "last_equals_first": same})
    print(json.dumps(out))
    eng.close()
    return 0


def sharded_main(args, say, spawn):
    """--sharded: alternating fresh processes, five sides"""
    sides = ([("parent", 0, args.parent, "sharded")] if args.parent else []) + [("off", 0, None, "sharded"), ("wide", 1, None, "sharded"), ("wide1", 1, None, "sharded1"), ("run", 1, None, "")]
    names = {"parent": "parent, plain sharded step", "off": "this tree, switch off, sharded step", "wide": "this tree, wide sharded step (mode 1)",
             "wide1": "this tree, vdl_run_sharded in mode 1", "run": "this tree, vdl_run in mode 1"}
    queries = [q for q in args.queries.split(",") if q]
    got = {}
    for rep in range(args.repeats):
        for query in queries:
            for side, mode, root, leg in sides:
                r = spawn(query, mode, root, args.rows, leg)
                if "error_code" in r:
                    say("FAILED: %s %s: [%d] %s" % (query, side, r["error_code"], r["message"]))
                    raise SystemExit(1)
                got.setdefault((query, side), []).append(r)
                say("round %d %s %-6s step %s us  %s" % (rep, query, side, spread(r["wall_us"]), r["kernel"]))
    say()
    say("One rank on one device (a one-rank RCCL communicator: no gather, the merge kernel reads the send buffer).  No multi-GPU timing exists")
    say("or was taken: what a wider all-gather costs between devices is not in these numbers.")
    say()
    for query in queries:
        say("%s at %d rows, %d processes per side, %d timed steps each: median over processes of the process medians (min .. max), host microseconds per step" %
            (query, got[(query, "off")][0]["rows"], args.repeats, args.steps))
        med, spreads = {}, {}
        for side, _, _, _ in sides:
            xs = [statistics.median(r["wall_us"]) for r in got[(query, side)]]
            med[side], spreads[side] = statistics.median(xs), max(xs) - min(xs)
            say("  %-40s %s   %s" % (names[side], spread(xs), got[(query, side)][-1]["kernel"]))
        if args.parent:
            d = med["off"] - med["parent"]
            say("  switch off - parent: %+.1f us (ratio %.4f); spread of the repeats: parent %.1f us, switch off %.1f us -> %s" %
                (d, med["off"] / med["parent"], spreads["parent"], spreads["off"], "within the spread" if abs(d) <= max(spreads["parent"], spreads["off"]) else "OUTSIDE the spread"))
        say("  wide sharded step - vdl_run in mode 1: %+.1f us (ratio %.4f): what the wider block, the merge kernel and the second copy add, less what the" %
            (med["wide"] - med["run"], med["wide"] / med["run"]))
        say("      pipelined step hides (vdl_run waits for its copy-out; a sharded step collects the query before, whose copy ran behind this one's scan)")
        say("  vdl_run_sharded in mode 1 (one call per query, nothing overlapped) - vdl_run in mode 1: %+.1f us (ratio %.4f): the wider block, the merge" %
            (med["wide1"] - med["run"], med["wide1"] / med["run"]))
        say("      kernel, the second copy and the hop to the communication stream, with nothing hidden")
        say("  wide sharded step / switch-off sharded step: %.4f" % (med["wide"] / med["off"]))
        wide, off, run = (got[(query, s)][-1]["results"] for s in ("wide", "off", "run"))
        say("  wide sharded results == vdl_run's in mode 1: %s; low words == the switch-off sharded results: %s; every pipelined answer its own: %s" %
            (wide == run, all([(x & ((1 << 64) - 1)) for x in wide[k]] == [(x & ((1 << 64) - 1)) for x in off[k]] for k in off),
             all(r.get("last_equals_first", True) for s in ("off", "wide") for r in got[(query, s)])))
        say("  wide note: %s" % got[(query, "wide")][-1]["wide_note"])
        say()


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--query", default="q6")
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--root", default=None)
    ap.add_argument("--sf", default="sf100")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a tree of the parent commit, built: the third side")
    ap.add_argument("--wrap-rows", type=int, default=0)
    ap.add_argument("--queries", default="q6,q1")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sharded", action="store_true", help="the sharded leg: begin / end steps on a one-rank RCCL communicator")
    ap.add_argument("--leg", default="", help="(child) sharded: the pipelined sharded step instead of vdl_run")
    args = ap.parse_args()
    if args.child:
        return child(args)

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def spawn(query, mode, root, rows, leg=""):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--query", query, "--mode", str(mode), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--sf", args.sf, "--rows", str(rows), "--leg", leg] + (["--root", root] if root else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.timeout)
        if p.returncode != 0:
            say("FAILED (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr.decode()[-2000:]))
            raise SystemExit(1)
        return json.loads(p.stdout.decode().strip().splitlines()[-1])

    sides = ([("parent", 0, args.parent)] if args.parent else []) + [("off", 0, None), ("wide", 1, None)]
    queries = [q for q in args.queries.split(",") if q] if args.repeats > 0 else []      # (--repeats 0: the --wrap-rows part alone)
    got = {}
    try:
        if args.sharded:
            sharded_main(args, say, spawn)
            return 0
        for rep in range(args.repeats):                        # alternating: every side once per round
            for query in queries:
                for side, mode, root in sides:
                    r = spawn(query, mode, root, args.rows)
                    if "error_code" in r:
                        say("FAILED: %s %s: [%d] %s" % (query, side, r["error_code"], r["message"]))
                        raise SystemExit(1)
                    got.setdefault((query, side), []).append(r)
                    say("round %d %s %-6s scan %s us  wall %s us  %s" % (rep, query, side, spread(r["scan_us"]), spread(r["wall_us"]), r["kernel"]))
        say()
        base = "parent" if args.parent else "off"
        for query in queries:
            say("%s at %d rows, %d processes per side, %d timed queries each: median over processes of the process medians (min .. max), microseconds" %
                (query, got[(query, "off")][0]["rows"], args.repeats, args.steps))
            med = {}
            for side, _, _ in sides:
                rs = got[(query, side)]
                scan = [statistics.median(r["scan_us"]) for r in rs]
                wall = [statistics.median(r["wall_us"]) for r in rs]
                med[side] = (statistics.median(scan), statistics.median(wall))
                say("  %-6s kernel %s   wall %s   bytes moved %s   %s" % (side, spread(scan), spread(wall), sorted(set(r["bytes_moved"] for r in rs)), rs[-1]["kernel"]))
            for side, _, _ in sides:
                if side != base:
                    say("  %s / %s: kernel %.3f  wall %.3f" % (side, base, med[side][0] / med[base][0], med[side][1] / med[base][1]))
            moved = set(r["bytes_moved"] for side, _, _ in sides for r in got[(query, side)])
            # (the tuner of every process picks its own form, and near-ties fall either way: another form moves other bytes)
            say("  bytes moved equal on every side: %s%s" % (len(moved) == 1, "" if len(moved) == 1 else " -- by kernel: %s" % sorted(
                set((r["kernel"][0].split("FusedScan_")[-1], r["bytes_moved"]) for side, _, _ in sides for r in got[(query, side)]))))
            wide, off = got[(query, "wide")][-1]["results"], got[(query, "off")][-1]["results"]
            same_low = all([(x & ((1 << 64) - 1)) for x in wide[k]] == [(x & ((1 << 64) - 1)) for x in off[k]] for k in off)
            say("  low words of mode 1 == the switch-off results: %s" % same_low)
            if query == "q1":
                top = max(wide["sum_charge"])
                say("  largest sum_charge: %d = %.4f of INT64_MAX (exact, mode 1)" % (top, top / I64_MAX))
            say("  wide note: %s" % got[(query, "wide")][-1]["wide_note"])
            say()
        if args.wrap_rows:
            r2 = spawn("q1", 2, None, args.wrap_rows)
            say("Q1 at %d rows, mode 2 (checked): %s" % (args.wrap_rows, ("[%d] %s" % (r2["error_code"], r2["message"])) if "error_code" in r2 else "NO ERROR: %s" % r2["results"].get("sum_charge")))
            r1 = spawn("q1", 1, None, args.wrap_rows)
            if "error_code" in r1:
                say("Q1 at %d rows, mode 1: FAILED [%d] %s" % (args.wrap_rows, r1["error_code"], r1["message"]))
                raise SystemExit(1)
            say("Q1 at %d rows, mode 1 (wide): sum_charge = %s; as fractions of INT64_MAX: %s" %
                (args.wrap_rows, r1["results"]["sum_charge"], ["%.4f" % (x / I64_MAX) for x in r1["results"]["sum_charge"]]))
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
