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
    if args.mode:
        plan.set_wide_sums(args.mode)                          # (never called on the parent's package: it has no such switch)
    out = {"query": args.query, "mode": args.mode, "rows": rows, "root": root}
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
    args = ap.parse_args()
    if args.child:
        return child(args)

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def spawn(query, mode, root, rows):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--query", query, "--mode", str(mode), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--sf", args.sf, "--rows", str(rows)] + (["--root", root] if root else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.timeout)
        if p.returncode != 0:
            say("FAILED (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr.decode()[-2000:]))
            raise SystemExit(1)
        return json.loads(p.stdout.decode().strip().splitlines()[-1])

    sides = ([("parent", 0, args.parent)] if args.parent else []) + [("off", 0, None), ("wide", 1, None)]
    queries = [q for q in args.queries.split(",") if q] if args.repeats > 0 else []      # (--repeats 0: the --wrap-rows part alone)
    got = {}
    try:
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
