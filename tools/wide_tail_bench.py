#!/usr/bin/env python3
"""What wide sums cost in the GROUP BY tail (DESIGN.md section 5.17 "The tail"): TPC-H Q3 over the catalog datagen.register_q3_columns
builds in place (k_group_fold), and two micro cases of tools/op_roofline.py over the generator's lineitem with fusion off -- `tail`, its
group tail (a dense-domain Partition of 32 buckets, two Scatters, one FoldSum over the runs: k_seg_fold), and `global`, its statements
17-20 (one single-run FoldSum over a filtered vector: k_fold_global) -- with the switch off and in mode 1 with the tail switch, and, with
--parent DIR, against a build of the parent commit, off and in mode 1 as well (DIR holds that commit's mplan2vdl_amd package with its
libvdl.so built): this tree's off is held against the parent's off, its wide against the parent's wide.  Taken as ALTERNATING
FRESH PROCESSES, `--repeats` per side: every process builds its columns, warms up, times `--steps` queries on the host (profiling off:
no synchronisation between statements), and then runs three times more with per-statement events for the time of the fold statements
(FoldSum / Min / Max / Count / Choose: the folds of one GROUP BY share a launch, which is timed under the first of them).
Reported per case and side: the median over the processes of each process's median wall time per query and of the fold statements' time, with
min .. max, and the ratios; for Q3 in mode 1 the largest revenue as a fraction of INT64_MAX.  A child that fails ends the whole
measurement: nothing more is started on the device.

    python tools/wide_tail_bench.py --sf sf10 --repeats 3 --steps 10 --parent /path/to/parent/tree --out profiles/r22/wide_tail_bench.txt
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
Q3_ORDERS = {"sf0.01": 15000, "sf1": 1500000, "sf10": 15000000, "sf100": 150000000}      # lineitem = 4 x orders, customer = orders / 10
TAIL = "\n".join(["1,Load,lineitem.l_quantity", "2,Project,val,Id 1,l_quantity", "3,Load,lineitem.l_extendedprice", "4,Project,val,Id 3,l_extendedprice",
                  "21,RangeV,val,31,Id 4,0", "22,BitwiseAnd,val,Id 4,val,Id 21,val", "23,RangeC,val,0,32,1", "24,Partition,val,Id 22,val,Id 23,val",
                  "25,RangeV,val,0,Id 22,1", "26,Scatter,Id 22,Id 25,val,Id 24,val", "27,Scatter,Id 2,Id 25,val,Id 24,val",
                  "28,FoldSum,val,Id 26,val,Id 27,val", "29,Project,s,Id 28,val", "30,MaterializeCompact,Id 29"]) + "\n"
GLOBAL = "\n".join(["3,Load,lineitem.l_extendedprice", "4,Project,val,Id 3,l_extendedprice", "5,Load,lineitem.l_discount", "6,Project,val,Id 5,l_discount",
                    "12,RangeV,val,5,Id 6,0", "13,Greater,val,Id 6,val,Id 12,val", "14,RangeV,val,0,Id 13,1", "15,FoldSelect,val,Id 14,val,Id 13,val",
                    "17,Gather,Id 4,Id 15,val", "18,RangeV,val,0,Id 17,0", "19,FoldSum,val,Id 18,val,Id 17,val", "20,Project,s,Id 19,val",
                    "21,MaterializeCompact,Id 20"]) + "\n"
MICRO = {"tail": (TAIL, ("lineitem.l_quantity", "lineitem.l_extendedprice")), "global": (GLOBAL, ("lineitem.l_extendedprice", "lineitem.l_discount"))}


def child(args):
    root = os.path.abspath(args.root or ROOT)
    sys.path.insert(0, root)
    import mplan2vdl_amd as m
    from mplan2vdl_amd import datagen

    eng = m.Engine(device=0)
    if args.case == "q3":
        rows = 4 * Q3_ORDERS[args.sf]
        keep = datagen.register_q3_columns(eng, Q3_ORDERS[args.sf])
        plan = eng.parse(open(os.path.join(ROOT, "tests", "golden", "q3.vdl")).read())
        plan.set_device_outputs(True)                          # the result rows stay in HBM, as bench.py leaves them
    else:
        rows = args.rows or datagen.LINEITEM_ROWS[args.sf]
        keep = None
        text, columns = MICRO[args.case]
        for name in columns:
            eng.generate(datagen.LINEITEM[name], 0, rows)
        plan = eng.parse(text)
        plan.set_fusion(False)
    if args.mode:
        plan.set_wide_sums(args.mode, tail=True)
    out = {"case": args.case, "mode": args.mode, "rows": rows, "root": root}
    try:
        plan.execute()
    except m.VdlError as exc:
        out.update({"error_code": exc.code, "message": str(exc)})
        print(json.dumps(out))
        return 0
    for _ in range(args.warmup):
        plan.execute()
    wall = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        plan.execute()
        wall.append((time.perf_counter() - t0) * 1e6)
    plan.set_profiling(True)
    folds = []
    for _ in range(3):
        plan.execute()
        # (every fold of one GROUP BY runs in the launch of the first of them: the time of all Fold statements, not of the FoldSums alone)
        folds.append(sum(v for k, v in plan.collect()["timings"].items() if "Statement" in k and "_Fold" in k and "_FoldSelect" not in k))
    plan.set_profiling(False)
    top = None
    if args.case == "q3" and args.mode:
        plan.set_device_outputs(False)
        res = plan.run()["results"]
        rev = next(v for f in res.values() for k, v in f.items() if k == ".revenue")
        top = max(int(x) for x in rev)
    out.update({"wall_us": wall, "fold_us": folds, "wide_note": plan.wide_note() if args.mode else "", "largest_revenue": top})
    print(json.dumps(out))
    del keep
    eng.close()
    return 0


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--case", default="q3")
    ap.add_argument("--cases", default="q3,tail,global")
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--root", default=None)
    ap.add_argument("--sf", default="sf10")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a tree of the parent commit, built: two more sides, off and wide")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def spawn(case, mode, root):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--case", case, "--mode", str(mode), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--sf", args.sf, "--rows", str(args.rows)] + (["--root", root] if root else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.timeout)
        if p.returncode != 0:
            say("FAILED (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr.decode()[-2000:]))
            raise SystemExit(1)
        return json.loads(p.stdout.decode().strip().splitlines()[-1])

    sides = ([("parent", 0, args.parent), ("parent wide", 1, args.parent)] if args.parent else []) + [("off", 0, None), ("wide", 1, None)]
    pairs = [("off", "parent"), ("wide", "parent wide")] if args.parent else []      # this tree's side, the parent's side it is held against
    cases = [c for c in args.cases.split(",") if c]
    got = {}
    try:
        for rep in range(args.repeats):                        # alternating: every side once per round
            for case in cases:
                for side, mode, root in sides:
                    r = spawn(case, mode, root)
                    if "error_code" in r:
                        say("FAILED: %s %s: [%d] %s" % (case, side, r["error_code"], r["message"]))
                        raise SystemExit(1)
                    got.setdefault((case, side), []).append(r)
                    say("round %d %-6s %-11s wall %s us  fold statements %s us" % (rep, case, side, spread(r["wall_us"]), spread(r["fold_us"])))
        say()
        base = "parent" if args.parent else "off"
        for case in cases:
            say("%s at %d rows, %d processes per side, %d timed queries each: median over processes of the process medians (min .. max), microseconds" %
                (case, got[(case, "off")][0]["rows"], args.repeats, args.steps))
            med, width = {}, {}
            for side, _, _ in sides:
                rs = got[(case, side)]
                wall = [statistics.median(r["wall_us"]) for r in rs]
                fold = [statistics.median(r["fold_us"]) for r in rs]
                med[side], width[side] = (statistics.median(wall), statistics.median(fold)), (max(wall) - min(wall), max(fold) - min(fold))
                say("  %-11s wall %s   fold statements %s" % (side, spread(wall), spread(fold)))
            for side, _, _ in sides:
                if side != base:
                    say("  %s / %s: wall %.3f  fold statements %.3f" % (side, base, med[side][0] / med[base][0], med[side][1] / max(med[base][1], 1e-9)))
            for mine, theirs in pairs:                         # the margin: the larger of the two sides' own spread over the repeats
                for what, k in (("wall", 0), ("fold statements", 1)):
                    d = med[mine][k] - med[theirs][k]
                    say("  %s - %s, %s: %+.1f us; spread of the repeats: %s %.1f us, %s %.1f us -> %s" %
                        (mine, theirs, what, d, theirs, width[theirs][k], mine, width[mine][k],
                         "within the spread" if abs(d) <= max(width[theirs][k], width[mine][k]) else "OUTSIDE the spread"))
            top = got[(case, "wide")][-1].get("largest_revenue")
            if top is not None:
                say("  largest revenue: %d = %.3e of INT64_MAX (exact, mode 1)" % (top, top / I64_MAX))
            say("  wide note: %s" % got[(case, "wide")][-1]["wide_note"])
            say()
    finally:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
