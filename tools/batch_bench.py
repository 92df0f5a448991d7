#!/usr/bin/env python3
"""What a batched run is worth on TPC-H Q6: K literal sets answered one plan after another, or by one pass over the columns.

    python tools/batch_bench.py [--rows N] [--k 1,2,4,8] [--repeats R] [--legs ab|a] [--no-verify] [--out FILE]

Generated lineitem columns with their images (default: SF100, 600 M rows), K = 1, 2, 4, 8 literal sets -- the year, the discount
and the quantity limit shifted inside the columns' domains, every range keeping its shape.  Two legs, alternating in one process:
  (a) K tuned plans run one after another with run()            -- the path of a caller without vdl_run_batch
  (b) the same K plans through Engine.run_batch                 -- one scan per batch
Wall time around each leg with the device idle before and after; medians of R (default 9) repeats and their spread (min, max).
Every answer of (b) must equal (a)'s, and (unless --no-verify) the widest K's answers are computed again on the CPU from the
downloaded columns.  For (b) the file also gives the bytes the batch kernel reads -- the eager form reads every column it binds,
n x sum of widths; the packed form its packed images -- the form and row pairs the tuner chose, and the fraction of the 8 TB/s peak
the batch kernel's own time (timeInMicrosecondsForBatchedScan) gives.  --legs a runs leg (a) alone (a tree without run_batch).

    python tools/batch_bench.py --query q1 [--k 2,3,4] ...

Grouped batches (Engine.set_batch_grouped) on TPC-H Q1: always EIGHT literal sets that shift the ship-date cutoff; K is the batch
WIDTH, pinned by VDL_BATCH_WIDTH (8 sets at K = 4: two batches; at K = 3: 3 + 3 + 2; at K = 2: four), which also fixes the table
replicas by the LDS rule (K = 4: R = 2, K = 3: R = 4, K = 2: R = 8).  Leg (a) is the eight tuned run()s, leg (b) run_batch of the
eight; per-query figures divide by eight.  The batch kernels' time is the sum over the call's batches, the bytes n x the sum of the
image widths per batch.  No CPU check: every answer of (b) must equal (a)'s, and (a)'s kernels are checked by the suite.

    python tools/batch_bench.py --query q14 [--k 2,4,8] ...

Join batches (Engine.set_batch_joins) on TPC-H Q14: 600 M lineitems and 20 M parts as tools/lookup_bench.py sets them up
(datagen.register_q14_columns, part.p_type encoded), K month windows (the month shifted by 30 days per set).  Leg (a) is K tuned
run()s -- K LIKE tables over the p_type heap, K scans, up to K times the p_type lookups --, leg (b) run_batch of the K plans: the
prelude once, the fact columns once, a row looked up once if any month wants it.  Beside the walls: the scan kernels' own time of
both legs (timeInMicrosecondsForFusedScan summed over the K runs, timeInMicrosecondsForBatchedScan) and, per leg, wall minus
kernels -- the prelude (k_like), the launches and the finalisation, which the engine does not time apart.  --legs a runs on a tree
without the switch.  No CPU check: every answer of (b) must equal (a)'s, and (a)'s kernels are checked by the suite.

    python tools/batch_bench.py --sharded [--rows N] [--k 2,4,8] [--repeats 3] [--steps 30] [--parent TREE] [--out FILE]

Sharded batches (Engine.run_batch_sharded) on Q6 over one rank's shard (default 75 004 738 rows, an eighth of SF100) with a ONE-RANK
RCCL communicator, as tools/wide_bench.py --sharded: no gather is performed, so the figures cover the kernels, the copies and the hop
to the communication stream, not the interconnect.  Legs, each in fresh processes that alternate, --repeats per side:
  (a)  K x run_sharded                            (a') K pipelined run_sharded_begin / _end steps over two slots
  (b)  run_batch_sharded of the K plans           with --parent TREE (a checkout of the parent commit, built): (a) and (a') there too
A process times --steps call sequences per K and reports their median; the table gives the median over the processes and min .. max,
checks every answer against (a)'s, and says whether (b) beats (a') by more than the spread of the repeats."""
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--tree DIR: a child of --sharded imports the package, and with it the library, of another checkout -- the parent commit's build)
sys.path.insert(0, sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else ROOT)
import numpy as np
import torch

import mplan2vdl_amd as m
from mplan2vdl_amd import datagen

PEAK = 8.0e12
args = sys.argv[1:]


def opt(name, default):
    return args[args.index(name) + 1] if name in args else default


rows = int(opt("--rows", 75004738 if "--sharded" in args else datagen.LINEITEM_ROWS["sf100"]))      # (--sharded: an eighth of SF100, one rank's shard of an 8-rank job)
widths = [int(x) for x in str(opt("--k", "1,2,4,8")).split(",")]
repeats = int(opt("--repeats", 9))
legs = opt("--legs", "ab")
query = opt("--query", "q6")
COLUMNS = datagen.Q1_COLUMNS if query == "q1" else datagen.Q6_COLUMNS
if query == "q1" and "--k" not in args:
    widths = [2, 3, 4]
if query == "q14" and "--k" not in args:
    widths = [2, 4, 8]
out_path = opt("--out", None)
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def literal_set(k):
    """Q6's constants for set k: the year's two ends, the discount's centre, the quantity's limit"""
    return {728294: 728294 + 90 * k, 728659: 728659 + 90 * k, 6: 2 + k % 7, 24: 24 + k}


def q6_text(k):
    text = open(os.path.join(ROOT, "tests", "golden", query + ".vdl")).read()
    mp, seen = ({729999: 729999 - 30 * k} if k else {}) if query == "q1" else literal_set(k), set()      # (Q1: the cutoff, 30 days earlier per set)
    if query == "q14":
        mp = {728902: 728902 + 30 * k, 728932: 728932 + 30 * k} if k else {}                               # (Q14: the month window)

    def sub(mo):
        c = int(mo.group(2))
        if c not in mp:
            return mo.group(0)
        seen.add(c)
        return "%s%d%s" % (mo.group(1), mp[c], mo.group(3))

    text = re.sub(r"^(\d+,RangeV,val,)(-?\d+)(,Id \d+,0)$", sub, text, flags=re.M)
    assert seen == set(mp), sorted(set(mp) - seen)
    return text


def cpu_q6(cols, k):
    """Q6's SQL for literal set k over the downloaded columns, in pieces: [] when no row is selected"""
    mp = literal_set(k)
    ship, disc, qty, price = (torch.from_numpy(cols[c]) for c in datagen.Q6_COLUMNS)
    total, count = 0, 0
    step = 1 << 26
    for at in range(0, len(ship), step):
        s, d, q, p = ship[at:at + step], disc[at:at + step], qty[at:at + step], price[at:at + step]
        keep = (s >= mp[728294]) & (s < mp[728659]) & (d >= mp[6] - 1) & (d <= mp[6] + 1) & (q < mp[24] * 100)
        total += int((p[keep] * d[keep]).sum().item())
        count += int(keep.sum().item())
    total = (total + (1 << 63)) % (1 << 64) - (1 << 63)
    return [total] if count else []


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, got


def stats(v):
    return "median %8.3f ms   min %8.3f   max %8.3f" % (float(np.median(v)), min(v), max(v))


# ---- --sharded: K literal sets over one rank's shard, as K sharded calls or as one sharded batch ------------------------------------------
def sharded_child(leg):
    """one fresh process, one leg, every K: prints one line "RESULT <json>" {K: [ms per call sequence, ...], "answers": {K: [...]}}"""
    import json
    steps = int(opt("--steps", 30))
    torch.cuda.set_device(0)
    eng = m.Engine(0)
    for name in datagen.Q6_COLUMNS:
        eng.generate(datagen.LINEITEM[name], 0, rows)
    eng.comm_init_rccl(0, 1, eng.comm_unique_id())             # one rank: no gather; the kernels, the copies and the stream hop are all there
    kmax = max(widths)
    ps = [eng.parse(q6_text(k)) for k in range(kmax)]
    for p in ps:
        p.set_jit(True, tune=True, runtime_bounds=True)
    first = [answer(p.run_sharded()["results"]) for p in ps]   # builds, tunes
    out = {"answers": {}, "ms": {}}
    for k in widths:
        sub = ps[:k]
        if leg == "a":
            run = lambda: [answer(p.run_sharded()["results"]) for p in sub]
        elif leg == "a2":                                       # pipelined: plan j + 1 begun before plan j is collected (two slots)
            def run():
                got = []
                for j, p in enumerate(sub):
                    p.run_sharded_begin(j & 1)
                    if j:
                        got.append(answer(sub[j - 1].run_sharded_end(1 - (j & 1))["results"]))
                got.append(answer(sub[-1].run_sharded_end((len(sub) - 1) & 1)["results"]))
                return got
        else:
            run = lambda: [answer(r["results"]) for r in eng.run_batch_sharded(sub)]
        for _ in range(5):
            got = run()
        assert got == first[:k], (leg, k)
        ts = []
        for _ in range(steps):
            ms, got = once(run)
            ts.append(ms)
        assert got == first[:k], (leg, k)
        out["ms"][str(k)] = float(np.median(ts))
        out["answers"][str(k)] = [str(x) for x in got]
        if leg == "b":
            out.setdefault("notes", {})[str(k)] = sub[0].batch_note() + " | " + sub[-1].batch_sharded_note()
    print("RESULT " + json.dumps(out), flush=True)
    for p in ps:
        p.close()
    eng.close()


def sharded_main():
    """(a) K x run_sharded, (a') K pipelined begin / end steps, (b) run_batch_sharded; with --parent TREE also (a) and (a') on that tree"""
    import json
    import subprocess
    parent = opt("--parent", None)
    sides = [("a", None), ("a2", None), ("b", None)] + ([("a", parent), ("a2", parent)] if parent else [])
    label = {("a", False): "(a)  K x run_sharded", ("a2", False): "(a') K pipelined begin/end steps", ("b", False): "(b)  run_batch_sharded",
             ("a", True): "parent (a)", ("a2", True): "parent (a')"}
    say("Q6 over %d generated rows with images (one rank's shard), a ONE-RANK RCCL communicator: no gather is performed -- the figures cover" % rows)
    say("the kernels, the copies and the hop to the communication stream, not the interconnect.  K tuned plans; every figure the median of %s"
        % opt("--steps", 30))
    say("timed call sequences in a fresh process; %d processes per side, alternating; median over them and min .. max" % repeats)
    got = {s: [] for s in sides}
    for _ in range(repeats):
        for side in sides:
            leg, tree = side
            cmd = [sys.executable, os.path.abspath(__file__), "--sharded-child", leg, "--rows", str(rows), "--k", ",".join(map(str, widths)), "--steps", str(opt("--steps", 30))]
            if tree:
                cmd += ["--tree", tree]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                say("side %s failed (exit %d): %s" % (side, r.returncode, r.stderr[-1500:]))
                sys.exit(1)
            got[side].append(json.loads(line[-1][7:]))
            print("  ... %s%s: %s" % (leg, " (parent)" if tree else "", got[side][-1]["ms"]), flush=True)
    ok = True
    for k in widths:
        say()
        say("K = %d" % k)
        med, span = {}, {}
        for side in sides:
            v = [g["ms"][str(k)] for g in got[side]]
            med[side], span[side] = float(np.median(v)), max(v) - min(v)
            say("  %-34s median %8.3f ms   min %8.3f   max %8.3f   per query %7.3f ms" % (label[(side[0], side[1] is not None)], med[side], min(v), max(v), med[side] / k))
        same = all(g["answers"][str(k)] == got[("a", None)][0]["answers"][str(k)] for s in sides for g in got[s])
        ok = ok and same
        say("  every answer of every side equals (a)'s: %s" % same)
        gain, spread = med[("a2", None)] - med[("b", None)], max(span[("a2", None)], span[("b", None)])
        say("  (a') - (b) = %+.3f ms; the wider spread of the two sides' repeats is %.3f ms: (b) %s (a')" %
            (gain, spread, "beats" if gain > spread else "does not beat by more than the spread of the repeats" if gain > 0 else "is slower than"))
        say("  (a) - (b) = %+.3f ms" % (med[("a", None)] - med[("b", None)]))
        if parent:
            for leg in ("a", "a2"):
                d = med[(leg, None)] - med[(leg, parent)]
                say("  %s, this tree - parent: %+.3f ms (spreads %.3f / %.3f)" % (label[(leg, False)].strip(), d, span[(leg, None)], span[(leg, parent)]))
        say("  notes of (b): %s" % got[("b", None)][0]["notes"][str(k)])
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


def answer(results):
    return str(sorted(results.items())) if query in ("q1", "q14") else next(iter(next(iter(results.values())).values()))


if "--sharded-child" in args:
    sharded_child(opt("--sharded-child", "a"))
    sys.exit(0)
if "--sharded" in args:
    if "--k" not in args:
        widths = [2, 4, 8]
    if "--repeats" not in args:
        repeats = 3
    sharded_main()

torch.cuda.set_device(0)
e = m.Engine(0)
e.use_torch_stream()
if query == "q14":
    e.set_lookup_images(True)                                             # (p_type is looked up through its 2-byte image, as lookup_bench's leg "on")
    keep = datagen.register_q14_columns(e, rows, lookup_images=True)      # (600 M lineitems: 20 M parts)
    if "b" in legs:
        e.set_batch_joins(True)
else:
    for name in COLUMNS:
        e.generate(datagen.LINEITEM[name], 0, rows)
if query == "q1" and "b" in legs:
    e.set_batch_grouped(True)
say("%s, %d rows of generated lineitem with images, %d alternating repeats, legs %s" % (query.upper(), rows, repeats, legs))
kmax = 8 if query == "q1" else max(widths)
plans = [e.parse(q6_text(k)) for k in range(kmax)]
for p in plans:
    p.set_jit(True, tune=True, runtime_bounds=True)      # (run-time bounds: the K plans of leg (a) share their code, as since round 11)
t0 = time.perf_counter()
answers = [answer(p.run()["results"]) for p in plans]
say("first runs of the %d plans (tuning, compiles): %.1f s" % (kmax, time.perf_counter() - t0))
say("leg (a) kernel of plan 0: %s" % re.findall(r"-> ([^;]*);", plans[0].jit_note())[-1:])
assert query == "q14" or len({str(a) for a in answers}) == kmax, answers      # (Q14's answer is a percentage: months may agree)


def leg_a(k):
    return [answer(p.run()["results"]) for p in plans[:k]]


def leg_b(k):
    return [answer(r["results"]) for r in e.run_batch(plans[:k])]


for k in widths:
    say()
    say("K = %d" % k)
    width = k
    if query == "q1":                                     # K is the batch width; the plans are always the eight
        os.environ["VDL_BATCH_WIDTH"] = str(width)
        k = kmax
    if "b" in legs and k > 1:
        t0 = time.perf_counter()
        assert leg_b(k) == answers[:k], "run_batch differs from run()"
        say("  first batch (tuning, compiles): %.1f s; %s" % (time.perf_counter() - t0, plans[0].batch_note()))
        if query == "q1":
            say("  notes: %s" % "; ".join(p.batch_note().split(",")[0] for p in plans[:k]))
    elif "b" in legs:
        leg_b(k)
    leg_a(k)
    ta, tb = [], []
    for _ in range(repeats):                              # alternating: a drift of the machine falls on both legs alike
        ms, got = once(lambda: leg_a(k))
        assert got == answers[:k]
        ta.append(ms)
        if "b" in legs:
            ms, got = once(lambda: leg_b(k))
            assert got == answers[:k]
            tb.append(ms)
    say("  (a) %d x run()     %s   per query %7.3f ms" % (k, stats(ta), float(np.median(ta)) / k))
    if "b" not in legs:
        continue
    say("  (b) run_batch      %s   per query %7.3f ms" % (stats(tb), float(np.median(tb)) / k))
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    say("  (a) / (b) = %.2f; medians differ by %.3f ms, the widest spread of repeats is %.3f ms" %
        (float(np.median(ta)) / float(np.median(tb)), float(np.median(ta)) - float(np.median(tb)), spread))
    if k > 1 and query == "q14":
        # the kernels' own time of both legs; what is left of the wall is the prelude (k_like over the heap), the launches, the finalisation
        for p in plans[:k]:
            p.set_profiling(True)
        ka, kb, wa, wb, pb = [], [], [], [], []
        for _ in range(repeats):
            ms, rs = once(lambda: [p.run() for p in plans[:k]])
            wa.append(ms)
            ka.append(sum(v for r in rs for key, v in r["timings"].items() if "FusedScan" in key) / 1e3)
            ms, rs = once(lambda: e.run_batch(plans[:k]))
            wb.append(ms)
            kb.append(next(v for key, v in rs[0]["timings"].items() if "BatchedScan" in key) / 1e3)
            pb.append(sum(v for r in rs for key, v in r["timings"].items() if "BatchedPrelude" in key) / 1e3)
        for p in plans[:k]:
            p.set_profiling(False)
        say("  batch kernel: %s" % plans[0].batch_note().split(", ", 1)[1])
        say("  under profiling (a): %d scan kernels %s; wall - kernels: median %.3f ms per call, %.3f per query" %
            (k, stats(ka), float(np.median(np.array(wa) - np.array(ka))), float(np.median(np.array(wa) - np.array(ka))) / k))
        say("  under profiling (b): batch kernel    %s; wall - kernel:  median %.3f ms per call" % (stats(kb), float(np.median(np.array(wb) - np.array(kb)))))
        say("  (b) prelude, once per call (k_like over the p_type heap; timeInMicrosecondsForBatchedPrelude): %s" % stats(pb))
        say("  (a run() alone launches the same k_like over the same heap once per plan: %d times per call of leg (a), not timed apart)" % k)
    elif k > 1:
        note = plans[0].batch_note()
        name = note.split(", ", 1)[1]
        packed = ",packed," in name
        if packed:
            nbytes = sum((rows + 2047) // 2048 * 2048 * e.packed_info(c)[0] // 8 for c in datagen.Q6_COLUMNS)
        else:
            nbytes = sum(rows * (e.image_info(c)[0] or np.dtype(datagen.LINEITEM[c].dtype).itemsize) for c in COLUMNS)
        heads = [i for i, p in enumerate(plans[:k]) if ": slot 0 of " in p.batch_note()]      # one plan per batch of the call
        nbytes *= len(heads)
        for p in plans[:k]:
            p.set_profiling(True)
        us = []
        for _ in range(repeats):
            r = e.run_batch(plans[:k])
            us.append(sum(next(v for key, v in r[i]["timings"].items() if "BatchedScan" in key) for i in heads))
        for p in plans[:k]:
            p.set_profiling(False)
        kern = float(np.median(us)) * 1e-6
        say("  batch kernel: %s (%s form, u = %s)" % (name, "packed" if packed else "eager", re.search(r"<\d+,(\d+),", name).group(1)))
        say("  batches in the call: %d; batched plans: %d of %d" % (len(heads), sum(p.batch_note().startswith("batch") for p in plans[:k]), k))
        say("  batch kernel time: median %d us (min %d, max %d); it reads %d bytes: %.2f TB/s = %.3f of the 8 TB/s peak; per query %.1f us" %
            (int(np.median(us)), min(us), max(us), nbytes, nbytes / kern / 1e12, nbytes / kern / PEAK, np.median(us) / k))

if "--no-verify" not in args and query not in ("q1", "q14"):
    t0 = time.perf_counter()
    cols = {c: e.download(c) for c in datagen.Q6_COLUMNS}
    ok = all(cpu_q6(cols, k) == answers[k] for k in range(kmax))
    say()
    say("CPU check of the %d literal sets over the downloaded columns: %s (%.0f s)" % (kmax, "every answer equal" if ok else "MISMATCH", time.perf_counter() - t0))
    if not ok:
        sys.exit(1)
for p in plans:
    p.close()
e.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
