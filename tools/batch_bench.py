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
image widths per batch.  No CPU check: every answer of (b) must equal (a)'s, and (a)'s kernels are checked by the suite."""
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import mplan2vdl_amd as m
from mplan2vdl_amd import datagen

PEAK = 8.0e12
args = sys.argv[1:]


def opt(name, default):
    return args[args.index(name) + 1] if name in args else default


rows = int(opt("--rows", datagen.LINEITEM_ROWS["sf100"]))
widths = [int(x) for x in str(opt("--k", "1,2,4,8")).split(",")]
repeats = int(opt("--repeats", 9))
legs = opt("--legs", "ab")
query = opt("--query", "q6")
COLUMNS = datagen.Q1_COLUMNS if query == "q1" else datagen.Q6_COLUMNS
if query == "q1" and "--k" not in args:
    widths = [2, 3, 4]
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


torch.cuda.set_device(0)
e = m.Engine(0)
e.use_torch_stream()
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
def answer(results):
    return str(sorted(results.items())) if query == "q1" else next(iter(next(iter(results.values())).values()))


answers = [answer(p.run()["results"]) for p in plans]
say("first runs of the %d plans (tuning, compiles): %.1f s" % (kmax, time.perf_counter() - t0))
say("leg (a) kernel of plan 0: %s" % re.findall(r"-> ([^;]*);", plans[0].jit_note())[-1:])
assert len({str(a) for a in answers}) == kmax, answers


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
    if k > 1:
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

if "--no-verify" not in args and query != "q1":
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
