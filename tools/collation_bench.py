#!/usr/bin/env python3
"""What ORDER BY on a string key costs: the collation index's build, and an ordered run of many rows over a large dictionary.

    python tools/collation_bench.py [--rows N] [--repeats R] [--host-repeats H] [--skip-host]      default: 60000000 rows, 9, 3

1. Index build for heaps of 10^3, 10^5 and 10^6 strings of 18 bytes ("Customer#%09d", 8-aligned: 24 heap bytes each): the whole
   build (timeInMicrosecondsForCollation_<heap>) and its steps, median of five builds each (the heap is uploaded anew before each).
2. `rows` rows whose codes are drawn from the 10^6-string heap, ordered by the name -- limit 100 and whole -- three ways, alternating
   in one process:
     (a) the order on the raw code, no text mark: what the device could do before (the same selection / sort kernels; the order
         step of a plan without text keys is the one it was).  The heap is written in text order, so code order IS text order here
         and all three legs must deliver the same rows; the difference (c) - (a) is the price of the translate;
     (b) the route without an index: every row to the host, decoded and sorted there (numpy, stable);
     (c) name:text.
   Wall ms per query (median, min, max), timeInMicrosecondsForOrder, and for (c) the translate launch alone
   (timeInMicrosecondsForOrderTextKeys) with its fraction of 8 TB/s on the counted bytes: 16 B per row plus 128 B for every
   distinct table line the codes touch."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import mplan2vdl_amd as m

args = sys.argv[1:]


def opt(name, default):
    return int(args[args.index(name) + 1]) if name in args else default


rows, repeats, host_repeats, skip_host = opt("--rows", 60000000), opt("--repeats", 9), opt("--host-repeats", 3), "--skip-host" in args
PEAK = 8e12
SLOT = 24

PROGRAM = "\n".join([
    "1,Load,t.f", "2,Project,val,Id 1,f", "3,RangeV,val,0,Id 2,1", "4,FoldSelect,val,Id 3,val,Id 2,val",
    "5,Load,t.name", "6,Project,val,Id 5,name", "7,Gather,Id 6,Id 4,val", "8,Project,name__t__name,Id 7,val", "9,MaterializeCompact,Id 8",
    "10,Load,t.v", "11,Project,val,Id 10,v", "12,Gather,Id 11,Id 4,val", "13,Project,v,Id 12,val", "14,MaterializeCompact,Id 13"]) + "\n"
NAME, HEAP = "name__t__name", "t.name.heap"


def heap_of(d, in_text_order):
    """d names at offsets 16 + 24 i; in text order, or shuffled"""
    ids = np.arange(d) if in_text_order else np.random.default_rng(d).permutation(d)
    text = np.char.add("Customer#", np.char.zfill(ids.astype(str), 9)).astype("S%d" % SLOT)
    return np.concatenate([np.zeros(16, np.int8), np.frombuffer(text.tobytes(), dtype=np.int8)]), 16 + SLOT * np.arange(d, dtype=np.int64)


def once(plan):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan.execute()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return "median %10.3f   min %10.3f   max %10.3f" % (float(np.median(v)), min(v), max(v))


def host(v):
    return torch.as_tensor(v, device="cuda:0").cpu().numpy() if type(v).__name__ == "DeviceValues" else np.asarray(v)


torch.cuda.set_device(0)
e = m.Engine(0)
e.use_torch_stream()

# ---- 1. the build ---------------------------------------------------------------------------------------------------------------------
print("index build, 18-byte strings at 8-aligned offsets (24 heap bytes each), shuffled; us, median of 5 builds (min .. max)")
small = {"t.f": np.ones(64, np.int8), "t.v": np.arange(64, dtype=np.int64)}
for k, v in small.items():
    e.upload(k, v)
for d in (1000, 100000, 1000000):
    heap, codes = heap_of(d, in_text_order=False)
    e.upload("t.name", codes[np.arange(64) % d])
    p = e.parse(PROGRAM)
    p.set_profiling(True)
    p.set_order([(NAME, False, HEAP)], limit=10)
    seen = {}
    for _ in range(6):                                   # the first build warms the pool
        e.upload(HEAP, heap)
        t = p.run()["timings"]
        for label, us in t.items():
            if "Collation" in label:
                seen.setdefault(label.replace("timeInMicrosecondsFor", "").replace("_" + HEAP, ""), []).append(us)
    info = e.collation_info(HEAP)
    print("  D = %7d (heap %9d bytes, table %8d bytes)  %s" % (d, len(heap), 4 * ((len(heap) + 7) // 8), info))
    for label, v in seen.items():
        v = v[1:]
        print("    %-16s %10.0f  (%.0f .. %.0f)" % (label, float(np.median(v)), min(v), max(v)))
    p.close()

# ---- 2. the ordered run -----------------------------------------------------------------------------------------------------------------
d = 1000000
heap, codes = heap_of(d, in_text_order=True)
rng = np.random.default_rng(1)
name = codes[rng.integers(0, d, size=rows)]
e.upload(HEAP, heap)
e.upload("t.name", name)
e.upload("t.v", rng.integers(0, 1 << 40, size=rows, dtype=np.int64))
e.upload("t.f", np.ones(rows, np.int8))
e.build_collation(HEAP)
lines = len(np.unique((name >> 3) * 4 // 128))
counted = 16 * rows + 128 * lines
print("ordered run: %d rows, codes drawn from %d strings; the translate's counted bytes: 16 B x rows + 128 B x %d table lines = %.1f MB" % (rows, d, lines, counted / 1e6))
names_s = np.frombuffer(heap[16:].tobytes(), dtype="S%d" % SLOT)

for limit in (100, 0):
    plans = {"a: by code": e.parse(PROGRAM), "c: by text": e.parse(PROGRAM)}
    plans["a: by code"].set_order([(NAME, False)], limit=limit)
    plans["c: by text"].set_order([(NAME, False, HEAP)], limit=limit)
    if not skip_host:
        plans["b: to the host, sorted there"] = e.parse(PROGRAM)
    for p in plans.values():
        p.set_device_outputs(limit == 0)
        p.set_profiling(True)
    if not skip_host:
        plans["b: to the host, sorted there"].set_device_outputs(False)
        plans["b: to the host, sorted there"].set_profiling(False)

    def host_leg(p):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = p.run(as_numpy=True)["results"]
        t1 = time.perf_counter()
        col = {next(iter(v))[1:]: np.asarray(next(iter(v.values()))) for v in res.values()}
        text = names_s[(col[NAME] - 16) // SLOT]
        if limit:
            try:
                head = np.argpartition(text, limit - 1)[:limit]
                bound = text[head].max()
                cand = np.nonzero(text <= bound)[0]                      # ties of the boundary string included: the position decides among them
            except TypeError:
                cand = np.arange(len(text))
            order = cand[np.argsort(text[cand], kind="stable")][:limit]
        else:
            order = np.argsort(text, kind="stable")
        out = {f: v[order] for f, v in col.items()}
        return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, out

    ms = {k: [] for k in plans}
    fetch_ms, order_us, text_us, host_out = [], {k: [] for k in plans}, [], None
    for k, p in plans.items():
        if not k.startswith("b"):
            once(p); once(p)
    for r in range(repeats):
        print("    .. repeat %d" % r, file=sys.stderr, flush=True)
        for k, p in plans.items():
            if k.startswith("b"):
                if r < host_repeats:
                    t_all, t_fetch, host_out = host_leg(p)
                    ms[k].append(t_all); fetch_ms.append(t_fetch)
                continue
            ms[k].append(once(p))
            t = p.collect(as_numpy=True)["timings"]
            order_us[k].append(t["timeInMicrosecondsForOrder"])
            if k.startswith("c"):
                text_us.append(t["timeInMicrosecondsForOrderTextKeys"])
    print("  order by name %s, %d alternating repeats (%d of the host leg); wall ms per query" % ("limit %d" % limit if limit else "(whole)", repeats, host_repeats))
    for k, v in ms.items():
        print("    (%-28s)  %s" % (k, spread(v)))
    if fetch_ms:
        print("    (b)'s run with every row to the host alone: %s ms" % spread(fetch_ms))
    for k in ("a: by code", "c: by text"):
        print("    (%s) timeInMicrosecondsForOrder %s us; note: %s" % (k[0], spread(order_us[k]), plans[k].order_note()))
    tk = float(np.median(text_us))
    print("    translate launch: %s us = %.0f GB/s on the counted bytes = %.2f of 8 TB/s" % (spread(text_us), counted / tk / 1e3, counted / (tk * 1e-6) / PEAK))
    outs = {}
    for k in ("a: by code", "c: by text"):
        outs[k] = {next(iter(v))[1:]: host(next(iter(v.values()))) for v in plans[k].collect(as_numpy=True)["results"].values()}
    same = all(np.array_equal(outs["a: by code"][f], outs["c: by text"][f]) for f in outs["c: by text"])
    if host_out is not None:
        same = same and all(np.array_equal(host_out[f], outs["c: by text"][f]) for f in host_out)
    print("    all legs deliver the same rows: %s" % same)
    if not same:
        sys.exit(1)
    for p in plans.values():
        p.close()
e.close()
