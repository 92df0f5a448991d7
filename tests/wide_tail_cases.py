"""Programs, data and Python-integer references of the tests of wide sums in the GROUP BY tail and the per-operator folds
(tests/test_wide_tail.py, tests/test_wide_tail_cpu.py; DESIGN.md section 5.17 "The tail").

The reference for every SUM is Python integer arithmetic over the uploaded columns, as in tests/wide_cases.py: the per-entry terms are
computed in wrapped int64, as numpy does, and summed as Python ints per group; an engine result (lo, hi) stands for
(hi << 64) | (lo & (2^64 - 1))."""
import numpy as np

from helpers import prog
from wide_cases import BIG, I64_MAX, I64_MIN, MASK, NEG

FOLDS = ["FoldSum", "FoldMin", "FoldMax", "FoldCount", "FoldChoose"]
# the split's own edges (a term is H * 2^32 + L) and the ends of int64
EDGE_VALUES = [BIG, NEG, I64_MAX, I64_MIN, -1, 0, (1 << 32) - 1, 1 << 32, -(1 << 32), -(1 << 32) - 1, 1 << 31, -(1 << 31) - 1]
SIZES = [1, 8, 9, 64, 65, 512, 513, 2048, 2049, 4096, 4097, 8193, 100003]


def group_program(filtered, domain=1 << 40, folds=FOLDS):
    """The program of tests/test_group_tail.py restated: key, v, w, v * (w - 1), ones and row ids scattered into key order, every fold kind
    over them.  Returns (text, [(tmp, fold, operand)]): operand one of "v", "w", "vw", "ones", "rowid", "key"."""
    L = ["1,Load,t.k", "2,Project,val,Id 1,k", "3,Load,t.v", "4,Project,val,Id 3,v", "5,Load,t.w", "6,Project,val,Id 5,w", "7,Load,t.f", "8,Project,val,Id 7,f"]
    nid = [8]

    def emit(body):
        nid[0] += 1
        L.append("%d,%s" % (nid[0], body))
        return nid[0]

    k, v, w = 2, 4, 6
    if filtered:
        zero = emit("RangeV,val,0,Id 8,0")
        pred = emit("Greater,val,Id 8,val,Id %d,val" % zero)
        sel = emit("FoldSelect,val,Id %d,val,Id %d,val" % (emit("RangeV,val,0,Id %d,1" % pred), pred))
        k, v, w = (emit("Gather,Id %d,Id %d,val" % (x, sel)) for x in (k, v, w))
    piv = emit("RangeC,val,0,%d,1" % domain)
    part = emit("Partition,val,Id %d,val,Id %d,val" % (k, piv))
    sk = emit("Scatter,Id %d,Id %d,val,Id %d,val" % (k, emit("RangeV,val,0,Id %d,1" % k), part))
    ones = emit("RangeV,val,1,Id %d,0" % v)
    rowid = emit("RangeV,val,0,Id %d,1" % v)
    vw = emit("Multiply,val,Id %d,val,Id %d,val" % (v, emit("Subtract,val,Id %d,val,Id %d,val" % (w, ones))))
    outs = []
    for data, name in ((v, "v"), (w, "w"), (vw, "vw"), (ones, "ones"), (rowid, "rowid")):
        sd = emit("Scatter,Id %d,Id %d,val,Id %d,val" % (data, emit("RangeV,val,0,Id %d,1" % data), part))
        for f in (folds if name in ("v", "vw") else [x for x in ("FoldSum", "FoldChoose") if x in folds]):
            outs.append((emit("%s,val,Id %d,val,Id %d,val" % (f, sk, sd)), f, name))
    outs.append((emit("FoldChoose,val,Id %d,val,Id %d,val" % (sk, sk)), "FoldChoose", "key"))
    meta = []
    for o, f, name in outs:
        meta.append(("tmp%d" % emit("MaterializeCompact,Id %d" % o), f, name))
    return prog(*L), meta


def keys_of(n, seed, shape):
    r = np.random.default_rng(seed)
    if shape == "short":            # runs of 1 .. 7
        k = np.cumsum(r.integers(0, 2, n) | (r.integers(0, 7, n) == 0))
    elif shape == "mixed":          # runs of 1 up to 9000: across waves, blocks and tiles
        lens, total = [], 0
        while total < n:
            ln = int(r.choice([1, 1, 2, 3, 70, 600, 5000, 9000]))
            lens.append(ln); total += ln
        k = np.repeat(np.arange(len(lens)) * 3, lens)[:n]
    else:                           # one run
        k = np.zeros(n, np.int64)
    return k.astype(np.int64) + 5


def group_columns(n, seed, shape, values=EDGE_VALUES):
    r = np.random.default_rng(seed + 1000003)
    return {"t.k": keys_of(n, seed, shape), "t.v": np.array(values, np.int64)[r.integers(0, len(values), n)], "t.w": r.integers(-3, 50, n).astype(np.int32),
            "t.f": (r.integers(0, 10, n) < 7).astype(np.int64)}


def exact_group_sums(cols, filtered, meta):
    """{tmp: [exact sum per group, in key order]} for the FoldSum outputs of group_program over `cols`"""
    keep = cols["t.f"] > 0 if filtered else np.ones(len(cols["t.k"]), bool)
    k, v, w, rowid = cols["t.k"][keep], cols["t.v"][keep].astype(np.int64), cols["t.w"][keep].astype(np.int64), np.flatnonzero(keep).astype(np.int64)
    order = np.argsort(k, kind="stable")                       # the Partition: stable by key (every key lies inside the pivots)
    k, v, w, rowid = k[order], v[order], w[order], rowid[order]      # (a row id is the slot of the unfiltered vector)
    if len(k) == 0:
        return {tmp: [] for tmp, f, _ in meta if f == "FoldSum"}
    heads = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    with np.errstate(over="ignore"):
        terms = {"v": v, "w": w, "vw": v * (w - 1), "ones": np.ones(len(k), np.int64), "rowid": rowid}    # wrapped, as the engine's
    return {tmp: [int(x) for x in np.add.reduceat(terms[name].astype(object), heads)] for tmp, f, name in meta if f == "FoldSum"}


def low(x):
    """an exact value reduced to its low 64 bits, signed: what the switch-off engine delivers"""
    x &= MASK
    return x - (1 << 64) if x >> 63 else x


def exact(lo, hi):
    return (int(hi) << 64) | (int(lo) & MASK)


# ---- consumed sums ------------------------------------------------------------------------------------------------------------------
# Q18's shape: sum(v) per key in the tail, `sum > 300` filters the groups, the surviving keys and sums come out
HAVING = prog("1,Load,t.k", "2,Project,val,Id 1,k", "3,Load,t.v", "4,Project,val,Id 3,v",
              "5,RangeC,val,0,1099511627776,1", "6,Partition,val,Id 2,val,Id 5,val", "7,RangeV,val,0,Id 2,1",
              "8,Scatter,Id 2,Id 7,val,Id 6,val", "9,Scatter,Id 4,Id 7,val,Id 6,val",
              "10,FoldSum,val,Id 8,val,Id 9,val", "11,FoldChoose,val,Id 8,val,Id 8,val",
              "12,RangeV,val,300,Id 10,0", "13,Greater,val,Id 10,val,Id 12,val",
              "14,RangeV,val,0,Id 13,1", "15,FoldSelect,val,Id 14,val,Id 13,val",
              "16,Gather,Id 11,Id 15,val", "17,Project,key,Id 16,val", "18,MaterializeCompact,Id 17",
              "19,Gather,Id 10,Id 15,val", "20,Project,total,Id 19,val", "21,MaterializeCompact,Id 20")
HAVING_CONSUMER = 13                                           # the Greater reads the sums
# Q11's shape under fusion off: a global sum, times a constant, delivered
SCALED = prog("1,Load,t.v", "2,Project,val,Id 1,v", "3,RangeV,val,0,Id 2,0", "4,FoldSum,val,Id 3,val,Id 2,val",
              "5,RangeV,val,3,Id 4,0", "6,Multiply,val,Id 4,val,Id 5,val", "7,Project,scaled,Id 6,val", "8,MaterializeCompact,Id 7")
SCALED_CONSUMER = 6


def having_want(cols):
    k, v = cols["t.k"], cols["t.v"]
    keys, sums = [], []
    for key in sorted(set(int(x) for x in k)):
        s = sum(int(x) for x in v[k == key])
        if s > 300:
            keys.append(key); sums.append(s)
    return {"key": keys, "total": sums}
