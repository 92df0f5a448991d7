"""Programs, data and Python-integer references of the wide-sums tests (tests/test_wide_sums.py, tests/test_wide_sums_cpu.py).

The reference for every value is Python integer arithmetic over the uploaded columns: the per-row terms are computed in wrapped
int64, as numpy does, and summed as Python ints; an engine result (lo, hi) stands for (hi << 64) | (lo & (2^64 - 1))."""
import os

import numpy as np

from helpers import prog

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
BIG, NEG = (1 << 62) + 7, -(1 << 62) - 5

# ---- a global scan: sum(v), sum(v * w), min(v), max(w) over the rows with f < 10 ---------------------------------------------------
_HEAD = ["1,Load,t.v", "2,Project,val,Id 1,v", "3,Load,t.w", "4,Project,val,Id 3,w", "5,Load,t.f", "6,Project,val,Id 5,f",
         "7,RangeV,val,10,Id 6,0", "8,Greater,val,Id 7,val,Id 6,val", "9,RangeV,val,0,Id 8,1", "10,FoldSelect,val,Id 9,val,Id 8,val",
         "11,Gather,Id 2,Id 10,val", "12,Gather,Id 4,Id 10,val", "13,RangeV,val,0,Id 11,0"]
GLOBAL = prog(*(_HEAD + ["14,FoldSum,val,Id 13,val,Id 11,val", "15,Project,s,Id 14,val", "16,MaterializeCompact,Id 15",
                         "17,Multiply,val,Id 11,val,Id 12,val", "18,FoldSum,val,Id 13,val,Id 17,val", "19,Project,sp,Id 18,val", "20,MaterializeCompact,Id 19",
                         "21,FoldMin,val,Id 13,val,Id 11,val", "22,Project,mn,Id 21,val", "23,MaterializeCompact,Id 22",
                         "24,FoldMax,val,Id 13,val,Id 12,val", "25,Project,mx,Id 24,val", "26,MaterializeCompact,Id 25"]))
# one SUM and nothing else: the plan the hand-tuned single-aggregate kernel serves with the switch off
SINGLE = prog(*(_HEAD[:2] + _HEAD[4:11] + ["13,RangeV,val,0,Id 11,0", "14,FoldSum,val,Id 13,val,Id 11,val", "15,Project,s,Id 14,val", "16,MaterializeCompact,Id 15"]))


def global_cols(n, v=None, w=None, f=None):
    z = np.zeros(n, np.int64)
    return {"t.v": z.copy() if v is None else np.asarray(v, np.int64), "t.w": np.ones(n, np.int64) if w is None else np.asarray(w, np.int64),
            "t.f": z.copy() if f is None else np.asarray(f, np.int64)}


def exact_sum(terms):
    return sum(int(x) for x in terms)


def global_want(cols, single=False):
    """{field: [exact value]} ([] where no row passes the filter)"""
    keep = cols["t.f"] < 10
    if not keep.any():
        return {"s": []} if single else {"s": [], "sp": [], "mn": [], "mx": []}
    v = cols["t.v"][keep]
    out = {"s": [exact_sum(v)]}
    if not single:
        w = cols["t.w"][keep]
        with np.errstate(over="ignore"):
            prod = v * w                                       # the per-row term wraps in int64, as the engine's does
        out.update({"sp": [exact_sum(prod)], "mn": [int(v.min())], "mx": [int(w.max())]})
    return out


# ---- a grouped scan: TPC-H Q1 as compiled (tests/golden/q1.vdl) with MIN and MAX beside its sums -----------------------------------------
Q1_COLUMNS = ["lineitem.l_returnflag", "lineitem.l_linestatus", "lineitem.l_quantity", "lineitem.l_extendedprice", "lineitem.l_discount", "lineitem.l_tax",
              "lineitem.l_shipdate"]
GROUPED = open(os.path.join(ROOT, "tests", "golden", "q1.vdl")).read().rstrip("\n") + "\n" + prog(
    "102,FoldMin,val,Id 35,val,Id 48,val", "103,Project,min_qty,Id 102,val", "104,MaterializeCompact,Id 103",
    "105,FoldMax,val,Id 35,val,Id 56,val", "106,Project,max_price,Id 105,val", "107,MaterializeCompact,Id 106")
FLAGS, STATUS = (65, 78, 82), (70, 79)                        # 'A' 'N' 'R', 'F' 'O': six groups


def grouped_cols(n, seed=3):
    """small Q1-shaped data, every column int64 (so that a test can plant any value anywhere); every row passes the date filter"""
    rng = np.random.default_rng(seed)
    return {"lineitem.l_returnflag": rng.choice(FLAGS, n).astype(np.int64), "lineitem.l_linestatus": rng.choice(STATUS, n).astype(np.int64),
            "lineitem.l_quantity": rng.integers(100, 5001, n, dtype=np.int64), "lineitem.l_extendedprice": rng.integers(90091, 10494951, n, dtype=np.int64),
            "lineitem.l_discount": rng.integers(0, 11, n, dtype=np.int64), "lineitem.l_tax": rng.integers(0, 9, n, dtype=np.int64),
            "lineitem.l_shipdate": rng.integers(727000, 729999, n, dtype=np.int64)}


def group_of(cols):
    rf, ls = cols["lineitem.l_returnflag"], cols["lineitem.l_linestatus"]
    return ((((rf >> 3) - 2) << 2) | ((ls >> 3) - 2)) & 31


def _div(a, b):
    """the engine's Divide on Python ints: truncation towards zero, x / 0 = 0"""
    if b == 0:
        return 0
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def grouped_want(cols):
    """{field: [exact value per non-empty group, ascending group key]}"""
    keep = cols["lineitem.l_shipdate"] <= 729999
    g = group_of(cols)
    qty, ep, disc, tax = (cols["lineitem.l_" + k] for k in ("quantity", "extendedprice", "discount", "tax"))
    with np.errstate(over="ignore"):
        dp = ep * (100 - disc)
        ch = dp * (100 + tax)
    out = {k: [] for k in ("l_returnflag__lineitem__l_returnflag", "l_linestatus__lineitem__l_linestatus", "sum_qty", "sum_base_price", "sum_disc_price",
                           "sum_charge", "avg_qty", "avg_price", "avg_disc", "count_order", "min_qty", "max_price")}
    for key in sorted(set(int(x) for x in g[keep])):
        rows = np.nonzero(keep & (g == key))[0]
        cnt = len(rows)
        sq, sb, sd = exact_sum(qty[rows]), exact_sum(ep[rows]), exact_sum(disc[rows])
        out["l_returnflag__lineitem__l_returnflag"].append(int(cols["lineitem.l_returnflag"][rows[0]]))
        out["l_linestatus__lineitem__l_linestatus"].append(int(cols["lineitem.l_linestatus"][rows[0]]))
        out["sum_qty"].append(sq); out["sum_base_price"].append(sb)
        out["sum_disc_price"].append(exact_sum(dp[rows])); out["sum_charge"].append(exact_sum(ch[rows]))
        out["avg_qty"].append(_div(sq, cnt)); out["avg_price"].append(_div(sb, cnt)); out["avg_disc"].append(_div(sd, cnt))
        out["count_order"].append(cnt)
        out["min_qty"].append(int(qty[rows].min())); out["max_price"].append(int(ep[rows].max()))
    return out


# ---- results ------------------------------------------------------------------------------------------------------------------------
def by_field(results):
    """{tmpN: {".field": values}} -> {field: values}"""
    return {name[1:]: (vals.tolist() if hasattr(vals, "tolist") else list(vals)) for fields in results.values() for name, vals in fields.items()}


def wrapped(want):
    """what the switch-off engine and the oracle deliver for exact values `want`: each reduced to its low 64 bits, signed"""
    def low(x):
        x &= MASK
        return x - (1 << 64) if x >> 63 else x
    return {k: [low(x) for x in v] for k, v in want.items()}
