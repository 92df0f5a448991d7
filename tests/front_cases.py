"""What tests/test_front_levels.py (device) and tests/test_front_cases_cpu.py share: the two programs whose selection runs as the
one-pass fused front (csrc/vdl_mscan_body.h: project_front_body), survivor patterns that are functions of the BATCH number -- so a
missing or doubled node of the front's look-back shifts survivors visibly --, the reference in numpy and the comparison.

A batch is FRONT_BATCH tiles of T rows; the look-back is a fan-out-16 tree over batches (csrc/vdl_front_index.h): level-1 nodes are read
from 17 batches on, level-2 nodes from 257, level-3 nodes from 4097.  The programs carry the front's own vectors as outputs -- the row
ids, f.k, f.v and d.g[f.k] of the survivors in row order --: those must equal flatnonzero(mask), k[mask], v[mask], g[k[mask]] value for
value, which no displacement of a batch's survivors leaves intact (tests/test_front_cases_cpu.py shows it)."""
import re

import numpy as np

from helpers import prog
from level_cases import out
from test_step_images import T, FRONT_BATCH, FRONT_CARRY          # read from csrc/vdl_mscan_body.h

B = FRONT_BATCH * T                    # rows of a batch
FAN = 16                               # batches per node of the next level (kFrontFanBits = 4; tests/test_front_cases_cpu.py guards it)
ND = 1000                              # rows of the dimension table d
DOMAIN = 1 << 20                       # the GROUP BY key's declared domain

ROWS, K, V, G, SUM, CHOOSE, COUNT = "rows", "k", "v", "g", "sum", "choose", "count"
DIRECT = (ROWS, K, V, G)


def rows_of(batches, tiles=0, rows=0):
    """the length of a table of `batches` whole batches, `tiles` further whole tiles and `rows` further rows"""
    assert 0 <= tiles < FRONT_BATCH and 0 <= rows < T
    return batches * B + tiles * T + rows


def batches_of(n):
    return (n + B - 1) // B


# ---- the programs ------------------------------------------------------------------------------------------------------------------
def front_program(dimension_filter, extra_filters=0, extra_takes=0):
    """-> (text, {name: output node}).  Program A: rows with f.a < 7 survive; program B (dimension_filter): ... and d.g[f.k] > 5.
    The survivors' f.k, f.v and d.g[f.k] are grouped by f.k (Partition, three Scatters, FoldSum / FoldChoose / FoldCount) and are outputs
    as they leave the front, with the survivors' row ids (Id 16 .. 19).
    extra_filters: that many further int8 columns f.x0, f.x1, ... each with a range filter (100 > f.xi) ANDed into the selection --
    further deciding columns; extra_takes: that many further columns f.t0, ... gathered through the selection -- further take-side
    columns, each an output."""
    lines = ["1,Load,f.k", "2,Project,val,Id 1,k", "3,Load,f.a", "4,Project,val,Id 3,a", "5,Load,f.v", "6,Project,val,Id 5,v", "7,Load,d.g", "8,Project,val,Id 7,g",
             "9,RangeV,val,7,Id 4,0", "10,Greater,val,Id 9,val,Id 4,val"]
    sel = 10
    if dimension_filter:
        lines += ["11,Gather,Id 8,Id 2,val", "12,RangeV,val,5,Id 11,0", "13,Greater,val,Id 11,val,Id 12,val", "14,LogicalAnd,val,Id 10,val,Id 13,val"]
        sel = 14
    k = 100
    for i in range(extra_filters):
        lines += ["%d,Load,f.x%d" % (k, i), "%d,Project,val,Id %d,x%d" % (k + 1, k, i), "%d,RangeV,val,100,Id %d,0" % (k + 2, k + 1),
                  "%d,Greater,val,Id %d,val,Id %d,val" % (k + 3, k + 2, k + 1), "%d,LogicalAnd,val,Id %d,val,Id %d,val" % (k + 4, sel, k + 3)]
        sel, k = k + 4, k + 5
    takes = []
    for i in range(extra_takes):
        lines += ["%d,Load,f.t%d" % (k, i), "%d,Project,val,Id %d,t%d" % (k + 1, k, i)]
        takes.append(k + 1)
        k += 2
    s, p = (16, 20) if k == 100 else (k + 1, k + 5)          # (the plain programs keep their statement numbers: Id 16 .. 19 are the front's vectors)
    lines += ["%d,RangeV,val,0,Id %d,1" % (s - 1, sel), "%d,FoldSelect,val,Id %d,val,Id %d,val" % (s, s - 1, sel),
              "%d,Gather,Id 2,Id %d,val" % (s + 1, s), "%d,Gather,Id 6,Id %d,val" % (s + 2, s), "%d,Gather,Id 8,Id %d,val" % (s + 3, s + 1),
              "%d,RangeC,val,0,%d,1" % (p, DOMAIN), "%d,Partition,val,Id %d,val,Id %d,val" % (p + 1, s + 1, p),
              "%d,RangeV,val,0,Id %d,1" % (p + 2, s + 1),
              "%d,Scatter,Id %d,Id %d,val,Id %d,val" % (p + 3, s + 1, p + 2, p + 1), "%d,Scatter,Id %d,Id %d,val,Id %d,val" % (p + 4, s + 2, p + 2, p + 1),
              "%d,Scatter,Id %d,Id %d,val,Id %d,val" % (p + 5, s + 3, p + 2, p + 1),
              "%d,FoldSum,val,Id %d,val,Id %d,val" % (p + 6, p + 3, p + 4), "%d,FoldChoose,val,Id %d,val,Id %d,val" % (p + 7, p + 3, p + 5),
              "%d,FoldCount,val,Id %d,val,Id %d,val" % (p + 8, p + 3, p + 4)]
    q = p + 30
    gathered = []
    for i, t in enumerate(takes):
        lines.append("%d,Gather,Id %d,Id %d,val" % (q, t, s))
        gathered.append(("t%d" % i, q))
        q += 1
    named = {}
    for name, node in [(SUM, p + 6), (CHOOSE, p + 7), (COUNT, p + 8), (ROWS, s), (K, s + 1), (V, s + 2), (G, s + 3)] + gathered:
        lines.append("%d,MaterializeCompact,Id %d" % (q, node))
        named[name] = q
        q += 1
    return prog(*lines), named


# ---- survivor patterns: functions of the batch number -------------------------------------------------------------------------------
PATTERNS = ("all", "none", "signature", "isolated", "full head", "full tail")


def signature_count(b):
    return (7 * b + 3) % 13


def signature_positions():
    """where a batch's survivors sit, in the order they are handed out: its first row, its last row, both sides of each tile boundary,
    then rows beside those"""
    pos = [0, B - 1]
    for t in range(1, FRONT_BATCH):
        pos += [t * T - 1, t * T]
    extra = [1, B - 2] + [t * T + 1 for t in range(1, FRONT_BATCH)] + [t * T - 2 for t in range(1, FRONT_BATCH)] + [2, 3, 5, 7, 11, 13]
    for x in extra:
        if len(pos) < 12 and x not in pos and 0 <= x < B:
            pos.append(x)
    assert len(pos) == 12 and len(set(pos)) == 12
    return pos


def isolated_batches(nb):
    """batch 0, the batches around every power of 16 that fits, the last batch"""
    want = {0, nb - 1}
    p = FAN
    while p - 2 < nb:
        want.update(b for b in (p - 2, p - 1, p, p + 1) if 0 <= b < nb)
        p *= FAN
    return sorted(want)


def isolated_count(b):
    return 1 << (b % 11)


def head_batches(nb):
    """the largest power of 16 below the number of batches (1 when there are at most 16)"""
    p = 1
    while p * FAN < nb:
        p *= FAN
    return p


def pattern_mask(pattern, n):
    """the rows that are to survive, as a boolean array over the table's n rows"""
    nb = batches_of(n)
    if pattern == "all":
        return np.ones(n, bool)
    mask = np.zeros(n, bool)
    if pattern == "none":
        return mask
    if pattern == "signature":
        b = np.arange(nb, dtype=np.int64)
        cnt = signature_count(b)
        for s, p in enumerate(signature_positions()):
            at = b[cnt > s] * B + p
            mask[at[at < n]] = True
        return mask
    if pattern == "isolated":
        for b in isolated_batches(nb):
            c = isolated_count(b)
            stride = B // c
            at = b * B + np.arange(c, dtype=np.int64) * stride + (stride - 1 if b % 2 else 0)       # (odd batches end on their last row)
            mask[at[at < n]] = True
        return mask
    if pattern == "full head":
        mask[:head_batches(nb) * B] = True
        return mask
    assert pattern == "full tail", pattern
    mask[head_batches(nb) * B:] = True
    return mask


def batch_counts(mask):
    """survivors per batch"""
    nb = batches_of(len(mask))
    pad = np.zeros(nb * B, bool)
    pad[:len(mask)] = mask
    return pad.reshape(nb, B).sum(axis=1).astype(np.int64)


# ---- columns ----------------------------------------------------------------------------------------------------------------------
def dimension():
    """d.g: even rows pass program B's condition (6 .. 12), odd rows fail it (0 .. 5)"""
    i = np.arange(ND, dtype=np.int64)
    return np.where(i % 2 == 0, 6 + i % 7, i % 6).astype(np.int64)


def fact_a(mask, dimension_filter, seed=1):
    """f.a for a survivor mask: survivors hold 0 .. 6.  In program B a row that is not to survive fails on f.a alone, on d.g[f.k] alone or
    on both, by its row number modulo 3 (fact_k gives the second kind an odd key)."""
    n = len(mask)
    r = np.random.default_rng(seed).integers(0, 7, n).astype(np.int8)
    a = np.where(mask, r, r + 7 + 6 * (r & 1)).astype(np.int8)             # 0 .. 6 / 7 .. 18
    if dimension_filter:
        g_alone = ~mask & (np.arange(n) % 3 == 1)
        a[g_alone] = r[g_alone]
    return a


def fact_columns(mask, dimension_filter, seed=1):
    """f.k int32, f.a int8, f.v int32, d.g int64 such that exactly the rows of `mask` survive the program"""
    n = len(mask)
    rng = np.random.default_rng(seed + 1)
    k = (2 * rng.integers(0, ND // 2, n)).astype(np.int32)
    if dimension_filter:
        i = np.arange(n)
        k[~mask & (i % 3 != 0)] += 1
    v = rng.integers(-100, 100, n).astype(np.int32)
    return {"f.k": k, "f.a": fact_a(mask, dimension_filter, seed), "f.v": v, "d.g": dimension()}


def variant_columns(n, extra_filters, extra_takes, seed=5):
    """f.x0 .. (int8, every row passes 100 > x) and f.t0 .. (int16) of front_program's extra_filters / extra_takes"""
    rng = np.random.default_rng(seed)
    cols = {"f.x%d" % i: rng.integers(-128, 100, n).astype(np.int8) for i in range(extra_filters)}
    cols.update({"f.t%d" % i: rng.integers(-30000, 30000, n).astype(np.int16) for i in range(extra_takes)})
    return cols


def selection(cols, dimension_filter):
    """the mask as the program states it, from the columns"""
    sel = cols["f.a"].astype(np.int64) < 7
    if dimension_filter:
        sel &= cols["d.g"][cols["f.k"]] > 5
    return sel


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def front_reference(cols, dimension_filter, extra_takes=0):
    """every output of front_program in int64: the front's vectors in row order; SUM(v), g, COUNT(*) per key of k[mask] in key order by a
    stable argsort and reduceat"""
    sel = selection(cols, dimension_filter)
    rows = np.flatnonzero(sel).astype(np.int64)
    k = cols["f.k"][rows].astype(np.int64)
    v = cols["f.v"][rows].astype(np.int64)
    g = cols["d.g"][k].astype(np.int64)
    ref = {ROWS: rows, K: k, V: v, G: g}
    for i in range(extra_takes):
        ref["t%d" % i] = cols["f.t%d" % i][rows].astype(np.int64)
    order = np.argsort(k, kind="stable")
    sk, sv, sg = k[order], v[order], g[order]
    if len(sk):
        heads = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1])))
        ref.update({SUM: np.add.reduceat(sv, heads), CHOOSE: sg[heads], COUNT: np.diff(np.concatenate((heads, [len(sk)])))})
    else:
        ref.update({SUM: np.zeros(0, np.int64), CHOOSE: np.zeros(0, np.int64), COUNT: np.zeros(0, np.int64)})
    return ref


def outputs(results, named):
    return {name: out(results, node) for name, node in named.items()}


def front_mismatches(got, ref):
    """names of the outputs (arrays by name) that differ from the reference in length or in any value"""
    return [name for name in ref if name not in got or not np.array_equal(np.asarray(got[name], np.int64), ref[name])]


def front_column_counts(description):
    """(deciding columns, columns in all) of the fused front a plan's description shows: one "col" line per column of the scan, the
    deciding ones with their bounds; the select side of the kernel is instantiated for the former, the take side for the latter"""
    lines = description.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("fused front")][0]
    cols = []
    for ln in lines[at + 1:]:
        if not ln.startswith("  col "):
            break
        cols.append(ln)
    return sum(" in [" in ln for ln in cols), len(cols)


def front_output_columns(description):
    """how many columns the fused front of a plan's description hands over beside the row ids: the distinct `colN` among its statement
    vectors ("Id 16=rowid Id 17=col1 Id 18=col2 Id 22=rowid" -> 2).  run_projection sizes its output vectors by this number + 1."""
    (line,) = [ln for ln in description.splitlines() if ln.startswith("fused front")]
    vectors = re.findall(r"Id \d+=(\w+)", line)
    assert vectors and "rowid" in vectors, line
    return len({v for v in vectors if v != "rowid"})


def kept_note(timings, m, n):
    """the run's timing label of the front names m of n rows kept (run_projection: front_note)"""
    want = "_%d_of_%d_rows_kept" % (m, n)
    return [label for label in timings if "FusedFront" in label and want in label]


# ---- what a look-back error would leave (tests/test_front_cases_cpu.py) ------------------------------------------------------------
def displaced(ref, counts, batch, by):
    """the direct outputs as the front would leave them had batch `batch` added `by` (positive or negative) to its prefix: its survivors
    are written `by` places away, over whatever its neighbours wrote there; the places they should have gone to keep what the
    allocation held (zeros here)"""
    off = int(counts[:batch].sum())
    k = int(counts[batch])
    m = len(ref[ROWS])
    assert k > 0 and by != 0
    got = dict(ref)
    for name in DIRECT:
        a = ref[name].copy()
        a[off:off + k] = 0
        lo, hi = max(off + by, 0), min(off + by + k, m)              # (nothing is written beyond the capacity)
        if lo < hi:
            a[lo:hi] = ref[name][off + (lo - off - by):off + (hi - off - by)]
        got[name] = a
    return got
