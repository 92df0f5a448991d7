"""What tests/test_partition_levels.py and tests/test_scan_levels.py share: the GROUP BY program around a Partition, its reference
in numpy (a stable argsort of the pivot buckets, folds by reduceat over the sorted rows), and a checker that decides in O(n) whether
positions are THE stable partition of their buckets -- for sizes at which a sort on the host would take longer than the test may.
tests/test_level_cases_cpu.py ties the reference to the oracle and shows what the checker rejects."""
import numpy as np

from helpers import prog

T = 8192                 # rows of a tile of a radix pass: VDL_PART_BLOCK x VDL_PART_STEPS (tests/test_partition_index_cpu.py guards it)
CT = 4096                # rows of a compaction tile: 64 x kCompactWords


def out(results, node):
    """the one value list of output `node` of a run"""
    (vals,) = results["tmp%d" % node].values()
    return np.asarray(vals, dtype=np.int64)


def buckets(keys, pmin, pcount):
    """clamp(key - pmin, 0, pcount) for int64 keys without anything wrapping: a key above pmin lies 1 .. 2^64 - 1 above it, which uint64 holds"""
    keys = np.asarray(keys, dtype=np.int64)
    above = keys > pmin
    diff = keys.astype(np.uint64) - np.uint64(pmin % (1 << 64))              # exact where `above`
    return np.where(above, np.minimum(diff, np.uint64(pcount)), np.uint64(0)).astype(np.int64)


# ---- the program -------------------------------------------------------------------------------------------------------------------
# key = t.k + t.j: computed, as every GROUP BY key the compiler emits is, so it reaches the Partition as a dense vector of its own (the
# form whose sorted values the last pass can write: vdl_genexec.h, partition_positions, `sorted_keys`).
KEY, VAL, SKEY, SVAL, SUM, CHOOSE, MAX, POS, SLOTS = "key", "val", "skey", "sval", "sum", "choose", "max", "pos", "slots"


def partition_program(pmin, pcount, eps, positions, sorted_rows=True):
    """-> (text, {name: output node}).  eps: rows with t.f == 0 are EPS (FoldSelect -> Gather); positions: the Partition is also
    materialised (else only Scatters read it)."""
    lines = ["1,Load,t.k", "2,Project,val,Id 1,k", "3,Load,t.j", "4,Project,val,Id 3,j", "5,Add,val,Id 2,val,Id 4,val", "6,Load,t.v", "7,Project,val,Id 6,v"]
    key, val, k, outs = 5, 7, 8, {}
    if eps:
        lines += ["8,Load,t.f", "9,Project,val,Id 8,f", "10,RangeV,val,0,Id 9,1", "11,FoldSelect,val,Id 10,val,Id 9,val",
                  "12,Gather,Id 5,Id 11,val", "13,Gather,Id 7,Id 11,val"]
        key, val, k = 12, 13, 14
        outs[SLOTS] = 11
    lines += ["%d,RangeC,val,%d,%d,1" % (k, pmin, pcount), "%d,Partition,val,Id %d,val,Id %d,val" % (k + 1, key, k),
              "%d,RangeV,val,0,Id %d,1" % (k + 2, key),
              "%d,Scatter,Id %d,Id %d,val,Id %d,val" % (k + 3, key, k + 2, k + 1), "%d,Scatter,Id %d,Id %d,val,Id %d,val" % (k + 4, val, k + 2, k + 1),
              "%d,FoldSum,val,Id %d,val,Id %d,val" % (k + 5, k + 3, k + 4), "%d,FoldChoose,val,Id %d,val,Id %d,val" % (k + 6, k + 3, k + 3),
              "%d,FoldMax,val,Id %d,val,Id %d,val" % (k + 7, k + 3, k + 4)]
    outs.update({SUM: k + 5, CHOOSE: k + 6, MAX: k + 7})
    if sorted_rows:
        outs.update({SKEY: k + 3, SVAL: k + 4})
    if positions:
        outs[POS] = k + 1
    k += 8
    named = {}
    for name, node in sorted(outs.items(), key=lambda kv: kv[1]):
        lines.append("%d,MaterializeCompact,Id %d" % (k, node))
        named[name] = k
        k += 1
    return prog(*lines), named


def partition_cols(keys, vals, rng, flags=None):
    j = rng.integers(0, 4, len(keys)).astype(np.int8)
    cols = {"t.k": (np.asarray(keys, np.int64) - j), "t.j": j, "t.v": np.asarray(vals, np.int64)}
    if flags is not None:
        cols["t.f"] = np.asarray(flags, np.int8)
    return cols


def outputs_from_order(keys, vals, order):
    """what the program leaves when `order` lists the non-EPS slots in rank order: runs are runs of equal KEY VALUES of the scattered rows"""
    sk, sv = keys[order], vals[order]
    heads = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1])))
    return {SKEY: sk, SVAL: sv, SUM: np.add.reduceat(sv, heads), CHOOSE: sk[heads], MAX: np.maximum.reduceat(sv, heads)}


def partition_reference(keys, vals, valid, pmin, pcount):
    """every output of partition_program from a stable argsort of the buckets"""
    keys, vals = np.asarray(keys, np.int64), np.asarray(vals, np.int64)
    slots = np.arange(len(keys)) if valid is None else np.flatnonzero(valid)
    local = np.argsort(buckets(keys[slots], pmin, pcount), kind="stable")
    ref = outputs_from_order(keys, vals, slots[local])
    pos = np.empty(len(slots), np.int64)
    pos[local] = np.arange(len(slots))
    ref[POS], ref[SLOTS] = pos, slots
    return ref


def mismatches(results, named, ref):
    """names of the outputs of a run that differ from the reference"""
    return [name for name, node in named.items() if not np.array_equal(out(results, node), ref[name])]


# ---- the checker -------------------------------------------------------------------------------------------------------------------
def stable_partition_error(bucket, valid, pos=None, slots=None, order=None):
    """None when the positions are the stable partition of the non-EPS rows by `bucket`, else what is wrong.  Three properties, each
    O(n), that leave exactly one answer: the positions of the valid rows are a permutation of 0 .. m-1; the buckets scattered by
    position do not descend; where neighbours are equal their originating slots ascend.
    Either `pos` (the positions of the rows `slots`, or of every valid row in slot order when slots is None) or `order` (the slots in
    rank order) is given."""
    n = len(bucket)
    want = np.arange(n) if valid is None else np.flatnonzero(valid)
    m = len(want)
    if order is None:
        pos = np.asarray(pos, np.int64)
        slots = want if slots is None else np.asarray(slots, np.int64)
        if len(slots) != m or not np.array_equal(slots, want):
            return "the rows that carry a rank are not the non-EPS rows (%d ranks, %d rows)" % (len(slots), m)
        if len(pos) != m:
            return "%d positions for %d rows" % (len(pos), m)
        if m and (pos.min() < 0 or pos.max() >= m):
            return "a position outside 0 .. m-1"
        if m and np.bincount(pos, minlength=m).max() != 1:
            return "a position is given out twice"
        order = np.empty(m, np.int64)
        order[pos] = slots
    else:
        order = np.asarray(order, np.int64)
        if len(order) != m:
            return "%d rows in rank order, %d non-EPS rows" % (len(order), m)
        if m and (order.min() < 0 or order.max() >= n):
            return "a slot outside the vector"
        seen = np.bincount(order, minlength=n)
        if m and seen.max() != 1:
            return "a row appears twice"
        if valid is not None and np.any(seen[np.flatnonzero(~np.asarray(valid, bool))]):
            return "an EPS row carries a rank"
    sb = np.asarray(bucket)[order]
    if np.any(sb[1:] < sb[:-1]):
        return "buckets descend at rank %d" % (int(np.flatnonzero(sb[1:] < sb[:-1])[0]) + 1)
    tie = sb[1:] == sb[:-1]
    if np.any(tie & (order[1:] < order[:-1])):
        return "equal buckets out of slot order at rank %d" % (int(np.flatnonzero(tie & (order[1:] < order[:-1]))[0]) + 1)
    return None


# ---- compaction and group-by references (tests/test_scan_levels.py) -----------------------------------------------------------------
def compact_program():
    """FoldSelect -> Gather -> MaterializeCompact: the selected values and the slot list"""
    return prog("1,Load,t.f", "2,Project,val,Id 1,f", "3,Load,t.a", "4,Project,val,Id 3,a", "5,RangeV,val,0,Id 2,1", "6,FoldSelect,val,Id 5,val,Id 2,val",
                "7,Gather,Id 4,Id 6,val", "8,MaterializeCompact,Id 7", "9,MaterializeCompact,Id 6"), {"picked": 8, "slots": 9}


def general_select_program():
    """one FoldSelect over general runs of a control vector with EPS slots; its values, where they sit (slot - value) and a Gather through it"""
    text = prog("1,Load,t.c", "2,Project,val,Id 1,c", "3,Load,t.f", "4,Project,val,Id 3,f", "5,Load,t.d", "6,Project,val,Id 5,d",
                "7,RangeV,val,0,Id 4,1", "8,FoldSelect,val,Id 7,val,Id 4,val", "9,Gather,Id 2,Id 8,val",             # control with holes
                "10,FoldSelect,val,Id 9,val,Id 6,val", "11,MaterializeCompact,Id 10",
                "12,RangeV,val,0,Id 10,1", "13,Subtract,val,Id 12,val,Id 10,val", "14,MaterializeCompact,Id 13",
                "15,Gather,Id 6,Id 10,val", "16,MaterializeCompact,Id 15")
    return text, {"hits": 11, "offset": 14, "data": 16}


def general_select_reference(ctl, ctl_ok, data):
    """FoldSelect over general runs (tests/vdl_model.py, fold_select) in numpy: the runs are the runs of equal values among the non-EPS
    control slots; the positions of a run's non-zero data are packed into the run's member slots from its first.  Returns (the slots
    that hold a value, the values), both in slot order."""
    members = np.flatnonzero(ctl_ok)
    c = np.asarray(ctl)[members]
    head = np.concatenate(([True], c[1:] != c[:-1]))
    first = np.flatnonzero(head)                                      # index among the members of each run's first member
    run = np.cumsum(head) - 1
    hit = np.asarray(data)[members] != 0
    hits = np.flatnonzero(hit)                                        # (indices among the members)
    before = np.concatenate(([0], np.cumsum(hit)))                    # hits among the members before each one
    start = first[run[hits]]
    return members[start + (before[hits] - before[start])], members[hits]


def group_by_program(domain):
    """the GROUP BY idiom over an int64 key column without EPS rows: Partition, the key and a value scattered, three folds"""
    text = prog("1,Load,t.k", "2,Project,val,Id 1,k", "3,Load,t.v", "4,Project,val,Id 3,v", "5,RangeC,val,0,%d,1" % domain,
                "6,Partition,val,Id 2,val,Id 5,val", "7,RangeV,val,0,Id 2,1", "8,Scatter,Id 2,Id 7,val,Id 6,val", "9,Scatter,Id 4,Id 7,val,Id 6,val",
                "10,FoldSum,val,Id 8,val,Id 9,val", "11,FoldChoose,val,Id 8,val,Id 8,val", "12,FoldCount,val,Id 8,val,Id 9,val",
                "13,MaterializeCompact,Id 10", "14,MaterializeCompact,Id 11", "15,MaterializeCompact,Id 12")
    return text, {"sum": 13, "key": 14, "count": 15}


def group_by_reference(keys, vals):
    """GROUP BY key: SUM(v), key, COUNT(*) in key order (keys inside the pivots: bucket order is key order)"""
    keys, vals = np.asarray(keys), np.asarray(vals)
    if np.any(keys[1:] < keys[:-1]):
        order = np.argsort(keys, kind="stable")
        keys, vals = keys[order], vals[order]
    heads = np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1])))
    return {"sum": np.add.reduceat(vals, heads), "key": keys[heads], "count": np.diff(np.concatenate((heads, [len(keys)])))}


def sorted_keys(n, shape, descent_at=None):
    """int64 keys in non-decreasing order: "distinct", "runs of 7", "one run"; "descent at the end" / descent_at=r: distinct with
    keys[r] one below keys[r - 1]"""
    i = np.arange(n, dtype=np.int64)
    if shape == "runs of 7":
        return 11 + 5 * (i // 7)
    if shape == "one run":
        return np.full(n, 123456789, np.int64)
    keys = 11 + 3 * i
    if shape == "descent at the end":
        descent_at = n - 1
    if descent_at is not None:
        keys[descent_at] = keys[descent_at - 1] - 1
    return keys
