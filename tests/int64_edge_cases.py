"""Directed programs at the ends of int64, shared by tests/test_int64_edges_cpu.py (oracle against the model) and
tests/test_int64_edges.py (engine against both): values near +-2^63, positions at and beyond 2^31 / 2^32, sums that wrap.
Every builder returns (text, columns); nothing here runs anything."""
import numpy as np

from helpers import make_heap, prog
from vdl_model import I64_MAX, I64_MIN, POOL, pool_column, pool_for

FUSABLE = ["Add", "Subtract", "Multiply", "Greater", "Equals", "LogicalAnd", "LogicalOr", "BitwiseAnd", "BitwiseOr", "BitShift"]
BINOPS = FUSABLE + ["Divide", "Modulo"]
FOLDS = ["FoldSum", "FoldMin", "FoldMax", "FoldChoose", "FoldCount"]
SHIFTS = [63, -63, 64, -64, 65, -65, I64_MIN, I64_MAX]
DTYPES = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64}


class Prog:
    """A program under construction: statements by id, columns by name; every vector's field is `val`."""

    def __init__(self):
        self.lines, self.nid, self.cols = [], 0, {}

    def emit(self, body):
        self.nid += 1
        self.lines.append("%d,%s" % (self.nid, body))
        return self.nid

    def load(self, name, arr):
        self.cols[name] = arr
        return self.emit("Project,val,Id %d,%s" % (self.emit("Load," + name), name.split(".", 1)[1]))

    def rangev(self, frm, ref, step): return self.emit("RangeV,val,%d,Id %d,%d" % (frm, ref, step))
    def const(self, k, ref): return self.rangev(k, ref, 0)
    def ids(self, ref): return self.rangev(0, ref, 1)
    def rangec(self, frm, count): return self.emit("RangeC,val,%d,%d,1" % (frm, count))
    def bin(self, op, a, b): return self.emit("%s,val,Id %d,val,Id %d,val" % (op, a, b))
    def ge(self, a, b): return self.bin("LogicalOr", self.bin("Greater", a, b), self.bin("Equals", a, b))          # a >= b as the compiler prints it
    def ne(self, a, b): return self.bin("Subtract", self.const(1, a), self.bin("Equals", a, b))                    # a != b likewise
    def gather(self, src, pos): return self.emit("Gather,Id %d,Id %d,val" % (src, pos))
    def scatter(self, src, pos, fold=None): return self.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (src, fold if fold else self.ids(src), pos))
    def select(self, cond): return self.emit("FoldSelect,val,Id %d,val,Id %d,val" % (self.ids(cond), cond))
    def fold(self, kind, ctl, data): return self.emit("%s,val,Id %d,val,Id %d,val" % (kind, ctl, data))
    def partition(self, key, piv): return self.emit("Partition,val,Id %d,val,Id %d,val" % (key, piv))
    def like(self, data, heap, pat): return self.emit("Like,val,Id %d,val,Id %d,val,%s" % (data, heap, pat))
    def out(self, v): return self.emit("MaterializeCompact,Id %d" % v)

    def filtered(self, vs, cond):
        """the vectors `vs` with EPS where cond is zero: Gather(v, FoldSelect(RangeV 0 1 cond, cond))"""
        sel = self.select(cond)
        return [self.gather(v, sel) for v in vs]

    def done(self):
        return prog(*self.lines), self.cols


def pool_table(p, rng, n, table="t"):
    """one pool column per storage width"""
    return {k: p.load("%s.%s" % (table, k), pool_column(rng, n, dt)) for k, dt in DTYPES.items()}


# ---- a. element-wise operators ------------------------------------------------------------------------------------------------
def elementwise(n, width, seed=1):
    rng = np.random.default_rng(seed)
    p = Prog()
    a = p.load("t.a", pool_column(rng, n, DTYPES[width]))
    b = p.load("t.b", pool_column(rng, n, np.int64))
    for k, op in enumerate(BINOPS):
        consts = SHIFTS if op == "BitShift" else [POOL[(5 * k + j * 11) % len(POOL)] for j in range(3)] + [0, -1]
        rights = [b] + [p.const(c, a) for c in consts] + [p.ids(a), p.rangev(I64_MAX - 2, a, 1), p.rangev(7, a, (1 << 62) + 1), p.rangev(I64_MIN + 4, a, -3)]
        for r in rights:
            p.out(p.bin(op, a, r))
            if op in ("Subtract", "Greater", "Divide", "Modulo", "BitShift"):
                p.out(p.bin(op, r, a))
    return p.done()


# ---- b. fused expression trees --------------------------------------------------------------------------------------------------
def _chain(p, op, leaves):
    """right-deep: l0 op (l1 op (l2 op ...)); every intermediate has one reader"""
    acc = leaves[-1]
    for x in reversed(leaves[:-1]):
        acc = p.ge(x, acc) if op == ">=" else p.ne(x, acc) if op == "!=" else p.bin(op, x, acc)
    return acc


def _left_chain(p, op, leaves):
    acc = leaves[0]
    for x in leaves[1:]:
        acc = p.bin(op, acc, x)
    return acc


def expr_chains(n, sparse=False, seed=2):
    """right-deep chains of 2, 4 and 8 leaves per fusable operator and idiom, trees one past each limit of the fused kernel
    (13 leaves, 49 instructions, depth 9), chains that Divide / Modulo cut; `sparse`: all of it over the entries of a selection"""
    rng = np.random.default_rng(seed)
    p = Prog()
    t = pool_table(p, rng, n)
    cols = [t["i64"], t["i32"], t["i16"], t["i8"], p.load("t.c", pool_column(rng, n, np.int64)), p.load("t.d", pool_column(rng, n, np.int64))]
    if sparse:
        flag = p.load("t.f", (np.arange(n) % 3 != 1).astype(np.int64))
        cols = p.filtered(cols, flag)
    ref = cols[0]

    def leaves(k, salt):
        # distinct leaves, a constant now and then (the >= / != idioms repeat their operands, so they stay on stored vectors)
        return [cols[(i + salt) % len(cols)] if (i + salt) % 5 else p.const(POOL[(7 * i + salt) % len(POOL)], ref) for i in range(k)]

    for j, op in enumerate(FUSABLE + [">=", "!="]):
        for k in (2, 4, 8):
            ls = [cols[(i + j) % len(cols)] for i in range(k)] if op in (">=", "!=") else leaves(k, j)
            p.out(_chain(p, op, ls))
    p.out(_left_chain(p, "Add", leaves(13, 1)))                       # 13 leaves
    p.out(_chain(p, "Subtract", leaves(9, 2)))                       # depth 9
    p.out(_left_chain(p, "BitwiseOr", [p.bin("BitwiseAnd", x, y) for x, y in zip(leaves(13, 3), leaves(13, 4))]))      # 26 leaves, 51 instructions
    for op in ("Divide", "Modulo"):                                  # the tree ends at a division
        inner = p.bin("Add", cols[0], cols[4])
        p.out(p.bin("Multiply", cols[5], p.bin(op, inner, p.bin("Subtract", cols[1], cols[2]))))
        p.out(p.bin("Add", p.bin(op, cols[0], cols[3]), p.bin("Multiply", cols[4], cols[5])))
    return p.done()


# ---- c. predicates and filters ------------------------------------------------------------------------------------------------------
def predicates(n, seed=3):
    """GT / EQ / GE / NE between pool columns of every width (one with EPS slots) under right-deep AND / OR chains of depth 8 and 9
    and left-deep ones of 16 and 17 comparisons, each read by the filter idiom"""
    rng = np.random.default_rng(seed)
    p = Prog()
    t = pool_table(p, rng, n)
    u = pool_table(p, rng, n, "u")
    holes = p.scatter(u["i64"], p.load("t.pos", np.where(np.arange(n) % 5 == 2, -1, np.arange(n)).astype(np.int64)))     # a stored vector with EPS slots
    pairs = [(t["i64"], u["i64"]), (t["i32"], u["i32"]), (t["i16"], u["i8"]), (t["i8"], u["i16"]), (t["i64"], u["i32"]), (holes, t["i64"]), (u["i64"], holes)]

    def cmp(i):
        a, b = pairs[i % len(pairs)]
        return [p.bin("Greater", a, b), p.bin("Equals", a, b), p.ge(a, b), p.ne(a, b), p.bin("Greater", b, a)][i % 5]

    def connect(i, x, y): return p.bin("LogicalAnd" if i % 3 else "LogicalOr", x, y)

    for count in (8, 9, 10):                                         # right-deep: the kernel's stack grows with the chain
        acc = cmp(count)
        for i in range(count - 1):
            acc = connect(i, cmp(i), acc)
        p.out(p.gather(t["i64"], p.select(acc)))
    for count in (16, 17):                                           # left-deep: many comparisons, shallow
        acc = cmp(0)
        for i in range(1, count):
            acc = connect(i, acc, cmp(i))
        p.out(p.gather(t["i32"], p.select(acc)))
        p.out(p.fold("FoldSum", p.const(0, acc), acc))
    return p.done()


def column_filters(n, seed=4):
    """conjunctions of per-column interval sets over raw table columns: bounds at both ends of int64, IN lists holding extremes,
    1, 2, 4 and 5 intervals, 1 and 6 columns"""
    rng = np.random.default_rng(seed)
    p = Prog()
    names = "abcdef"
    dts = [np.int64, np.int32, np.int64, np.int16, np.int8, np.int64]
    c = [p.load("t." + k, pool_column(rng, n, dt)) for k, dt in zip(names, dts)]
    x = c[0]

    def gt(v, k): return p.bin("Greater", v, p.const(k, v))
    def lt(v, k): return p.bin("Greater", p.const(k, v), v)
    def eq(v, k): return p.bin("Equals", v, p.const(k, v))
    def isin(v, ks):
        acc = eq(v, ks[0])
        for k in ks[1:]:
            acc = p.bin("LogicalOr", acc, eq(v, k))
        return acc

    tests = [gt(x, I64_MAX), lt(x, I64_MIN), p.ge(x, p.const(I64_MIN, x)), p.ge(p.const(I64_MAX, x), x), gt(x, I64_MAX - 1), lt(x, I64_MIN + 1),
             gt(x, I64_MIN), lt(x, I64_MAX), eq(x, I64_MIN), eq(x, I64_MAX),
             p.bin("LogicalAnd", gt(x, -(1 << 62) - 1), lt(x, (1 << 62) + 1)),
             isin(x, [I64_MIN, I64_MAX]), isin(x, [I64_MIN, -1, 1, I64_MAX]), isin(x, [I64_MIN, -64, 0, 64, I64_MAX]),
             isin(x, [I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX, 0])]
    for cond in tests:
        p.out(p.gather(x, p.select(cond)))
    six = gt(c[0], I64_MIN)
    for v, dt in zip(c[1:], dts[1:]):
        lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
        six = p.bin("LogicalAnd", six, p.bin("LogicalOr", isin(v, [lo, hi, 0]), p.bin("LogicalAnd", gt(v, 1), lt(v, hi))))
    sel = p.select(six)
    for v in c:
        p.out(p.gather(v, sel))
    return p.done()


def wide_i32_filters(n=4351, seed=5):
    """a 16-byte aligned int32 column of >= 4096 rows plus a tail, under bounds outside int32: everything passes or nothing does"""
    rng = np.random.default_rng(seed)
    p = Prog()
    x = p.load("t.x", pool_column(rng, n, np.int32))
    y = p.load("t.y", pool_column(rng, n, np.int64))

    def gt(v, k): return p.bin("Greater", v, p.const(k, v))
    def lt(v, k): return p.bin("Greater", p.const(k, v), v)

    for cond in (gt(x, -(1 << 31) - 1), gt(x, (1 << 31) - 1), gt(x, 1 << 31), lt(x, -(1 << 31)), lt(x, 1 << 31), gt(x, I64_MIN), lt(x, I64_MAX), gt(x, I64_MAX),
                 p.bin("LogicalAnd", gt(x, -(1 << 32)), lt(x, 1 << 32)), p.bin("LogicalAnd", gt(x, 1 << 32), lt(x, 1 << 33)),
                 p.bin("LogicalAnd", gt(x, -(1 << 31)), lt(x, (1 << 31) - 1)), p.bin("LogicalAnd", gt(x, -2), lt(x, 65))):
        sel = p.select(cond)
        p.out(p.gather(y, sel))
        p.out(p.fold("FoldCount", p.const(0, sel), sel))
    return p.done()


# ---- d. positions --------------------------------------------------------------------------------------------------------------------
def position_values(n, dtype=np.int64):
    """positions a kernel must refuse (negative, at / beyond n, +-2^31, 2^32 + k whose low 32 bits alias slot k, both ends of the
    type) among positions it must follow"""
    info = np.iinfo(dtype)
    bad = [-1, n, n + 1, 1 << 31, -(1 << 31), (1 << 31) - 1, 1 << 32, -(1 << 32), I64_MIN, I64_MAX, I64_MIN + 1, int(info.min), int(info.max)]
    bad += [(1 << 32) + k for k in (0, 1, min(63, n - 1), n - 1)] + [-(1 << 32) + k for k in (1, n - 1)]
    bad = [v for v in bad if info.min <= v <= info.max and not 0 <= v < n]
    good = [0, n - 1, n // 2, min(64, n - 1), min(63, n - 1)]
    return bad, good


def position_column(rng, n, m, dtype=np.int64):
    """m positions into a vector of n slots: refused and followed ones interleaved, then random followed ones"""
    bad, good = position_values(n, dtype)
    vals = [v for pair in zip(bad, (good * len(bad))[:len(bad)]) for v in pair]
    col = rng.integers(0, n, m).astype(dtype)
    k = min(m, len(vals))
    col[:k] = vals[:k]
    if m > 70:
        col[63], col[64], col[m - 1] = bad[0], bad[1 % len(bad)], bad[-1]
    return col


def unique_position_column(rng, n, m, dtype=np.int64):
    """m Scatter positions into n slots: the followed ones all different (the engine, like the compiler, takes Scatter positions to
    be unique: which of two slots that name one position lands is the oracle's and the model's to say, not a kernel's), the refused
    ones -- which write nothing -- as often as they like"""
    bad, _ = position_values(n, dtype)
    col = np.array([bad[i % len(bad)] for i in range(m)], dtype)
    slots = rng.choice(m, size=min(n, (m + 1) // 2), replace=False)
    col[slots] = rng.permutation(n)[:len(slots)].astype(dtype)
    return col


def positions(n, width="i64", seed=6):
    """Gather, Scatter and the filter over a gather with such positions, from an int64 or an int32 column"""
    rng = np.random.default_rng(seed)
    p = Prog()
    nu = max(n // 3, 1)
    x = p.load("u.x", pool_column(rng, nu, np.int64))
    mask = p.load("u.m", (np.arange(nu) % 2).astype(np.int64))
    pos = p.load("t.pos", position_column(rng, nu, n, DTYPES[width]))
    a = p.load("t.a", pool_column(rng, n, np.int64))
    upos = p.load("t.upos", unique_position_column(rng, nu, n, DTYPES[width]))
    p.out(p.gather(x, pos))
    p.out(p.scatter(a, upos, fold=x))
    p.out(p.scatter(p.ids(a), upos, fold=x))
    g = p.gather(mask, pos)                                           # read by the filter idiom only: the filter over a gather
    sel = p.select(g)
    p.out(p.gather(a, sel))
    xf, = p.filtered([x], mask)                                       # a filtered dimension column looked up through filtered positions
    posf, af = p.filtered([pos, a], p.bin("Greater", a, p.const(-3, a)))
    p.out(p.gather(xf, posf))
    p.out(p.bin("Add", p.gather(xf, posf), af))
    ones = p.const(1, posf)                                           # a semi-join set: ones at the positions, read back as positions
    s = p.scatter(ones, posf, fold=x)
    p.out(p.gather(x, p.select(s)))
    p.out(p.fold("FoldCount", p.const(0, s), s))
    return p.done()


def join_filter(n=4351, width="i64", seed=7):
    """the join-filter idiom of the compiler: a fact FK column against a dimension mask scattered by the filtered row ids"""
    rng = np.random.default_rng(seed)
    p = Prog()
    nu = 300
    ux = p.load("u.x", pool_column(rng, nu, np.int64))
    upk = p.load("u.u_pkey", np.zeros(nu, np.int64))
    fk = p.load("t.t_u", position_column(rng, nu, n, DTYPES[width]))
    a = p.load("t.a", pool_column(rng, n, np.int64))
    tpk = p.load("t.t_pkey", np.zeros(n, np.int64))
    sel_u = p.select(p.bin("Greater", ux, p.const(-2, ux)))
    ids = p.gather(p.ids(upk), sel_u)
    ones = p.const(1, ids)
    valid = p.scatter(ones, ids)
    posv = p.ids(ids)
    idx = p.scatter(posv, ids)
    fkf = p.gather(fk, p.ids(tpk))
    sm = p.select(p.gather(valid, fkf))
    gm = p.gather(p.gather(idx, fkf), sm)
    fa = p.gather(a, sm)
    dx = p.gather(ux, gm)
    p.out(fa)
    p.out(dx)
    zero = p.const(0, fa)
    p.out(p.fold("FoldSum", zero, p.bin("Multiply", fa, dx)))
    p.out(p.fold("FoldCount", zero, fa))
    return p.done()


def like_offsets(n, seed=8):
    rng = np.random.default_rng(seed)
    heap, where = make_heap(["PROMO BRUSHED", "STANDARD", "ECONOMY", "SMALL PROMO"])
    offs = sorted(where.values())
    p = Prog()
    h = p.load("u.s.heap", heap)
    bad = [-1, -(1 << 31), -(1 << 32), I64_MIN, len(heap), len(heap) + 1, 1 << 31, (1 << 32) + offs[0], I64_MAX, len(heap) - 1, 0, 3]
    col = np.array([offs[int(k)] for k in rng.integers(0, len(offs), n)], np.int64)
    k = min(n, len(bad))
    col[:k] = bad[:k]
    s = p.load("u.s", col)
    for pat in ("PROMO%", "%PROMO%", "%", "S_ANDARD", ""):
        m = p.like(s, h, pat)
        p.out(m)
        p.out(p.gather(s, p.select(m)))
    return p.done()


# ---- e. folds ------------------------------------------------------------------------------------------------------------------------
def run_keys(n, length):
    """control values in runs of `length` keyed INT64_MIN, INT64_MAX, INT64_MIN, ... with a pool value now and then"""
    keys = [I64_MIN, I64_MAX, I64_MIN, 0, I64_MAX, I64_MAX - 1, -1, I64_MIN + 1]
    return np.array([keys[(i // length) % len(keys)] for i in range(n)], np.int64)


def folds(n, holes="none", seed=9):
    """the five folds over one run, over general runs of 1 / 7 / 64 / 65 slots with control values from the pool, runs that hold
    only INT64_MAX / only INT64_MIN, sums that wrap more than once; holes: EPS in the data, the control, or both"""
    rng = np.random.default_rng(seed)
    p = Prog()
    x = p.load("t.x", pool_column(rng, n, np.int64))
    big = p.load("t.big", pool_column(rng, n, np.int64, [I64_MAX, I64_MAX - 1, I64_MIN, 1 << 62]))       # sums wrap again and again
    top = p.load("t.top", np.where((np.arange(n) // 7) % 2 == 0, I64_MAX, I64_MIN).astype(np.int64))    # whole runs of the identities
    x32 = p.load("t.x32", pool_column(rng, n, np.int32))
    data = [x, big, top, x32]
    ctls = {L: p.load("t.k%d" % L, run_keys(n, L)) for L in (1, 7, 64, 65)}
    if holes in ("data", "both"):
        data = p.filtered(data, p.load("t.fd", (np.arange(n) % 4 != 1).astype(np.int64)))
    if holes in ("control", "both"):
        fc = p.load("t.fc", (np.arange(n) % 7 != 3).astype(np.int64))
        ctls = dict(zip(ctls, p.filtered(list(ctls.values()), fc)))
    for d in data:
        ctls[0] = p.const(0, d if holes == "data" else ctls[1] if holes == "control" else d)      # one run over everything
        for L, ctl in ctls.items():
            for kind in FOLDS:
                p.out(p.fold(kind, ctl, d))
    return p.done()


# ---- f. Partition ------------------------------------------------------------------------------------------------------------------------
PMINS = [I64_MIN, I64_MIN + 1, -5, 0, I64_MAX - 3]
COUNTS = [1, 10, 255, 256, 1 << 30, 1 << 40, 1 << 62]


def partitions(n, shape, pmin, seed=10):
    """Partition of pool data by pivots RangeC pmin count 1 for every count: the positions written out, and the lazy order read only
    by Scatters and the folds over them (the GROUP BY lowering).  shape: shuffled | sorted | eps"""
    rng = np.random.default_rng(seed)
    p = Prog()
    k = pool_column(rng, n, np.int64)
    if shape == "sorted":
        k = np.sort(k)
    key = p.load("t.k", k)
    x = p.load("t.x", pool_column(rng, n, np.int64))
    if shape == "eps":
        key, x = p.filtered([key, x], p.load("t.f", (np.arange(n) % 5 != 0).astype(np.int64)))
    for count in COUNTS:
        piv = p.rangec(pmin, count)
        p.out(p.partition(key, piv))                                  # positions written out
        part = p.partition(key, p.rangec(pmin, count))                # read by Scatters only
        skey = p.scatter(key, part)
        sx = p.scatter(x, part)
        p.out(skey)
        for kind in FOLDS:
            p.out(p.fold(kind, skey, sx))
    return p.done()


# ---- g. Semisort (VLite dialect) ------------------------------------------------------------------------------------------------------------
def semisort(n, span, low, holes, seed=11):
    """holes: none | some | all.  Values in [low, low + span]."""
    rng = np.random.default_rng(seed)
    vals = sorted(set([low, low + span] + [low + span // 2, low + min(span, 1), low + max(span - 1, 0)]))
    col = np.array([vals[int(i)] for i in rng.integers(0, len(vals), n)], np.int64)
    col[0], col[n - 1] = low + span, low
    flag = np.ones(n, np.int64) if holes == "none" else np.zeros(n, np.int64) if holes == "all" else (np.arange(n) % 3 != 1).astype(np.int64)
    text = prog("1,Load,t.k", "2,Project,Id 1", "3,Load,t.f", "4,Project,Id 3", "5,RangeV,0,Id 4,1", "6,FoldSelect,Id 5,Id 4", "7,Gather,Id 2,Id 6",
                "8,Semisort,Id 7", "9,Output,Id 8", "10,Gather,Id 7,Id 8", "sorted,Output,decimal_0,Id 10",
                "12,RangeV,1,Id 10,0", "13,FoldSum,Id 10,Id 12", "counts,Output,decimal_0,Id 13")
    return text, {"t.k": col, "t.f": flag}


# ---- h. fused scans: column against column ---------------------------------------------------------------------------------------------------
def compare_scan(n, width, form, grouped=False, seed=12):
    """SELECT [g,] SUM(x), COUNT(*), MIN(x), MAX(x) FROM t WHERE a <cmp> b [GROUP BY g] with a, b pool columns of one width.
    form: gt (a > b) | lt (b > a) | ge (a >= b as the compiler prints it)"""
    rng = np.random.default_rng(seed)
    dt = DTYPES[width]
    p = Prog()
    av = pool_column(rng, n, dt)
    bv = pool_column(rng, n, dt)
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    if n > 8:                                                         # the pairs whose difference wraps, and their mirror images
        av[1:7] = [hi, lo, hi, lo, -1, 1]
        bv[1:7] = [-1, 1, lo, hi, hi, lo]
    a, b = p.load("t.a", av), p.load("t.b", bv)
    x = p.load("t.x", pool_column(rng, n, np.int64))
    g = p.load("t.g", (np.arange(n) * 7 % 5).astype(np.int32))
    cond = p.bin("Greater", a, b) if form == "gt" else p.bin("Greater", b, a) if form == "lt" else p.ge(a, b)
    sel = p.select(cond)
    fx, fg = p.gather(x, sel), p.gather(g, sel)
    if not grouped:
        zero = p.const(0, fx)
        for kind in ("FoldSum", "FoldMin", "FoldMax"):
            p.out(p.fold(kind, zero, fx))
        p.out(p.fold("FoldSum", zero, p.const(1, fx)))
        return p.done()
    part = p.partition(fg, p.rangec(0, 5))
    skey = p.scatter(fg, part)
    sx = p.scatter(fx, part)
    p.out(p.fold("FoldChoose", skey, skey))
    for kind in ("FoldSum", "FoldMin", "FoldMax", "FoldCount"):
        p.out(p.fold(kind, skey, sx))
    return p.done()


def compare_front(n, width, seed=13):
    """the comparison as the filter of a fused front: the survivors feed a GROUP BY over a sparse domain, which does not fuse"""
    rng = np.random.default_rng(seed)
    dt = DTYPES[width]
    p = Prog()
    av, bv = pool_column(rng, n, dt), pool_column(rng, n, dt)
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    if n > 8:
        av[1:7] = [hi, lo, hi, lo, -1, 1]
        bv[1:7] = [-1, 1, lo, hi, hi, lo]
    a, b = p.load("t.a", av), p.load("t.b", bv)
    x = p.load("t.x", pool_column(rng, n, np.int64))
    g = p.load("t.g", (np.arange(n) * 7919 % 100003).astype(np.int64))
    sel = p.select(p.bin("Greater", a, b))
    fx, fg = p.gather(x, sel), p.gather(g, sel)
    part = p.partition(fg, p.rangec(0, 1 << 38))
    skey = p.scatter(fg, part)
    sx = p.scatter(fx, part)
    p.out(p.fold("FoldChoose", skey, skey))
    p.out(p.fold("FoldSum", skey, sx))
    return p.done()


def compare_dimension(n, width, seed=14):
    """the comparison as the filter of the dimension side of a join (a dimension scan of the fused plan)"""
    rng = np.random.default_rng(seed)
    dt = DTYPES[width]
    p = Prog()
    nu = 257
    ua, ub = pool_column(rng, nu, dt), pool_column(rng, nu, dt)
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    ua[1:7] = [hi, lo, hi, lo, -1, 1]
    ub[1:7] = [-1, 1, lo, hi, hi, lo]
    a, b = p.load("u.a", ua), p.load("u.b", ub)
    upk = p.load("u.u_pkey", np.zeros(nu, np.int64))
    fk = p.load("t.t_u", (np.arange(n) * 5 % nu).astype(np.int64))
    x = p.load("t.x", pool_column(rng, n, np.int64))
    tpk = p.load("t.t_pkey", np.zeros(n, np.int64))
    sel_u = p.select(p.bin("Greater", a, b))
    ids = p.gather(p.ids(upk), sel_u)
    valid = p.scatter(p.const(1, ids), ids)
    fkf = p.gather(fk, p.ids(tpk))
    sm = p.select(p.gather(valid, fkf))
    fx = p.gather(x, sm)
    zero = p.const(0, fx)
    p.out(p.fold("FoldSum", zero, fx))
    p.out(p.fold("FoldSum", zero, p.const(1, fx)))
    return p.done()


def identity_aggregates(n, grouped, seed=15):
    """MIN over nothing but INT64_MAX and MAX over nothing but INT64_MIN, in a fused scan: the identity equals the value"""
    p = Prog()
    hi = p.load("t.hi", np.full(n, I64_MAX, np.int64))
    lo = p.load("t.lo", np.full(n, I64_MIN, np.int64))
    f = p.load("t.f", (np.arange(n) % 3).astype(np.int32))
    g = p.load("t.g", (np.arange(n) % 4).astype(np.int32))
    sel = p.select(p.bin("Greater", f, p.const(0, f)))
    fhi, flo, fg = p.gather(hi, sel), p.gather(lo, sel), p.gather(g, sel)
    if not grouped:
        zero = p.const(0, fhi)
        for kind, v in (("FoldMin", fhi), ("FoldMax", flo), ("FoldMax", fhi), ("FoldMin", flo), ("FoldSum", fhi), ("FoldSum", flo)):
            p.out(p.fold(kind, zero, v))
        return p.done()
    part = p.partition(fg, p.rangec(0, 6))                            # two buckets stay empty
    skey = p.scatter(fg, part)
    p.out(p.fold("FoldChoose", skey, skey))
    for kind, v in (("FoldMin", fhi), ("FoldMax", flo), ("FoldMax", fhi), ("FoldMin", flo), ("FoldSum", fhi)):
        p.out(p.fold(kind, skey, p.scatter(v, part)))
    return p.done()


def directed_programs(sizes=(1, 65, 4097)):
    """(name, text, columns) of every family at the given sizes: what the CPU test runs through the oracle and the model"""
    for n in sizes:
        for w in DTYPES:
            yield ("elementwise_%s_n%d" % (w, n),) + elementwise(n, w)
        for sparse in (False, True):
            yield ("expr_chains_%s_n%d" % ("sparse" if sparse else "dense", n),) + expr_chains(n, sparse)
        yield ("predicates_n%d" % n,) + predicates(n)
        yield ("column_filters_n%d" % n,) + column_filters(n)
        for w in ("i32", "i64"):
            yield ("positions_%s_n%d" % (w, n),) + positions(n, w)
        yield ("like_offsets_n%d" % n,) + like_offsets(n)
        for holes in ("none", "data", "control", "both"):
            yield ("folds_%s_n%d" % (holes, n),) + folds(n, holes)
        for shape in ("shuffled", "sorted", "eps"):
            for pmin in PMINS:
                yield ("partition_%s_pmin%d_n%d" % (shape, pmin, n),) + partitions(n, shape, pmin)
        for w in ("i32", "i64"):
            for form in ("gt", "lt", "ge"):
                for grouped in (False, True):
                    yield ("compare_scan_%s_%s_%s_n%d" % (w, form, "grouped" if grouped else "global", n),) + compare_scan(n, w, form, grouped)
            yield ("compare_front_%s_n%d" % (w, n),) + compare_front(n, w)
            yield ("compare_dimension_%s_n%d" % (w, n),) + compare_dimension(n, w)
        for grouped in (False, True):
            yield ("identity_aggregates_%s_n%d" % ("grouped" if grouped else "global", n),) + identity_aggregates(n, grouped)
    for w in ("i32", "i64"):
        yield ("join_filter_%s" % w,) + join_filter(4351, w)
    yield ("wide_i32_filters",) + wide_i32_filters()
    for n in (1, 65):
        for span, low in ((0, 5), (255, -255), (256, I64_MIN), (1 << 40, -(1 << 39)), ((1 << 62) - 1, -(1 << 61)), ((1 << 62) - 1, I64_MAX - (1 << 62) + 1)):
            for holes in ("none", "some"):
                yield ("semisort_span%d_low%d_%s_n%d" % (span, low, holes, n),) + semisort(n, span, low, holes)
        yield ("semisort_all_eps_n%d" % n,) + semisort(n, 3, 0, "all")
