"""An independent statement of the VDL operators in plain Python: a third evaluation beside the CPU oracle
and the engine, written from the design text and the operator comments, importing nothing of oracle/ or libvdl.

A vector is a list of Python ints plus a list of holds-a-value flags (False = EPS).  Arithmetic is done in Python's exact
integers and then wrapped to 64 bits explicitly, so nothing here can overflow the way the code under test might.  `run`
evaluates a program text (either dialect) over host columns and returns the result dict the oracle and the engine return.

Also here, because every edge test shares it: the value pool at the ends of int64 and the column builder that draws from it.
"""
import bisect
import re

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
_M = 1 << 64


def wrap(x):
    """An exact integer as the int64 that holds its low 64 bits."""
    x &= _M - 1
    return x - _M if x >> 63 else x


# ---- the value pool ----------------------------------------------------------------------------------------------------------
POOL = sorted(set(
    [I64_MIN, I64_MIN + 1, I64_MIN + 2, I64_MAX, I64_MAX - 1, I64_MAX - 2, 1 << 62, -(1 << 62)]
    + [s * (1 << b) + d for s in (1, -1) for b in (31, 32) for d in (-1, 0, 1)]
    + [s * v for s in (1, -1) for v in (63, 64, 65)]
    + [-2, -1, 0, 1, 2]))


def pool_for(dtype):
    """The part of the pool a column of `dtype` can store, plus that type's own two ends."""
    info = np.iinfo(dtype)
    return sorted(set([v for v in POOL if info.min <= v <= info.max] + [int(info.min), int(info.max)]))


def pool_column(rng, n, dtype=np.int64, values=None):
    """n draws from the pool (or from `values`), with the extremes pinned at slots 0, 63, 64 and the last slot."""
    vals = sorted(values) if values is not None else pool_for(dtype)
    col = np.array([vals[int(k)] for k in rng.integers(0, len(vals), n)], dtype=dtype)
    for slot, v in ((0, vals[0]), (63, vals[-1]), (64, vals[0]), (n - 1, vals[-1])):
        if 0 <= slot < n:
            col[slot] = v
    return col


# ---- vectors -----------------------------------------------------------------------------------------------------------------
class Vec:
    """vals / ok over n slots; a RangeC stays virtual (rng = (from, count, step)): pivots of 2^62 entries are never written out."""

    def __init__(self, vals=None, ok=None, field="val", rng=None):
        self.vals, self.field, self.rng = vals, field, rng
        self.ok = ok if ok is not None else ([True] * len(vals) if vals is not None else None)

    @property
    def n(self):
        return self.rng[1] if self.rng else len(self.vals)

    def named(self, field):
        v = Vec(self.vals, self.ok, field, self.rng)
        return v

    def written_out(self):
        if self.rng is None:
            return self
        frm, count, step = self.rng
        if count > 1 << 22:
            raise ValueError("a virtual range of %d slots is not written out" % count)
        return Vec([wrap(frm + i * step) for i in range(count)], None, self.field)


def shift(a, b):
    """BitShift a b: b >= 0 shifts right arithmetically, b < 0 shifts left by -b; the amount saturates at the word size."""
    if b >= 0:
        return a >> min(b, 63)                      # Python's >> on a negative int is arithmetic
    return 0 if b <= -64 else wrap(a << -b)


def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


BINARY = {
    "Add": lambda a, b: wrap(a + b),
    "Subtract": lambda a, b: wrap(a - b),
    "Multiply": lambda a, b: wrap(a * b),
    "Divide": lambda a, b: 0 if b == 0 else wrap(_trunc_div(a, b)),          # INT64_MIN / -1 = 2^63, which wraps to INT64_MIN
    "Modulo": lambda a, b: 0 if b in (0, -1) else a - b * _trunc_div(a, b),  # C remainder: the sign of the dividend
    "Greater": lambda a, b: int(a > b),
    "Equals": lambda a, b: int(a == b),
    "LogicalAnd": lambda a, b: int(a != 0 and b != 0),
    "LogicalOr": lambda a, b: int(a != 0 or b != 0),
    "BitwiseAnd": lambda a, b: wrap(a & b),
    "BitwiseOr": lambda a, b: wrap(a | b),
    "BitShift": shift,
}
FOLDS = ("FoldSum", "FoldMin", "FoldMax", "FoldChoose", "FoldCount")


def binary(op, a, b):
    assert a.n == b.n, "%s: operand lengths differ" % op
    f = BINARY[op]
    ok = [x and y for x, y in zip(a.ok, b.ok)]
    return Vec([f(x, y) if k else 0 for x, y, k in zip(a.vals, b.vals, ok)], ok)


def rangev(frm, ref, step):
    """len(ref) slots holding from + i*step (wrapping), EPS where ref is EPS."""
    return Vec([wrap(frm + i * step) for i in range(ref.n)], list(ref.ok) if ref.rng is None else [True] * ref.n)


def rangec(frm, count, step):
    assert count >= 0
    return Vec(rng=(frm, count, step))


def gather(src, pos):
    """out_i = src[pos_i]; EPS where the position is EPS, negative, at or beyond len(src), or the source slot is EPS."""
    src = src.written_out()
    vals, ok = [0] * pos.n, [False] * pos.n
    for i in range(pos.n):
        p = pos.vals[i]
        if pos.ok[i] and 0 <= p < src.n and src.ok[p]:
            vals[i], ok[i] = src.vals[p], True
    return Vec(vals, ok, src.field)


def scatter(src, fold, pos):
    """out[pos_i] = src_i over len(fold) slots; positions outside are dropped; on duplicates the later slot wins."""
    assert src.n == pos.n, "Scatter: source and position lengths differ"
    n = fold.n
    vals, ok = [0] * n, [False] * n
    for i in range(src.n):
        if src.ok[i] and pos.ok[i] and 0 <= pos.vals[i] < n:
            vals[pos.vals[i]], ok[pos.vals[i]] = src.vals[i], True
    return Vec(vals, ok, src.field)


def _runs(ctl):
    """The runs of a control vector: lists of member slots (EPS control slots are skipped and break nothing)."""
    runs, key = [], None
    for i in range(ctl.n):
        if not ctl.ok[i]:
            continue
        if not runs or ctl.vals[i] != key:
            runs.append([])
            key = ctl.vals[i]
        runs[-1].append(i)
    return runs


def fold_select(ctl, data):
    """The positions of the non-zero data of each run, packed into the run's member slots from its start.  Over unit runs
    (every call site the compiler emits): out_i = i where data_i is non-zero, EPS elsewhere."""
    assert ctl.n == data.n
    vals, ok = [0] * data.n, [False] * data.n
    for members in _runs(ctl):
        hits = [i for i in members if data.ok[i] and data.vals[i] != 0]
        for slot, i in zip(members, hits):
            vals[slot], ok[slot] = i, True
    return Vec(vals, ok)


def fold(kind, ctl, data):
    """FoldSum / Min / Max / Choose / Count over runs: the non-EPS data of a run folded into the run's first slot, EPS when
    the run holds no datum.  The first run of the vector starts at slot 0 whatever EPS control slots precede its first member."""
    assert ctl.n == data.n
    vals, ok = [0] * data.n, [False] * data.n
    for r, members in enumerate(_runs(ctl)):
        xs = [data.vals[i] for i in members if data.ok[i]]
        if not xs:
            continue
        first = 0 if r == 0 else members[0]
        vals[first] = {"FoldSum": lambda: wrap(sum(xs)), "FoldMin": lambda: min(xs), "FoldMax": lambda: max(xs),
                       "FoldChoose": lambda: xs[0], "FoldCount": lambda: len(xs)}[kind]()
        ok[first] = True
    return Vec(vals, ok)


def bucket(x, piv):
    """Index of the first pivot >= x; with pivots RangeC pmin count 1: 0 for x <= pmin, else min(x - pmin, count), exactly."""
    if piv.rng and piv.rng[2] == 1:
        pmin, count, _ = piv.rng
        return 0 if x <= pmin else min(x - pmin, count)
    p = piv.written_out()
    return bisect.bisect_left(p.vals, x)


def partition(data, piv):
    """The stable counting-sort destination of every non-EPS slot: its rank by (bucket, slot).  EPS in, EPS out."""
    rows = sorted((bucket(data.vals[i], piv), i) for i in range(data.n) if data.ok[i])
    vals = [0] * data.n
    for rank, (_, i) in enumerate(rows):
        vals[i] = rank
    return Vec(vals, list(data.ok))


def semisort(data):
    """The slots of the non-EPS values in stable ascending value order, packed at the front; the rest EPS."""
    rows = sorted((data.vals[i], i) for i in range(data.n) if data.ok[i])
    m = len(rows)
    return Vec([rows[k][1] if k < m else 0 for k in range(data.n)], [k < m for k in range(data.n)])


def like(data, heap, pattern):
    """SQL LIKE ('%', '_', no escape) of the 0-terminated string at each byte offset of `heap`; an offset outside the heap
    matches nothing; EPS where the offset is EPS."""
    rx = re.compile("".join(".*" if ch == "%" else "." if ch == "_" else re.escape(ch) for ch in pattern), re.S)
    text = bytes((v & 0xff) if k else 0 for v, k in zip(heap.vals, heap.ok)).decode("latin-1")
    vals = []
    for off, k in zip(data.vals, data.ok):
        if not k or not 0 <= off < heap.n:
            vals.append(0)
            continue
        end = text.find("\0", off)
        vals.append(int(rx.fullmatch(text[off:end if end >= 0 else len(text)]) is not None))
    return Vec(vals, list(data.ok))


def materialize_compact(v):
    v = v.written_out()
    return [x for x, k in zip(v.vals, v.ok) if k]


# ---- programs ----------------------------------------------------------------------------------------------------------------
def _ref(s):
    s = s.strip()
    assert s.startswith("Id "), "operand %r" % s
    return int(s[3:])


def run(text, cols):
    """The results of a program over host columns, {"tmpN": {".field": [values]}} like the oracle's and the engine's.
    A program with an Output statement is read as the VLite dialect (no field names; outputs are called `val` or by name)."""
    vlite = ",Output," in text
    vec, results, last = {}, {}, 0
    for raw in text.splitlines():
        line = raw.split(";;")[0].strip()
        if not line:
            continue
        f = line.split(",")
        op = f[1]
        named_output = vlite and op == "Output" and not re.fullmatch(r"\s*-?\d+\s*", f[0])
        nid = last + 1 if named_output else int(f[0])
        last = nid
        a = f[2:]
        if vlite:                                               # the same operands, without the field names between them
            if op == "Load":
                out = Vec([int(x) for x in cols[a[0]]])
            elif op in ("Project", "Shuffle"):
                out = vec[_ref(a[0])]
            elif op == "Semisort":
                out = semisort(vec[_ref(a[0])])
            elif op == "RangeV":
                out = rangev(int(a[0]), vec[_ref(a[1])], int(a[2]))
            elif op == "RangeC":
                out = rangec(int(a[0]), int(a[1]), int(a[2]))
            elif op == "Scatter":
                out = scatter(vec[_ref(a[0])], vec[_ref(a[1])], vec[_ref(a[2])])
            elif op == "Like":
                out = like(vec[_ref(a[0])], vec[_ref(a[1])], ",".join(a[2:]))
            elif op == "Output":
                out = vec[_ref(a[-1])].named(f[0] if named_output else "val")
                results["tmp%d" % nid] = {"." + out.field: materialize_compact(out)}
                vec[nid] = out
                continue
            else:
                x, y = vec[_ref(a[0])], vec[_ref(a[1])]
                out = (binary(op, x, y) if op in BINARY else fold_select(x, y) if op == "FoldSelect" else fold(op, x, y) if op in FOLDS
                       else partition(x, y) if op == "Partition" else gather(x, y) if op == "Gather" else None)
                assert out is not None, "operator %s" % op
            vec[nid] = out.named("val")
            continue
        if op == "Load":
            out = Vec([int(x) for x in cols[a[0]]], None, a[0].split(".", 1)[1] if "." in a[0] else a[0])
        elif op == "Project":
            assert vec[_ref(a[1])].field == a[2], line
            out = vec[_ref(a[1])].named(a[0])
        elif op == "Shuffle":
            out = vec[_ref(a[0])]
        elif op == "RangeV":
            out = rangev(int(a[1]), vec[_ref(a[2])], int(a[3]))
        elif op == "RangeC":
            out = rangec(int(a[1]), int(a[2]), int(a[3]))
        elif op == "Gather":
            out = gather(vec[_ref(a[0])], vec[_ref(a[1])])
        elif op == "Scatter":
            out = scatter(vec[_ref(a[0])], vec[_ref(a[1])], vec[_ref(a[3])])
        elif op == "Like":
            out = like(vec[_ref(a[1])], vec[_ref(a[3])], ",".join(a[5:])).named(a[0])
        elif op == "MaterializeCompact":
            out = vec[_ref(a[0])]
            results["tmp%d" % nid] = {"." + out.field: materialize_compact(out)}
        else:
            x, y = vec[_ref(a[1])], vec[_ref(a[3])]
            out = (binary(op, x, y) if op in BINARY else fold_select(x, y) if op == "FoldSelect" else fold(op, x, y) if op in FOLDS
                   else partition(x, y) if op == "Partition" else None)
            assert out is not None, "operator %s" % op
            out = out.named(a[0])
        vec[nid] = out
    return results
