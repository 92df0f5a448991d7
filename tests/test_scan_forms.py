"""Every form of a fused aggregate scan that the tuner can pick, pinned one at a time and compared bit for bit with the oracle at
the row counts where its tile logic branches; the precompiled variants the JIT-off path can select; and columns whose
frame-of-reference images sit exactly on the width limits of csrc/vdl_column_image.h.

The tuner (vdl_specialise.cpp: tune_specialised) times its candidates and keeps the quickest, so which form runs in a tuned
benchmark is decided by timing, not by the suite.  VDL_JIT_PIN leaves the tuner one candidate: the tests here pin each
(rows per lane u, staged form) pair in turn.  A form that does not exist for a scan (build_specialised refuses it) is
dropped by the tuner without a word; REFUSED lists every such refusal the tests expect, with its reason, and both the GPU
tests and the CPU test (vdl_plan_jit_check) fail on any other refusal and on a listed one that no longer happens.

Row counts per u (TILE = 512 u rows): one tile (grid 1), one tile and one row (a one-row tail), 37 tiles and 511 rows (an
odd tail that splits a lane's row pair), and for Q6 and Q1 4096 tiles and 3 rows over generated columns, where every block
runs several tiles."""
import os
import re

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import catalog, datagen, frontend
from conftest import ROOT
from helpers import oracle_run, prog

META = os.path.join(ROOT, "tests", "golden", "tpch10noorder")
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1

# ---- the tuner's candidates ------------------------------------------------------------------------------------------------
# (u, late): late 0 = every column with the tile, 1 / 2 = staged with that many filter columns with the tile, 3 = the queue
# form, 4 = every filter column with the tile ("lateall").  The tuner's {0, 1} candidate is the staged form at the quickest
# eager u, so late 1 runs at every eager u as well.
FORMS = [(2, 0), (3, 0), (4, 0), (6, 0), (1, 1), (2, 1), (3, 1), (4, 1), (6, 1), (2, 2), (3, 2), (4, 2), (3, 3), (4, 3), (6, 3),
         (2, 4), (3, 4), (4, 4)]
SUFFIX = {0: "", 1: ",late", 2: ",late2", 3: ",queue", 4: ",lateall"}


def form_id(f):
    return "u%d%s" % (f[0], SUFFIX[f[1]].replace(",", "_") or "_eager")


def tile(u):
    return 512 * u


def row_counts(u):
    return [tile(u), tile(u) + 1, 37 * tile(u) + 511]


# ---- forms a scan does not have --------------------------------------------------------------------------------------------
# build_specialised / vdl_plan_jit_check refuse a staged or queue form, by program, late and whether the scan's most selective
# filter column counts as selective (sampled fraction < 0.6: then the other filter columns and the sources of derived columns
# and of the group key are read late too, else only the aggregate inputs are).
NO_LATE = "no column to read late"
QUEUE_ONE = "the queue form wants exactly one filter column with the tile"
QUEUE_NOFILTER = "a column that is no filter would come with the tile"
FOLD = "the descriptor did not fold"
REFUSED = {
    # Q6, the global edge program: without a selective filter the other filter columns come with the tile
    ("q6", 3, False): QUEUE_ONE, ("edge_global", 3, False): QUEUE_ONE,
    # Q1, Q14, Q19, the grouped edge programs: without a selective filter the group key's or the lookups' sources come with the tile
    ("q1", 3, False): QUEUE_NOFILTER, ("q14", 3, False): QUEUE_NOFILTER, ("q19", 3, False): QUEUE_NOFILTER,
    ("edge_group", 3, False): QUEUE_NOFILTER, ("edge_group_affine", 3, False): QUEUE_NOFILTER,
    # Q12: every column is a filter column or the source of a lookup, nothing only an aggregate input: without a selective
    # filter nothing is left to read late
    ("q12", 1, False): NO_LATE, ("q12", 2, False): NO_LATE, ("q12", 3, False): NO_LATE, ("q12", 4, False): NO_LATE,
}
# Q12's grouped join scan (11 columns) at 3 and more rows per lane, in every form but the queue form, is 120-230 KB of code over
# its 8-byte columns and over its images (which it decodes): the compiler did not fold the descriptor, and the tuner drops the form


def too_large(program, u, late):
    return program == "q12" and u >= 3 and late != 3


def expected_refusal(program, u, late, selective):
    why = REFUSED.get((program, late, selective)) if late else None
    return why or (FOLD if too_large(program, u, late) else None)


# ---- TPC-H programs -------------------------------------------------------------------------------------------------------
TPCH = {"q6": 6, "q1": 1, "q14": 14, "q19": 19, "q12": 12}


def tpch(name, scale=2e-3, seed=5):
    cfg = frontend.load_metadata(META)
    text = frontend.compile_plan(open(os.path.join(META, "%02d.sql.mplan" % TPCH[name])).read(), cfg)
    return text, catalog.synth_columns(META, cfg, text, scale=scale, seed=seed)


def sliced(cols, n, last=None):
    """the fact table cut to its first n rows (foreign-key indices into the dimensions stay valid); last: the fact row that
    becomes row n - 1"""
    out = {k: (v[:n].copy() if k.startswith("lineitem.") else v) for k, v in cols.items()}
    if last is not None:
        for k, v in out.items():
            if k.startswith("lineitem."):
                v[n - 1] = cols[k][last]
    return out


_passing = {}


def passing_row(name, text, cols):
    """a fact row that passes every filter of the plan: the last row of the smallest prefix whose answer differs from that of
    no passing row at all (bisection with the oracle).  It becomes the table's last row, so that a kernel that drops the last
    row -- of a partial tile, of an unpaired late load -- changes the answer."""
    if name not in _passing:
        n = len(next(v for k, v in cols.items() if k.startswith("lineitem.")))
        none = oracle_run(text, sliced(cols, 1))
        assert oracle_run(text, sliced(cols, n)) != none, name
        lo, hi = 1, n                                           # the answer over lo rows is `none`, over hi rows it is not
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if oracle_run(text, sliced(cols, mid)) == none else (lo, mid)
        _passing[name] = hi - 1
    return _passing[name]


# ---- edge-value columns: images on the width limits of vdl_column_image.h ----------------------------------------------------
B = -(1 << 62) + 7                      # base of the affine columns
M4 = I64MAX - 3                         # top of the 4-byte affine column
L8 = 1 << 40                            # bottom of the column with no image
EDGE_IMAGES = {
    "t.p1": (1, 0, 1),                  # pure 1-byte: int64 in [-128, 127]
    "t.p2": (2, 0, 1),                  # pure 2-byte: int32 in [-32768, 32767]
    "t.a1": (1, B, 1000),               # affine 1-byte: B + 1000 e, e in [0, 127]
    "t.a2": (2, B, 1000),               # affine, one step more: e in [0, 128] crosses to 2 bytes
    "t.w4": (4, M4 - (2**31 - 1), 1),   # affine 4-byte near INT64_MAX: span 2^31 - 1
    "t.w8": (0, 0, 1),                  # span 2^31: no image
    "t.mn": (2, I64MIN, 1000),          # base INT64_MIN: INT64_MIN + 1000 k, k in [0, 30000]
    "t.ak": (1, 5, 10),                 # affine group key: 5 + 10 e, e in [0, 40] (pure would take 2 bytes)
}


def edge_columns(n, seed=11):
    """the edge table: every column's two ends in the first rows (so that each image reaches both), its two smallest and two
    largest values again in about 2 % of the rows each (so that a filter bound at an end decides many rows, independently of the
    other columns), and a last row of middle values that passes the filters of every edge program (so that a kernel that drops
    the table's last row changes the answer)"""
    r = np.random.default_rng(seed)

    def col(lo, hi, step, dtype=np.int64, mul=1, add=0, mid=None):
        e = r.integers(lo, hi + 1, n, dtype=np.int64)
        for v in (lo, lo + step, hi - step, hi):
            e[r.random(n) < 0.02] = v
        e[:3] = [lo, hi, lo + step][:n]
        e[n - 1] = mid
        return (np.int64(add) + np.int64(mul) * e).astype(dtype) if mul != 1 or add else e.astype(dtype)

    with np.errstate(over="ignore"):
        return {
            "t.p1": col(-128, 127, 1, mid=0),
            "t.p2": col(-32768, 32767, 1, np.int32, mid=0),
            "t.a1": col(0, 127, 1, mul=1000, add=B, mid=64),
            "t.a2": col(0, 128, 1, mul=1000, add=B, mid=64),
            "t.w4": col(-(2**31 - 1), 0, 1, add=M4, mid=-(2**30)),       # (M4 - 2^30: the bound of bound set 0 and of edge_group)
            "t.w8": col(0, 2**31, 1, add=L8, mid=2**30),
            "t.mn": col(0, 30000, 1, mul=1000, add=I64MIN, mid=15000),
            "t.ak": col(0, 40, 1, mul=10, add=5, mid=20),
        }


def choose(stored, mn, mx, p):
    """vdl_column_image.h: choose(), written again from its comment"""
    def narrowest(lo, hi):
        return next((w for w in (1, 2, 4) if -(1 << (8 * w - 1)) <= lo and hi < (1 << (8 * w - 1))), 8)
    if mn > mx or stored <= 1:
        return (0, 0, 1)
    p = min(max(p, 0), 18)
    pure = narrowest(mn, mx)
    aff, base, scale = 8, mn, 10 ** p
    if mx - mn <= I64MAX:
        aff = narrowest(0, (mx - mn) // scale)
    w = min(pure, aff)
    if w >= stored:
        return (0, 0, 1)
    return (w, 0, 1) if pure <= aff else (w, base, scale)


class Prog:
    def __init__(self):
        self.lines, self.nid, self.c = [], 0, {}

    def emit(self, body):
        self.nid += 1
        self.lines.append("%d,%s" % (self.nid, body))
        return self.nid

    def col(self, name):
        if name not in self.c:
            self.c[name] = self.emit("Project,val,Id %d,%s" % (self.emit("Load,t." + name), name))
        return self.c[name]

    def const(self, k, ref):
        return self.emit("RangeV,val,%d,Id %d,0" % (k, ref))

    def bin(self, op, a, b):
        return self.emit("%s,val,Id %d,val,Id %d,val" % (op, a, b))

    def range_filter(self, name, lo, hi):
        """lo <= x <= hi (None: open) as the frontend writes it: x > lo or x = lo, lo > x ... """
        x, terms = self.col(name), []
        if lo is not None:
            k = self.const(lo, x)
            terms.append(self.bin("LogicalOr", self.bin("Greater", x, k), self.bin("Equals", k, x)))
        if hi is not None:
            k = self.const(hi, x)
            terms.append(self.bin("LogicalOr", self.bin("Greater", k, x), self.bin("Equals", x, k)))
        return terms

    def select(self, filters):
        terms = [t for f in filters for t in self.range_filter(*f)]
        p = terms[0]
        for t in terms[1:]:
            p = self.bin("LogicalAnd", p, t)
        return self.emit("FoldSelect,val,Id %d,val,Id %d,val" % (self.emit("RangeV,val,0,Id %d,1" % p), p))

    def text(self):
        return prog(*self.lines)


# bound sets of the global edge program: (column, lo, hi), None = one-sided.  Bound set 0 runs through every form.  The others
# each put one or two bounds on an image's edge -- min - 1, min, min + 1, max - 1, max, max + 1, between two steps of a scale-1000
# column, past what the width holds -- beside a wide filter on another column; every set keeps rows, and every filter in it
# changes which (test_bound_sets_keep_rows_their_filters_decide)
BOUNDS = [
    [("p1", -127, 126), ("a1", B + 500, B + 126000), ("w4", None, M4 - 2**30)],
    [("p1", -129, 126), ("a1", B - 1, B + 126999), ("mn", I64MIN, I64MIN + 1000 * 29999)],
    [("p1", -128, -100), ("a1", B + 1, B + 127000)],
    [("p2", -32769, -32767), ("p1", None, 100)],                     # below the 2-byte width
    [("p2", 32766, 32768), ("a1", B + 1000, None)],                 # above it
    [("a2", B + 127999, B + 10**15), ("p1", -100, None)],           # between the last two steps, past the 2-byte width
    [("a1", B - 10**17, B + 999), ("p2", None, 0)],                 # past the 1-byte width below, between the first two steps
    [("mn", None, I64MIN + 999), ("p1", -50, 50)],                  # base INT64_MIN: between its first two steps
    [("mn", I64MIN + 1, I64MIN + 1001), ("a1", None, B + 100000)],
    [("mn", I64MIN + 1000 * 30000, None), ("w8", None, L8 + 2**30)],
    [("w4", M4, M4 + 1), ("p2", -30000, 30000)],                     # the 4-byte image's top, one past it
    [("w4", M4 - (2**31 - 1) - 1, M4 - (2**31 - 1) + 1), ("a2", B + 1000, B + 127000)],
    [("w8", L8 + 2**31, None), ("p1", None, 0)],                     # no image: max
    [("w8", L8 - 1, L8), ("a1", B + 64000, None)],                   # no image: min - 1 .. min
    [("p1", 126, None), ("a2", B + 64000, None)],
    [("p1", None, -128), ("p2", None, 0)],
]


def edge_global(bounds=0):
    """one fused global scan: 3 range filters, a wrapping FoldSum of products, FoldMin / FoldMax near the int64 ends, FoldCount"""
    g = Prog()
    for c in ("p1", "p2", "a1", "a2", "w4", "w8", "mn"):
        g.col(c)
    sel = g.select(BOUNDS[bounds])
    take = lambda c: g.emit("Gather,Id %d,Id %d,val" % (g.col(c), sel))
    outs = [("FoldSum", g.bin("Multiply", take("a1"), take("p2"))),            # (-2^62 ... ) x 32767: wraps mod 2^64
            ("FoldSum", g.bin("Multiply", take("w8"), take("mn"))),
            ("FoldMin", take("w4")), ("FoldMax", take("mn")), ("FoldMin", take("mn")), ("FoldMax", take("a2")), ("FoldCount", take("p1"))]
    for kind, t in outs:
        g.emit("MaterializeCompact,Id %d" % g.emit("%s,val,Id %d,val,Id %d,val" % (kind, g.emit("RangeV,val,0,Id %d,0" % t), t)))
    return g.text()


def edge_group(key="p1"):
    """one fused grouped scan over four columns, keyed on the pure 1-byte column (p1 + 128: 256 groups) or on the affine one
    (ak - 5: 41 groups)"""
    g = Prog()
    for c in ("a1", "w4", "mn", key):
        g.col(c)
    lo, dom = (-128, 256) if key == "p1" else (5, 401)
    sel = g.select([("a1", B + 3000, B + 124000), ("w4", M4 - 2**30, None)])
    take = lambda c: g.emit("Gather,Id %d,Id %d,val" % (g.col(c), sel))
    k = g.bin("Subtract", take(key), g.const(lo, g.col(key)))
    part = g.emit("Partition,val,Id %d,val,Id %d,val" % (k, g.emit("RangeC,val,0,%d,1" % dom)))
    skey = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (k, g.emit("RangeV,val,0,Id %d,1" % k), part))
    for kind, t in (("FoldSum", g.bin("Multiply", take("a1"), take("mn"))), ("FoldMin", take("w4")), ("FoldMax", take("mn")),
                    ("FoldCount", take("a1"))):
        st = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (t, g.emit("RangeV,val,0,Id %d,1" % t), part))
        g.emit("MaterializeCompact,Id %d" % g.emit("Project,%s,Id %d,val" % (kind.lower(), g.emit("%s,val,Id %d,val,Id %d,val" % (kind, skey, st)))))
    raw = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (take(key), g.emit("RangeV,val,0,Id %d,1" % k), part))
    g.emit("MaterializeCompact,Id %d" % g.emit("Project,key,Id %d,val" % g.emit("FoldChoose,val,Id %d,val,Id %d,val" % (skey, raw))))
    return g.text()


EDGE = {"edge_global": edge_global, "edge_group": lambda: edge_group("p1"), "edge_group_affine": lambda: edge_group("ak")}
# the columns each edge scan reads from images (vdl_plan_image_columns, role scan0), with their widths: every use of an affine
# column there is a range filter or an aggregate factor; a group key accepts a pure narrowing only
EDGE_IMAGE_COLUMNS = {
    "edge_global": {"t.p1": 1, "t.p2": 2, "t.a1": 1, "t.a2": 2, "t.w4": 4, "t.mn": 2},
    "edge_group": {"t.p1": 1, "t.a1": 1, "t.w4": 4, "t.mn": 2},
    "edge_group_affine": {"t.a1": 1, "t.w4": 4, "t.mn": 2},
}


def program(name, n=None):
    """(text, columns) of a program of the tables above, the fact table cut to n rows"""
    if name in EDGE:
        cols = edge_columns(n or 120000)
        keep = {"edge_global": ("p1", "p2", "a1", "a2", "w4", "w8", "mn"), "edge_group": ("p1", "a1", "w4", "mn"),
                "edge_group_affine": ("ak", "a1", "w4", "mn")}[name]
        cols = {"t." + k: cols["t." + k] for k in keep}
        return EDGE[name](), cols
    text, cols = tpch(name)
    return text, (sliced(cols, n) if n else cols)


# ---- CPU: the tables above against the rules and the planner ----------------------------------------------------------------
def test_forms_are_the_tuners_candidates():
    """FORMS covers the tuner's candidate list (vdl_specialise.cpp: tune_specialised), read from the source"""
    src = open(os.path.join(ROOT, "mplan2vdl_amd", "csrc", "vdl_specialise.cpp")).read()
    body = re.search(r"std::vector<std::pair<int, int>> cands = \{(.*?)\};", src, re.S).group(1)
    cands = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", body)]
    assert len(cands) == 17, cands
    eager_u = sorted(u for u, late in cands if late == 0)
    want = set()
    for u, late in cands:
        want |= {(x, late) for x in eager_u} if u == 0 else {(u, late)}
    assert want == set(FORMS), sorted(want ^ set(FORMS))


@pytest.mark.parametrize("name", sorted(EDGE_IMAGES))
def test_edge_columns_have_the_images_the_rules_choose(name):
    cols = edge_columns(5000)
    v = cols[name]
    assert v.min() == min(v[:2]) and v.max() == max(v[:2])       # the extremes sit in the first rows
    vals = [int(x) for x in v]
    tz = 19
    for x in vals:
        d = abs(x - vals[0])
        if d:
            z = 0
            while z < tz and d % 10 == 0:
                d //= 10
                z += 1
            tz = z
    assert choose(v.dtype.itemsize, min(vals), max(vals), tz) == EDGE_IMAGES[name]


def kept(cols, filters):
    keep = np.ones(len(cols["t.p1"]), bool)
    for c, lo, hi in filters:
        v = cols["t." + c].astype(np.int64)
        if lo is not None:
            keep &= v >= lo
        if hi is not None:
            keep &= v <= hi
    return keep


def test_bound_sets_keep_rows_their_filters_decide():
    """every bound set keeps rows at the n the GPU runs it at, and every one of its filters changes which: no bound is only ever
    compared with an empty answer or one it cannot change"""
    cols = edge_columns(37 * tile(2) + 511)
    for b, filters in enumerate(BOUNDS):
        k = kept(cols, filters)
        assert k.sum() >= 20, (b, int(k.sum()))
        for f in filters:
            without = kept(cols, [g for g in filters if g is not f])
            assert (without & ~k).any(), (b, f)


def test_the_last_row_of_every_edge_table_counts():
    """the answer of each edge program changes when its table loses the last row: a kernel that drops it is caught"""
    for name in EDGE:
        for n in sorted({n for u in (1, 2, 3, 4, 6) for n in row_counts(u)}):
            text, cols = program(name, n)
            assert oracle_run(text, cols) != oracle_run(text, {k: v[:-1] for k, v in cols.items()}), (name, n)
    cols = edge_columns(5000)
    for b, filters in enumerate(BOUNDS[:1]):
        assert kept(cols, filters)[-1], b


def declared_engine(cols, widths=None):
    e = m.Engine(device=None)
    for k, v in cols.items():
        e.register_pointer(k, 0x10000, (widths or {}).get(k, v.dtype.itemsize), len(v))
    return e


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_programs_fuse(name):
    text, cols = program(name, 5000)
    assert oracle_run(text, cols) is not None
    e = declared_engine(cols)
    p = e.parse(text)
    assert p.is_fused, p.describe()
    assert "key form: general" not in p.describe()
    e.close()
    for b in range(1, len(BOUNDS)):
        e = declared_engine(cols)
        p = e.parse(edge_global(b))
        assert p.is_fused, (b, p.describe())
        e.close()


def image_widths(cols):
    """each column declared at the width of its image, where it has one"""
    out = {}
    for k, v in cols.items():
        vals = v.astype(np.int64)
        d = np.abs(vals.astype(object) - int(vals[0]))
        tz = 19
        for x in set(int(y) for y in d if y):
            z = 0
            while z < tz and x % 10 == 0:
                x //= 10
                z += 1
            tz = min(tz, z)
        w = choose(v.dtype.itemsize, int(vals.min()), int(vals.max()), tz)[0]
        out[k] = w or v.dtype.itemsize
    return out


def refusals_of(note):
    return {int(s): why for s, why in re.findall(r"scan (\d+): not specialised \(([^)]*)\)", note)}


@pytest.mark.parametrize("name", list(TPCH) + list(EDGE))
def test_jit_check_refuses_what_the_tuner_refuses(name, tmp_path, monkeypatch):
    """every (VDL_JIT_U, VDL_JIT_LATE) pair built by hiprtc (no GPU) over the columns at their own and at their image widths, with
    and without selective filters: a form builds, or is refused for the reason REFUSED gives, and its code stays under the
    tuner's 96 KB limit"""
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    text, cols = program(name, 20000) if name in EDGE else tpch(name, scale=1e-4)
    for widths in (None, image_widths(cols)):
        e = declared_engine(cols, widths)
        p = e.parse(text)
        assert p.is_fused
        for selective in (False, True):
            monkeypatch.setenv("VDL_JIT_ASSUME_SELECTIVITY", "0.3" if selective else "1")
            for u, late in FORMS:
                monkeypatch.setenv("VDL_JIT_U", str(u))
                monkeypatch.setenv("VDL_JIT_GROUP_U", str(u))
                if late:
                    monkeypatch.setenv("VDL_JIT_LATE", str(late))
                else:
                    monkeypatch.delenv("VDL_JIT_LATE", raising=False)
                note = p.jit_check()
                why = expected_refusal(name, u, late, selective)
                got = refusals_of(note)
                assert got == ({0: why} if why and why != FOLD else {}), (name, u, late, selective, widths is not None, note)
                if not got:
                    tag = " (queue)" if late == 3 else " (late)" if late else ","
                    assert re.search(r"k_mscan_specialised<\d+,%d,[^>]*>%s" % (u, re.escape(tag)), note), (name, u, late, note)
                    sizes = [int(x) for x in re.findall(r"(\d+) B of code", note)]
                    assert sizes, note
                    if widths is None:                          # (columns declared narrow are not decoded: less code than over images)
                        assert (max(sizes) > 96 << 10) == (why == FOLD), (name, u, late, why, note)
                    else:
                        assert max(sizes) <= 96 << 10 or why == FOLD, (name, u, late, note)
        e.close()
    monkeypatch.delenv("VDL_JIT_LATE", raising=False)


# ---- GPU: every pinned form against the oracle -------------------------------------------------------------------------------
# whether a scan's filters count as selective when the tuner samples the columns of these tests
# (Q19's most selective column keeps more than 60 % of the sampled rows; the edge programs' w4 filter keeps half)
SELECTIVE_ON_GPU = {"q6": True, "q1": False, "q12": True, "q14": True, "q19": False, "edge_global": True, "edge_group": True,
                    "edge_group_affine": True}
GLOBAL = ("q6", "q14", "q19", "edge_global")
_want = {}


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one code-object cache for the module: a form compiles once across row counts (the cache is keyed by the source)"""
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


def oracle_of(name, n, text, cols):
    if (name, n) not in _want:
        _want[(name, n)] = oracle_run(text, cols)
    return _want[(name, n)]


def gpu_engine(cols, images):
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
        if k in EDGE_IMAGES:                                    # the ingest passes built the image the rules choose
            assert e.image_info(k) == EDGE_IMAGES[k], (k, e.image_info(k))
    e.set_column_images(images)
    return e


def scan_label(res):
    k = next(k for k in res["timings"] if "FusedScan_" in k)
    return k.split("FusedScan_", 1)[1]


def run_pinned(e, text, u, late):
    """one tuned run with the tuner left the single candidate (u, late): (results, note, kernel label of the dominant scan)"""
    p = e.parse(text)
    p.set_profiling(True)
    p.set_jit(True, tune=True)
    res = p.run()
    note, label = p.jit_note(), scan_label(res)
    p.close()
    return res["results"], note, label


def check_form(name, u, late, note, images, why):
    """the tuned note names the pinned form, or (where the form is refused) says nothing about tuning"""
    chosen = re.findall(r"scan 0 tuned:[^;]*-> (k_mscan_specialised<\d+,(\d+),[^>]*>)", note)
    if why:
        assert "tuned:" not in note, (name, u, late, why, note)
        return
    assert len(chosen) == 1, (name, u, late, note)
    kname, ku = chosen[0]
    assert int(ku) == u, (name, u, late, note)
    assert kname.endswith(SUFFIX[late] + ">") and (late or not re.search(r",(late|late2|queue|lateall)>", kname)), (name, u, late, note)
    if name in EDGE:
        assert (",img" in kname) == images, (name, images, note)
    elif not images:
        assert ",img" not in kname, note


# (the affine group key matters only where images are read)
PINNED = [(name, f, images) for name in list(TPCH) + list(EDGE) for f in FORMS for images in (True, False)
          if images or name != "edge_group_affine"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,form,images", PINNED, ids=["%s-%s-%s" % (n, form_id(f), "img" if i else "noimg") for n, f, i in PINNED])
def test_pinned_form_matches_the_oracle(name, form, images, jit_cache, monkeypatch):
    u, late = form
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % (u, late))
    settings = [(SELECTIVE_ON_GPU[name], {})]
    if late and name in GLOBAL:                                 # every filter counts as selective: the staged-filter code runs
        settings.append((True, {"VDL_JIT_ASSUME_SELECTIVITY": "0.3"}))
    if late:
        settings.append((SELECTIVE_ON_GPU[name], {"VDL_JIT_NO_PAIR_LOADS": "1"}))
    full_text, full_cols = program(name)
    for n in row_counts(u):
        text, cols = program(name, n) if name in EDGE else (full_text, sliced(full_cols, n, passing_row(name, full_text, full_cols)))
        want = oracle_of(name, n, text, cols)
        e = gpu_engine(cols, images)
        if name in EDGE:
            p = e.parse(text)
            p.run()
            assert p.image_columns().get("scan0", {}) == (EDGE_IMAGE_COLUMNS[name] if images else {}), (name, images, p.image_columns())
            p.close()
        for selective, env in settings:
            if env and n != row_counts(u)[-1]:                # (the extra settings at the odd tail only)
                continue
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got, note, label = run_pinned(e, text, u, late)
            for k in env:
                monkeypatch.delenv(k)
            assert got == want, (name, n, u, late, images, env, note)
            check_form(name, u, late, note, images, expected_refusal(name, u, late, selective))
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bounds", range(len(BOUNDS)))
def test_filter_bounds_at_the_image_ends_match_the_oracle(bounds, jit_cache, monkeypatch):
    """the global edge program under each bound set of BOUNDS, precompiled and in four pinned forms, images on and off"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    monkeypatch.setenv("VDL_JIT_ASSUME_SELECTIVITY", "0.3")    # (every staged form and the queue form exist for this scan)
    n = 37 * tile(2) + 511
    _, cols = program("edge_global", n)
    text = edge_global(bounds)
    want = oracle_run(text, cols)
    for images in (True, False):
        e = gpu_engine(cols, images)
        got, label = run_plain(e, text)
        assert got == want, (bounds, images, label)
        for u, late in ((2, 0), (2, 1), (3, 3), (2, 4)):
            monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % (u, late))
            got, note, label = run_pinned(e, text, u, late)
            assert got == want, (bounds, images, u, late, note)
            check_form("edge_global", u, late, note, images, None)
        e.close()


# ---- GPU: every block runs several tiles (Q6 and Q1 over generated columns, checked by the SQL loops of the oracle) ------------
GENERATED = {"q6": datagen.Q6_COLUMNS, "q1": datagen.Q1_COLUMNS}


def generated_want(query, n):
    import oracle
    from bench import Q1_SQL_ORDER
    order = datagen.Q6_COLUMNS if query == "q6" else Q1_SQL_ORDER
    specs = [(datagen.SEED, datagen.col_id(c), datagen.LINEITEM[c].lo, datagen.LINEITEM[c].hi, datagen.LINEITEM[c].mul,
              datagen.LINEITEM[c].add) for c in order]
    if query == "q6":
        rev, cnt = oracle.sql_q6_generated(specs, 0, n, threads=16)
        return [rev] if cnt else []
    return oracle.sql_q1_generated(specs, 0, n, threads=16)


def generated_matches(query, results, want):
    from bench import Q1_OUTPUTS
    if query == "q6":
        return results["tmp42"][".revenue"] == want
    flat = {list(v.keys())[0][1:]: list(v.values())[0] for v in results.values()}
    return all(flat.get(nm) == [int(x) for x in want[:, j]] for j, nm in enumerate(Q1_OUTPUTS))


MANY_TILES = [(q, u) for q in GENERATED for u in sorted({f[0] for f in FORMS})]


@pytest.mark.gpu
@pytest.mark.parametrize("query,u", MANY_TILES, ids=["%s-u%d" % x for x in MANY_TILES])
def test_pinned_forms_where_every_block_runs_several_tiles(query, u, jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    n = 4096 * tile(u) + 3
    text = open(os.path.join(ROOT, "tests", "golden", query + ".vdl")).read()
    want = generated_want(query, n)
    e = m.Engine(device=0)
    for name in GENERATED[query]:
        e.generate(datagen.LINEITEM[name], 0, n)
    ran = 0
    for images in (True, False):
        e.set_column_images(images)
        for late in [f[1] for f in FORMS if f[0] == u]:
            monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % (u, late))
            got, note, label = run_pinned(e, text, u, late)
            assert generated_matches(query, got, want), (query, n, u, late, images, note)
            why = expected_refusal(query, u, late, SELECTIVE_ON_GPU[query])
            check_form(query, u, late, note, images, why)
            if not why:
                grid = int(re.search(r"_grid(\d+)", label).group(1))
                assert n > 2 * grid * tile(u), (label, n)
                ran += 1
    e.close()
    assert ran


# ---- GPU: the precompiled variants (JIT off) ---------------------------------------------------------------------------------
def run_plain(e, text):
    p = e.parse(text)
    p.set_profiling(True)
    res = p.run()
    p.close()
    return res["results"], scan_label(res)


def variant_u(label):
    return int(re.match(r"k_mscan(?:_join)?<\d+,(\d+),", label).group(1))


def precompiled_cases():
    out = []
    for name in ("q6", "edge_global"):
        out.append((name, {"VDL_NO_KSCAN": "1"}))
    for name in ("q1", "edge_group"):
        for gu in ((1, 2, 3, 4) if name == "q1" else (1, 2, 3, 4, 6)):
            out.append((name, {"VDL_GROUP_U": str(gu)}))
        for r in (1, 2, 8):
            out.append((name, {"VDL_GROUP_TUNE": str(r)}))
    return out


# (the misaligned columns have one grouped variant, u = 4: VDL_GROUP_U does not apply to them)
PRECOMPILED = [(name, env, images, novec) for name, env in precompiled_cases() for images in (True, False) for novec in (False, True)
               if not (novec and "VDL_GROUP_U" in env)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,images,novec", PRECOMPILED,
                         ids=["%s-%s-%s-%s" % (n, "-".join("%s=%s" % kv for kv in e.items()), "img" if i else "noimg", "novec" if v else "vec")
                              for n, e, i, v in PRECOMPILED])
def test_precompiled_variant_matches_the_oracle(name, env, images, novec, monkeypatch):
    """Q6 and the global edge program on k_mscan (VDL_NO_KSCAN), Q1 and the grouped edge program on each grouped variant
    (VDL_GROUP_U) and replica count (VDL_GROUP_TUNE); novec: the columns one element off their allocation (torch tensors at an
    offset), where the variants without paired loads run -- an image is aligned, so with images on one column stays unencoded"""
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    full_text, full_cols = program(name)

    def run(n):
        text, cols = program(name, n) if name in EDGE else (full_text, sliced(full_cols, n, passing_row(name, full_text, full_cols)))
        want = oracle_of(name, n, text, cols)
        e = m.Engine(device=0)
        keep = []
        for i, (k, v) in enumerate(sorted(cols.items())):
            if novec:
                t = torch.tensor(np.concatenate([v[:1], v]), device="cuda:0")
                keep.append(t)
                e.register_tensor(k, t[1:])                     # shifted by one element: misaligned for the 2-row loads
                if images and i > 0:
                    e.encode(k)
                    if k in EDGE_IMAGES:
                        assert e.image_info(k) == EDGE_IMAGES[k], (k, e.image_info(k))
            else:
                e.upload(k, v)
                e.encode(k)
                if k in EDGE_IMAGES:
                    assert e.image_info(k) == EDGE_IMAGES[k], (k, e.image_info(k))
        e.set_column_images(images)
        got, label = run_plain(e, text)
        e.close()
        assert got == want, (name, n, env, images, novec, label)
        assert label.startswith("k_mscan<"), label
        assert (",false,false," in label) == novec, label
        if "VDL_GROUP_U" in env:
            assert variant_u(label) == int(env["VDL_GROUP_U"]), label
        if "VDL_GROUP_TUNE" in env:
            # (VDL_GROUP_TUNE is taken only where the replicas fit in 8192 words: 8 x 1280 words of the grouped edge program's 256
            # groups do not, and the default for 1280 words -- the largest r <= 8 whose r x words fit in 2304 -- is 1)
            r = int(env["VDL_GROUP_TUNE"])
            assert label.endswith("_rep%d" % (1 if name == "edge_group" and r == 8 else r)), label
        return label

    u = variant_u(run(37 * tile(6) + 511))                      # the variant does not depend on n: its u sets the row counts
    for n in row_counts(u):
        run(n)
