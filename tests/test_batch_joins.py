"""Join batches on the GPU (Engine.set_batch_joins + Engine.run_batch): plans whose one scan has derived columns and a prelude and
that differ in range bounds alone are answered by ONE pass -- the prelude's tables are built once, a row is looked up once while any
plan still wants it -- and every plan's results equal, bit for bit, those of the same plan run alone and the oracle's for its text.

edge_join is a directed join scan: fact table t (an int32 date, an int64 price, an int8 discount, an int64 foreign key) against a
dimension u of 70 rows, so the dimension bitmap is two words with the second partly used.  u.x is looked up and range-filtered, u.y
looked up and aggregated, u.s a string tested by LIKE (a lookup table over its heap), u.z filtered on the dimension side (the bitmap);
the fact side compares two of its columns (price > date: a difference).  Foreign keys -1 and 70 make the row EPS for every plan.
The literal sets vary the date range and the range on u.x.  Every case pins 2 row pairs per lane and runs at one row more than a tile
and at 37 tiles and 511 rows, over images and over the columns themselves."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_jit as J
import test_scan_forms as F
from helpers import make_heap, oracle_run, prog
from test_batch_cpu import slots
from test_batch_joins_cpu import q12_years, q14_months, q4_quarters
from test_pipe_end import VDLRUN

pytestmark = pytest.mark.gpu

U = 2
ROWS = {"1tile": F.tile(U) + 1, "37tiles": 37 * F.tile(U) + 511}
NU = 70
WORDS = ["PROMO BRUSHED", "PROMO PLATED", "STANDARD", "MEDIUM POLISHED", "ECONOMY", "PROMOTION", "SMALL PROMO"]
D0 = 730000                                                     # the dates are D0 .. D0 + 999
# (date lo, date hi, x lo, x hi): two-sided ranges inside the columns' domains -- one shape
SETS = [(100, 700, 10, 80), (150, 650, 20, 90), (50, 500, 5, 60), (300, 900, 30, 70), (200, 800, 15, 85), (120, 420, 40, 95), (400, 950, 8, 55), (250, 600, 25, 75)]
EMPTY = (100, 700, 101, 120)                                    # u.x is 0 .. 99: no dimension row lies in the range
_cols, _want = {}, {}


def columns(n, seed=29):
    r = np.random.default_rng(seed)
    heap, where = make_heap(WORDS)
    offs = np.array(sorted(where.values()), np.int64)
    fk = r.integers(0, NU, n).astype(np.int64)
    fk[r.random(n) < 0.02] = -1                                 # outside the dimension: EPS for every plan
    fk[r.random(n) < 0.02] = NU
    fk[:8] = [0, 63, 64, 69, -1, NU, 1, 2]
    date = (D0 + r.integers(0, 1000, n)).astype(np.int32)
    price = r.integers(D0 - 3000, D0 + 200000, n).astype(np.int64)         # some prices lie at or below the date
    disc = r.integers(0, 11, n).astype(np.int8)
    # rows 4 and 5 (keys -1 and 70) would pass every set's fact filters; the last row passes every set
    date[4:6] = D0 + 410
    price[4:6] = D0 + 5000
    x = r.integers(0, 100, NU).astype(np.int64)
    z = r.integers(0, 10, NU).astype(np.int32)
    s = offs[r.integers(0, len(offs), NU)]
    x[[0, 63, 64, 69]] = [45, 46, 47, 48]
    z[[0, 63, 64, 69]] = 9
    s[[0, 64]] = where["PROMO PLATED"]
    date[n - 1], price[n - 1], fk[n - 1] = D0 + 410, D0 + 7000, 64
    return {"t.date": date, "t.price": price, "t.disc": disc, "t.fk": fk, "u.x": x, "u.y": r.integers(-5, 6, NU).astype(np.int32), "u.z": z,
            "u.s": s, "u.s.heap": heap, "u.u_pkey": np.zeros(NU, np.int64)}


class Emit:
    """the emitter idioms of test_random_joins.Gen"""
    def __init__(self):
        self.lines, self.nid = [], 0

    def emit(self, body):
        self.nid += 1
        self.lines.append("%d,%s" % (self.nid, body))
        return self.nid

    def load(self, name): return self.emit("Project,val,Id %d,%s" % (self.emit("Load," + name), name.split(".", 1)[1]))
    def const(self, k, ref): return self.emit("RangeV,val,%d,Id %d,0" % (k, ref))
    def pos(self, ref): return self.emit("RangeV,val,0,Id %d,1" % ref)
    def bin(self, op, a, b): return self.emit("%s,val,Id %d,val,Id %d,val" % (op, a, b))
    def gather(self, src, p): return self.emit("Gather,Id %d,Id %d,val" % (src, p))
    def select(self, pred): return self.emit("FoldSelect,val,Id %d,val,Id %d,val" % (self.pos(pred), pred))

    def between(self, x, lo, hi):
        a, b = self.const(lo, x), self.const(hi, x)
        return self.bin("LogicalAnd", self.bin("LogicalOr", self.bin("Greater", x, a), self.bin("Equals", a, x)),
                        self.bin("LogicalOr", self.bin("Greater", b, x), self.bin("Equals", x, b)))


def edge_join(bounds=SETS[0]):
    dlo, dhi, xlo, xhi = bounds
    g = Emit()
    c = {name: g.load(name) for name in ("t.date", "t.price", "t.disc", "t.fk", "u.x", "u.y", "u.z", "u.s", "u.u_pkey", "u.s.heap")}
    # the fact side's Select: the date range, and price > date (a difference of two fact columns)
    sel = g.select(g.bin("LogicalAnd", g.between(c["t.date"], D0 + dlo, D0 + dhi), g.bin("Greater", c["t.price"], c["t.date"])))
    fact = {k: g.gather(c[k], sel) for k in ("t.date", "t.price", "t.disc")}
    fact_pos = g.gather(g.pos(c["t.date"]), sel)
    # the dimension side: z > 2 as a validity mask and positions scattered by the filtered row ids
    sel_u = g.select(g.bin("Greater", c["u.z"], g.const(2, c["u.z"])))
    ids = g.gather(g.pos(c["u.u_pkey"]), sel_u)
    ones = g.const(1, ids)
    valid = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (ones, g.pos(ones), ids))
    posv = g.pos(ids)
    idx = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (posv, g.pos(posv), ids))
    # the fact side looks both up through the foreign key and is cleaned
    fkf = g.gather(c["t.fk"], fact_pos)
    sm = g.select(g.gather(valid, fkf))
    fact = {k: g.gather(v, sm) for k, v in fact.items()}
    gm = g.gather(g.gather(idx, fkf), sm)
    dim = {k: g.gather(c[k], gm) for k in ("u.x", "u.y", "u.s")}
    # a range on the looked-up x
    sx = g.select(g.between(dim["u.x"], xlo, xhi))
    fact = {k: g.gather(v, sx) for k, v in fact.items()}
    dim = {k: g.gather(v, sx) for k, v in dim.items()}
    like = g.emit("Like,val,Id %d,val,Id %d,val,PROMO%%" % (dim["u.s"], c["u.s.heap"]))
    price, disc, y = fact["t.price"], fact["t.disc"], dim["u.y"]
    terms = [("FoldCount", price), ("FoldSum", g.bin("Multiply", price, g.bin("Subtract", g.const(100, disc), disc))),
             ("FoldSum", g.bin("Multiply", g.bin("Multiply", like, price), g.bin("Add", g.const(7, y), y))), ("FoldMin", price), ("FoldMax", fact["t.date"])]
    for kind, t in terms:
        g.emit("MaterializeCompact,Id %d" % g.emit("%s,val,Id %d,val,Id %d,val" % (kind, g.const(0, t), t)))
    return prog(*g.lines)


def semi_join(bounds=(10, 80), modulus=None, dim=None):
    """Q4-shaped: the fact rows with b > 12 set the bits of the dimension rows they point at (mod N), the dimension scan tests the bit of
    its own row id and a range on x; the literal sets vary that range alone, so every plan builds the same set.
    dim: a filter on the dimension ahead of the set, as Q4's quarter -- ("eq", k): y = k, a range the outer scan applies itself;
    ("cmp",): x > y, a difference, which is no range on a table column"""
    xlo, xhi = bounds
    g = Emit()
    c = {name: g.load(name) for name in ("s.b", "s.s_pkey", "s.s_u", "u.x", "u.y", "u.u_pkey")}
    uids = g.pos(c["u.u_pkey"])
    if dim:
        su = g.select(g.bin("Equals", c["u.y"], g.const(dim[1], c["u.y"])) if dim[0] == "eq" else g.bin("Greater", c["u.x"], c["u.y"]))
        c["u.x"], c["u.y"], uids = g.gather(c["u.x"], su), g.gather(c["u.y"], su), g.gather(uids, su)
    p0 = g.pos(uids)
    idmap = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (p0, p0, uids))
    st = g.select(g.bin("Greater", c["s.b"], g.const(12, c["s.b"])))
    fk = g.gather(c["s.s_u"], g.gather(g.pos(c["s.s_pkey"]), st))
    hit = g.gather(idmap, fk)
    ones = g.const(1, hit)
    where = g.bin("Modulo", hit, g.const(modulus, hit))
    sel = g.select(g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (ones, g.pos(ones), where)))
    x, y = g.gather(c["u.x"], sel), g.gather(c["u.y"], sel)
    sx = g.select(g.between(x, xlo, xhi))
    x, y = g.gather(x, sx), g.gather(y, sx)
    for kind, t in (("FoldCount", x), ("FoldSum", g.bin("Multiply", x, g.bin("Add", y, g.const(3, y)))), ("FoldMax", x)):
        g.emit("MaterializeCompact,Id %d" % g.emit("%s,val,Id %d,val,Id %d,val" % (kind, g.const(0, t), t)))
    return prog(*g.lines)


SEMI_NU, SEMI_NS = 3000, 20000
SEMI_SETS = [(10, 80), (20, 90), (5, 60)]


def semi_columns(seed=31):
    r = np.random.default_rng(seed)
    fk = r.integers(0, SEMI_NU, SEMI_NS).astype(np.int64)
    fk[:3] = [-1, SEMI_NU, SEMI_NU - 1]
    return {"s.b": r.integers(0, 30, SEMI_NS).astype(np.int32), "s.s_pkey": np.zeros(SEMI_NS, np.int64), "s.s_u": fk,
            "u.x": r.integers(0, 100, SEMI_NU).astype(np.int64), "u.y": r.integers(0, 5, SEMI_NU).astype(np.int32), "u.u_pkey": np.zeros(SEMI_NU, np.int64)}


# ---- fixtures and helpers ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


@pytest.fixture
def pinned(jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    monkeypatch.setenv("VDL_JIT_PIN", "u=%d" % U)
    for name in ("VDL_BATCH_WIDTH", "VDL_BATCH_JOINS", "VDL_BATCH_GROUPED", "VDL_JIT_U", "VDL_JIT_GROUP_U"):
        monkeypatch.delenv(name, raising=False)


def table(n):
    if n not in _cols:
        _cols[n] = columns(n)
    return _cols[n]


def wanted(key, text, cols):
    """the oracle's answer for one text, computed once"""
    if key not in _want:
        _want[key] = oracle_run(text, cols)
    return _want[key]


def engine(cols, images, lookup_images=False, joins=True, grouped=False):
    e = F.gpu_engine(cols, images)
    if lookup_images:
        e.set_lookup_images(True)
    e.set_batch_joins(joins)
    e.set_batch_grouped(grouped)
    return e


def parse_all(e, texts, profiling=False):
    plans = [e.parse(t) for t in texts]
    for p in plans:
        assert p.is_fused, p.describe()
        p.set_jit(True, tune=True, runtime_bounds=True)        # (tuned: VDL_JIT_PIN leaves the one candidate at U row pairs)
        p.set_profiling(profiling)
    return plans


def results(replies):
    return [r["results"] for r in replies]


def check_kernel(notes, width, grouped=False):
    got = slots(notes)
    assert [(q, k) for _, q, k, _ in got] == [(q, width) for q in range(width)] and len({b for b, _, _, _ in got}) == 1, notes
    name = got[0][3]
    assert len({x[3] for x in got}) == 1 and ",derived" in name and name.endswith(",batch%d,rtb>" % width), name
    assert re.match(r"k_mscan_specialised<\d+,%d,(no)?vec,%s," % (U, "grouped" if grouped else "global"), name), name


def alone(e, texts):
    """every text as a plan of its own, run alone"""
    return [p.run()["results"] for p in parse_all(e, texts)]


def passes(cols, bounds):
    """per fact row: (the set's own filters hold, the row's key lies inside the dimension)"""
    dlo, dhi, xlo, xhi = bounds
    fk = cols["t.fk"]
    inside = (fk >= 0) & (fk < NU)
    k = np.where(inside, fk, 0)
    fact = (cols["t.date"] >= D0 + dlo) & (cols["t.date"] <= D0 + dhi) & (cols["t.price"] > cols["t.date"])
    dim = (cols["u.z"][k] > 2) & (cols["u.x"][k] >= xlo) & (cols["u.x"][k] <= xhi)
    return fact, fact & dim & inside, inside


# ---- edge_join ---------------------------------------------------------------------------------------------------------------------------
# K = 8 literal sets of 1 + 4 words are cut at the width cap of a scan of four aggregates (6): one batch of 6 and one of 2
SHAPES = [(images, limg, size) for images, limg in ((True, False), (False, False), (True, True)) for size in ROWS if not (limg and size == "37tiles")]
IDS = ["%s-%s" % ("limg" if limg else "img" if images else "noimg", size) for images, limg, size in SHAPES]


@pytest.mark.parametrize("images,limg,size", SHAPES, ids=IDS)
@pytest.mark.parametrize("width", [2, 3, 8])
def test_edge_join_batches(width, images, limg, size, pinned):
    n = ROWS[size]
    cols = table(n)
    sets = SETS[:width]
    texts = [edge_join(s) for s in sets]
    want = [wanted(("edge", n, s), t, cols) for s, t in zip(sets, texts)]
    e = engine(cols, images, limg)
    plans = parse_all(e, texts)
    got = results(e.run_batch(plans))
    notes = [p.batch_note() for p in plans]
    assert got == want, notes
    if width <= 6:
        check_kernel(notes, width)
    else:
        check_kernel(notes[:6], 6)
        check_kernel(notes[6:], 2)
    assert (",limg" in notes[0]) == limg, notes[0]
    assert all(0 < p.batch_code_bytes() < 96 << 10 for p in plans)
    assert alone(e, texts) == want
    e.close()


@pytest.mark.parametrize("images", [True, False], ids=["img", "noimg"])
def test_a_set_that_keeps_no_row_beside_two_that_do(images, pinned):
    n = ROWS["37tiles"]
    cols = table(n)
    sets = [SETS[0], EMPTY, SETS[1]]
    texts = [edge_join(s) for s in sets]
    want = [wanted(("edge", n, s), t, cols) for s, t in zip(sets, texts)]
    e = engine(cols, images)
    plans = parse_all(e, texts)
    got = results(e.run_batch(plans))
    assert got == want
    assert all(v == [] for entry in got[1].values() for v in entry.values())
    check_kernel([p.batch_note() for p in plans], 3)
    e.close()


# ---- TPC-H at scale 2e-3 -----------------------------------------------------------------------------------------------------------------
def tpch_case(name):
    if name == "q14":
        text, cols = F.tpch("q14")
        return cols, q14_months(text, range(8)), False
    if name == "q12":
        text, cols = F.tpch("q12")
        return cols, q12_years(text, range(4)), True
    text, cols = J.compiled(4, 2e-3, seed=5)
    return cols, q4_quarters(text, range(3)), True


def tables_built(fn):
    """(what fn returns, the prelude tables built meanwhile: LIKE tables, dimension bitmaps, semi-join sets -- mplan2vdl_amd.prelude_counters)"""
    import mplan2vdl_amd as m
    before = m.prelude_counters()["items"]
    out = fn()
    return out, m.prelude_counters()["items"] - before


# prelude tables a plan builds alone / a batch builds for all its members: Q14 its LIKE table; Q12 has no prelude; Q4 alone its orders
# bitmap and its semi-join set, a batch the set alone (the bitmap is left open)
TABLES = {"q14": (1, 1), "q12": (0, 0), "q4": (2, 1)}


@pytest.mark.parametrize("name", ["q14", "q12", "q4"])
def test_tpch_join_plans_share_one_pass(name, pinned):
    """Q14 for eight months, Q12 for four years and Q4 for three quarters: every answer is the plan's alone and the oracle's, one kernel
    served the batch, and the prelude's tables are built once per batch where K plans alone build them K times"""
    cols, texts, grouped = tpch_case(name)
    per_plan, per_batch = TABLES[name]
    want = [wanted((name, k), t, cols) for k, t in enumerate(texts)]
    assert len({json.dumps(w, sort_keys=True) for w in want}) == len(texts)
    e = engine(cols, True, grouped=grouped)
    plans = parse_all(e, texts, profiling=True)
    got, built = tables_built(lambda: e.run_batch(plans))
    notes = [p.batch_note() for p in plans]
    assert results(got) == want, notes
    assert built == per_batch, (built, notes)
    check_kernel(notes, len(texts), grouped)
    label = "timeInMicrosecondsForBatchedScan_" + slots(notes)[0][3]
    assert all(label in r["timings"] and r["timings"][label] > 0 for r in got), [r["timings"] for r in got]
    # the batch's one prelude is timed once, on its first plan
    others = [k for r in got for k in r["timings"] if k != label]
    assert others == (["timeInMicrosecondsForBatchedPrelude"] if per_batch else []) and (not per_batch or "timeInMicrosecondsForBatchedPrelude" in got[0]["timings"]), others
    ran, built = tables_built(lambda: alone(e, texts))
    assert ran == want and built == per_plan * len(texts), built
    e.close()


# ---- discipline ----------------------------------------------------------------------------------------------------------------------------
def test_batch_then_alone_then_batch_again_and_the_switch_off(pinned):
    import mplan2vdl_amd as m
    n = ROWS["37tiles"]
    cols = table(n)
    sets = SETS[:3]
    texts = [edge_join(s) for s in sets]
    want = [wanted(("edge", n, s), t, cols) for s, t in zip(sets, texts)]
    e = engine(cols, True)
    plans = parse_all(e, texts)
    assert results(e.run_batch(plans)) == want
    for k in (1, 2, 0):
        assert plans[k].batch_note().startswith("batch 0: slot %d of 3" % k)
        assert plans[k].run()["results"] == want[k]
        assert plans[k].batch_note() == "" and plans[k].batch_code_bytes() == 0
    before = m.jit_counters()["compiled"]
    assert results(e.run_batch(plans)) == want
    assert m.jit_counters()["compiled"] == before
    check_kernel([p.batch_note() for p in plans], 3)
    e.set_batch_joins(False)
    assert results(e.run_batch(plans)) == want
    assert all(p.batch_note().startswith("alone: ") and "are not batched" in p.batch_note() for p in plans), [p.batch_note() for p in plans]
    e.close()


# ---- semi-join sets ------------------------------------------------------------------------------------------------------------------------
def test_a_semi_join_set_is_built_once_for_the_batch(pinned):
    cols = semi_columns()
    texts = [semi_join(s, SEMI_NU + 7) for s in SEMI_SETS]
    want = [wanted(("semi", s), t, cols) for s, t in zip(SEMI_SETS, texts)]
    assert len({json.dumps(w, sort_keys=True) for w in want}) == 3
    e = engine(cols, True)
    plans = parse_all(e, texts)
    assert "semi-join set" in plans[0].describe()
    got, built = tables_built(lambda: results(e.run_batch(plans)))
    assert got == want and built == 1, (built, [p.batch_note() for p in plans])
    check_kernel([p.batch_note() for p in plans], 3)
    ran, built = tables_built(lambda: alone(e, texts))
    assert ran == want and built == 3
    e.close()


def test_a_dimension_bitmap_the_scan_repeats_is_left_open(pinned):
    """y = k ahead of the set, k another per plan (Q4's quarter): the outer scan applies y = k itself, so the batch leaves the bitmap open,
    builds ONE set for the three plans and each slot's own y = k drops the rest -- a plan alone builds its bitmap and its set"""
    cols = semi_columns()
    texts = [semi_join(s, SEMI_NU + 7, ("eq", k)) for k, s in enumerate(SEMI_SETS)]
    want = [wanted(("semi_eq", s), t, cols) for s, t in zip(SEMI_SETS, texts)]
    assert len({json.dumps(w, sort_keys=True) for w in want}) == 3 and all(v for w in want for en in w.values() for v in en.values())
    e = engine(cols, True)
    plans = parse_all(e, texts)
    got, built = tables_built(lambda: results(e.run_batch(plans)))
    assert got == want and built == 1, (built, [p.batch_note() for p in plans])
    check_kernel([p.batch_note() for p in plans], 3)
    ran, built = tables_built(lambda: alone(e, texts))
    assert ran == want and built == 6
    e.close()


def test_a_dimension_bitmap_that_is_no_range_on_table_columns_stays(pinned):
    """x > y ahead of the set: a difference, not a range the outer scan could be seen to repeat -- the bitmap is built (two tables per
    batch) and tested; the three plans share it because its text is the same"""
    cols = semi_columns()
    texts = [semi_join(s, SEMI_NU + 7, ("cmp",)) for s in SEMI_SETS]
    want = [wanted(("semi_cmp", s), t, cols) for s, t in zip(SEMI_SETS, texts)]
    assert len({json.dumps(w, sort_keys=True) for w in want}) == 3
    e = engine(cols, True)
    plans = parse_all(e, texts)
    got, built = tables_built(lambda: results(e.run_batch(plans)))
    assert got == want and built == 2, (built, [p.batch_note() for p in plans])
    check_kernel([p.batch_note() for p in plans], 3)
    e.close()


def test_a_set_taken_mod_less_than_its_table_sends_every_member_back_alone(pinned):
    cols = semi_columns()
    texts = [semi_join(s, SEMI_NU - 3) for s in SEMI_SETS]
    want = [wanted(("semi_wrap", s), t, cols) for s, t in zip(SEMI_SETS, texts)]
    e = engine(cols, True)
    plans = parse_all(e, texts, profiling=True)
    got = e.run_batch(plans)
    notes = [p.batch_note() for p in plans]
    assert results(got) == want, notes
    assert all(x.startswith("alone: rerun after batch 0: ") and "semi-join" in x for x in notes), notes
    assert all(any(k.startswith("fusedPlanAbandoned: ") for k in r["timings"]) and not any("BatchedScan" in k for k in r["timings"]) for r in got)
    assert all(p.batch_code_bytes() == 0 for p in plans)
    e.close()


# ---- vdlrun ----------------------------------------------------------------------------------------------------------------------------------
def test_vdlrun_batch_joins_end_to_end(tmp_path):
    """`vdlrun --jit --batch FILE --batch FILE --batch-joins --data DIR` over Q14 for three months; without the flag the notes say alone"""
    from mplan2vdl_amd import catalog
    text, cols = F.tpch("q14")
    texts = q14_months(text, range(3))
    coldir = str(tmp_path / "cols")
    catalog.export_columns(cols, coldir)
    args = [VDLRUN, "--jit", "--data", coldir]
    for k in (1, 2):
        path = tmp_path / ("q14_%d.vdl" % k)
        path.write_text(texts[k])
        args += ["--batch", str(path)]
    r = subprocess.run(args + ["--batch-joins"], input=texts[0].encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 3
    want = [wanted(("q14", k), t, cols) for k, t in enumerate(texts)]
    for k, line in enumerate(lines):
        assert json.load(io.StringIO(line))["results"] == want[k], k
    notes = re.findall(r"vdlrun: batch: (.*)", r.stderr.decode())
    assert [(q, k) for _, q, k, _ in slots(notes)] == [(0, 3), (1, 3), (2, 3)] and all(",derived" in x for x in notes), r.stderr.decode()[-2000:]
    off = subprocess.run(args, input=texts[0].encode(), capture_output=True, timeout=600)
    assert off.returncode == 0 and off.stdout.decode().splitlines() == lines
    notes = re.findall(r"vdlrun: batch: (.*)", off.stderr.decode())
    assert len(notes) == 3 and all(x.startswith("alone: ") and "are not batched" in x for x in notes), off.stderr.decode()[-2000:]
