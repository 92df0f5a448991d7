"""Grouped batches (vdl_set_batch_grouped, Engine.set_batch_grouped, VDL_BATCH_GROUPED=1) without a GPU: vdl_batch_jit_check groups
plans whose one scan is a GROUP BY over declared columns, chooses the batch width by the LDS rule, builds the grouped batch kernels
for gfx950 by hiprtc and fills the notes; the answers are checked on the device (test_batch_grouped.py).

group16: one fused grouped scan over five columns of table t, keyed on g (int64 in 0..15: a pure 1-byte image, pivots RangeC 0 16 1),
filtered by a range on f (B + 1000 e: an affine 1-byte image) and a range on h (int32 in -1000..1000: a pure 2-byte image), with a
wrapping FoldSum of x * y, FoldMin, FoldMax, FoldCount and the FoldChoose key: 16 groups x (1 + 5) words, so four plans' fifteen
class tables fit LDS at eight replicas.  f has no value with e in 60..69: a range inside that gap lies inside both images and keeps
no row.  With oob=True the rows whose e is 122 or more carry g in 16..19, outside the pivots: only a plan whose range on f reaches
that far sees them.

Over declared columns there are no images, so every variant of edge_group has one shape here (a bound "one step outside an image"
is an ordinary bound of an int64 column): the five of them are two batches of 2 and a plan left over.  What variants 3 and 4 become
over images is checked on the device (test_batch_grouped.py: test_edge_group_variants_of_other_shapes_run_alone)."""
import re

import numpy as np
import pytest

import mplan2vdl_amd as m
from test_batch_cpu import NOTE, slots
from test_jit_bounds_cpu import changed, program
from test_scan_forms import B, Prog

GAP = (60, 69)
OOB_FROM = 122


def columns(n, oob=False, seed=23):
    r = np.random.default_rng(seed)
    e = r.integers(0, 118, n, dtype=np.int64)
    e[e >= GAP[0]] += GAP[1] - GAP[0] + 1                      # 0..59, 70..127
    e[:2] = [0, 127]
    h = r.integers(-1000, 1001, n, dtype=np.int64)
    h[:2] = [-1000, 1000]
    g = r.integers(0, 16, n, dtype=np.int64)
    g[:2] = [0, 15]
    # four hot groups hold half the rows: lanes of a wave meet on the same words
    hot = r.random(n) < 0.5
    g[hot] = g[hot] % 4
    x = r.integers(-(1 << 61), 1 << 61, n, dtype=np.int64)      # x * y wraps mod 2^64
    y = r.integers(-30000, 30001, n, dtype=np.int64)
    e[n - 1], h[n - 1], g[n - 1] = 45, 0, 9                    # the last row passes every literal set
    if oob:
        out = e >= OOB_FROM
        g[out] = 16 + np.arange(n, dtype=np.int64)[out] % 4
    with np.errstate(over="ignore"):
        return {"t.g": g, "t.f": np.int64(B) + np.int64(1000) * e, "t.h": h.astype(np.int32), "t.x": x, "t.y": y.astype(np.int32)}


# (e_lo, e_hi, h_lo, h_hi): two-sided ranges strictly inside both images -- one shape
SETS = [(10, 100, -800, 800), (20, 90, -500, 900), (5, 50, -900, 100), (30, 120, -300, 300), (40, 110, -700, 650), (15, 75, -950, 950)]
EMPTY = (61, 68, -801, 801)                                    # inside the gap of f
REACHES_OOB = (31, 125, -301, 301)                             # admits e >= 122; SETS[0] and SETS[1] do not


def group16(bounds=SETS[0]):
    lo, hi, hlo, hhi = bounds
    g = Prog()
    for c in ("f", "h", "x", "y", "g"):
        g.col(c)
    sel = g.select([("f", B + 1000 * lo, B + 1000 * hi), ("h", hlo, hhi)])
    take = lambda c: g.emit("Gather,Id %d,Id %d,val" % (g.col(c), sel))
    k = g.bin("Subtract", take("g"), g.const(0, g.col("g")))
    part = g.emit("Partition,val,Id %d,val,Id %d,val" % (k, g.emit("RangeC,val,0,16,1")))
    skey = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (k, g.emit("RangeV,val,0,Id %d,1" % k), part))
    for kind, t in (("FoldSum", g.bin("Multiply", take("x"), take("y"))), ("FoldMin", take("x")), ("FoldMax", take("y")), ("FoldCount", take("f"))):
        st = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (t, g.emit("RangeV,val,0,Id %d,1" % t), part))
        g.emit("MaterializeCompact,Id %d" % g.emit("Project,%s,Id %d,val" % (kind.lower(), g.emit("%s,val,Id %d,val,Id %d,val" % (kind, skey, st)))))
    raw = g.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (take("g"), g.emit("RangeV,val,0,Id %d,1" % k), part))
    g.emit("MaterializeCompact,Id %d" % g.emit("Project,key,Id %d,val" % g.emit("FoldChoose,val,Id %d,val,Id %d,val" % (skey, raw))))
    return g.text()


GROUPED_NOTE = r"^batch (\d+): slot (\d+) of (\d+), (k_mscan_specialised<\d+,\d+,(?:no)?vec,grouped[^>]*,batch(\d+),rtb>)$"


# ---- the checks -------------------------------------------------------------------------------------------------------------------
ALONE_OFF = "alone: grouped scans are not batched"
LEFT_OVER = "alone: the one plan left over when its group was cut into batches of %d"


def texts_of(sets):
    base = group16()
    lo, hi, hlo, hhi = SETS[0]
    return [changed(base, {B + 1000 * lo: B + 1000 * a, B + 1000 * hi: B + 1000 * b, hlo: c, hhi: d}) if s != SETS[0] else base for s in sets for a, b, c, d in [s]]


def test_literal_sets_are_group16_with_its_constants_changed():
    assert texts_of(SETS[1:3] + [EMPTY, REACHES_OOB]) == [group16(s) for s in SETS[1:3] + [EMPTY, REACHES_OOB]]


@pytest.fixture
def g16(tmp_path, monkeypatch):
    import test_scan_forms as F
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    monkeypatch.delenv("VDL_BATCH_WIDTH", raising=False)
    monkeypatch.delenv("VDL_BATCH_GROUPED", raising=False)
    e = F.declared_engine(columns(5000))
    yield e
    e.close()


def parsed(e, texts):
    plans = [e.parse(t) for t in texts]
    for p in plans:
        assert p.is_fused, p.describe()
        p.set_jit(True)
    return plans


def grouped_slots(notes):
    got = slots(notes)
    for note in notes:
        assert re.match(GROUPED_NOTE, note), note
    return got


def test_switch_off_the_notes_are_the_parents(g16):
    plans = parsed(g16, texts_of(SETS[:3]))                    # (three: the batch of four is built, and counted, below)
    assert g16.batch_jit_check(plans) == [ALONE_OFF] * 3
    assert [p.batch_code_bytes() for p in plans] == [0] * 3
    g16.set_batch_grouped(True)
    assert all(NOTE.match(x) for x in g16.batch_jit_check(plans))
    g16.set_batch_grouped(False)
    assert g16.batch_jit_check(plans) == [ALONE_OFF] * 3


def test_the_environment_switches_it_on_when_the_context_opens(tmp_path, monkeypatch):
    import test_scan_forms as F
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("VDL_BATCH_GROUPED", "1")
    e = F.declared_engine(columns(5000))
    monkeypatch.setenv("VDL_BATCH_GROUPED", "0")               # (read when the context opened)
    assert [(q, k) for _, q, k, _ in grouped_slots(e.batch_jit_check(parsed(e, texts_of(SETS[:2]))))] == [(0, 2), (1, 2)]
    e.close()


def test_four_group16_sets_build_as_one_batch(g16):
    g16.set_batch_grouped(True)
    plans = parsed(g16, texts_of(SETS[:4]))
    before = m.jit_counters()["compiled"]
    notes = g16.batch_jit_check(plans)
    got = grouped_slots(notes)
    assert [(b, q, k) for b, q, k, _ in got] == [(0, q, 4) for q in range(4)], notes
    assert ",grouped" in got[0][3] and got[0][3].endswith(",batch4,rtb>") and len({name for _, _, _, name in got}) == 1
    assert m.jit_counters()["compiled"] == before + 1
    again = parsed(g16, texts_of([SETS[5], SETS[4], EMPTY, SETS[2]]))[::-1]        # other literals, another order: nothing compiles
    assert grouped_slots(g16.batch_jit_check(again)) == got
    assert m.jit_counters()["compiled"] == before + 1
    # the descriptor folded: a code object of the size of a specialised scan's
    assert all(0 < p.batch_code_bytes() < 64 << 10 for p in plans), [p.batch_code_bytes() for p in plans]


def test_batch_width_cuts_four_plans_into_two_batches_of_two(g16, monkeypatch):
    g16.set_batch_grouped(True)
    monkeypatch.setenv("VDL_BATCH_WIDTH", "2")
    got = grouped_slots(g16.batch_jit_check(parsed(g16, texts_of(SETS[:4]))))
    assert [(b, q, k) for b, q, k, _ in got] == [(0, 0, 2), (0, 1, 2), (1, 0, 2), (1, 1, 2)]
    monkeypatch.setenv("VDL_BATCH_WIDTH", "3")
    notes = g16.batch_jit_check(parsed(g16, texts_of(SETS[:4])))
    assert [(b, q, k) for b, q, k, _ in grouped_slots(notes[:3])] == [(0, q, 3) for q in range(3)] and notes[3] == LEFT_OVER % 3, notes


def test_edge_group_fits_two_plans_and_no_third(tmp_path, monkeypatch):
    """256 groups x 6 words: three class tables at one replica fit 64 KiB, seven do not"""
    import test_jit_bounds as JB
    import test_scan_forms as F
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    base, cols = F.program("edge_group", 5000)
    texts = [changed(base, mp) for mp, _ in JB.VARIANTS["edge_group"]]
    e = F.declared_engine(cols)
    e.set_batch_grouped(True)
    notes = e.batch_jit_check(parsed(e, texts[:3]))
    assert [(b, q, k) for b, q, k, _ in grouped_slots(notes[:2])] == [(0, 0, 2), (0, 1, 2)] and notes[2] == LEFT_OVER % 2, notes
    # all five have one shape over declared columns (no images): two batches and the left-over plan
    notes = e.batch_jit_check(parsed(e, texts))
    assert [(b, q, k) for b, q, k, _ in grouped_slots(notes[:4])] == [(0, 0, 2), (0, 1, 2), (1, 0, 2), (1, 1, 2)] and notes[4] == LEFT_OVER % 2, notes
    # a plan whose shape no other has runs alone with the words a global plan gets
    one_sided = changed(base, {B + 3000: -(1 << 63)})
    notes = e.batch_jit_check(parsed(e, texts[:2] + [one_sided]))
    assert notes[2] == "alone: its filter shapes differ from every other plan's", notes
    e.close()


def test_q1_and_q6_in_one_call_never_mix(tmp_path, monkeypatch):
    import test_jit as J
    from test_batch_cpu import literal_set
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    q6_text, e = program("q6")
    q1_text, q1_cols = J.compiled(1, 1e-4)
    for k, v in q1_cols.items():
        if k not in ("lineitem.l_shipdate", "lineitem.l_discount", "lineitem.l_quantity", "lineitem.l_extendedprice"):
            e.register_pointer(k, 0x10000, v.dtype.itemsize, 600000)
    e.set_batch_grouped(True)
    q1 = parsed(e, [q1_text, changed(q1_text, {729999: 729939}), changed(q1_text, {729999: 729879})])
    q6 = parsed(e, [changed(q6_text, literal_set(k)) for k in range(2)])
    plans = [q1[0], q6[0], q1[1], q1[2], q6[1]]
    notes = e.batch_jit_check(plans)
    got = slots(notes)
    assert [(got[i][0], got[i][1], got[i][2]) for i in (0, 2, 3)] == [(0, q, 3) for q in range(3)], notes
    assert [(got[i][0], got[i][1], got[i][2]) for i in (1, 4)] == [(1, 0, 2), (1, 1, 2)], notes
    assert ",grouped" in got[0][3] and ",global" in got[1][3], notes
    assert 0 < q1[0].batch_code_bytes() < 64 << 10, q1[0].batch_code_bytes()      # Q1 at K = 3: the descriptor folded
    # a lone Q1 beside the Q6s: nothing to share its scan with
    assert e.batch_jit_check([q1[0], q6[0], q6[1]])[0] == "alone: no other plan scans the same columns"
    e.close()
