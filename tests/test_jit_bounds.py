"""Filter bounds of the specialised scans at run time (Plan.set_jit(runtime_bounds=True)) on the GPU: plans over the same columns
that differ in the values of their bounds share one kernel, each with its own descriptor, and every answer is the oracle's, bit
for bit.

Every case pins one form (VDL_JIT_PIN; VDL_JIT_ASSUME_SELECTIVITY pins which columns it reads late) at the smallest row counts at
which its tile logic branches, and runs a list of variants of a program -- the program with the constants of its range filters
replaced -- each as a new plan on one engine.  After the first variant of a shape (which sides of a range are open, whether it is
a point; a bound at or beyond the end of an image counts as absent) the later ones compile nothing and read nothing from the
code-object cache; the first plan run again after the others gives its own answer again; with the bounds as constants (the
default) the answers are the same.

The variants of the edge table's programs (test_scan_forms.py) put bounds inside the images, one step inside and outside each end
of an image (clamping), past what an image's width holds, and make a range empty in the image's domain ([1, 0] in the descriptor:
a range between two steps of an affine image, or past the width; a range with lo > hi in the text never reaches a kernel) -- also on
`mn`, whose image starts at INT64_MIN."""
import os
import re

import pytest

import mplan2vdl_amd as m
import test_scan_forms as F
from helpers import oracle_run
from test_jit_bounds_cpu import CHANGES, changed
from test_scan_forms import B, I64MIN, M4

pytestmark = pytest.mark.gpu

# (u, late): eager, staged with one / two / all filter columns with the tile, the queue form; the packed forms (filters packed and the
# aggregate inputs late; every column packed) for the global scans over table columns
FORMS = [(2, 0), (2, 1), (3, 2), (2, 4), (4, 3)]
PACKED = [(2, 5), (2, 6)]
SUFFIX = {**F.SUFFIX, 5: ",packed,late", 6: ",packed"}
HAS_PACKED = ("edge_global", "q6")

# ---- the variants: [(mapping of the base text's RangeV constants, same shape as the one before)] ---------------------------------
# edge_global, bound set 0: p1 in [-127, 126] (pure 1-byte image, [-128, 127]), a1 in [B + 500, B + 126000] (B + 1000 e, e in
# [0, 127], 1 byte), w4 <= M4 - 2^30 (4 bytes, e' up to 2^31 - 1)
P1, A1, W4 = (-127, 126), (B + 500, B + 126000), M4 - 2**30


def g0(p1=P1, a1=A1, w4=W4):
    return {P1[0]: p1[0], P1[1]: p1[1], A1[0]: a1[0], A1[1]: a1[1], W4: w4}


# edge_global, bound set 1: p1 in [-129, 126], a1 in [B - 1, B + 126999], mn in [INT64_MIN, INT64_MIN + 1000 * 29999]
# (INT64_MIN + 1000 k, k in [0, 30000], a 2-byte image)
MN_HI = I64MIN + 1000 * 29999


def g1(lo=I64MIN, hi=MN_HI):
    return {I64MIN: lo, MN_HI: hi}


# edge_group: a1 in [B + 3000, B + 124000], w4 >= M4 - 2^30
def gg(a1=(B + 3000, B + 124000), w4=M4 - 2**30):
    return {B + 3000: a1[0], B + 124000: a1[1], M4 - 2**30: w4}


VARIANTS = {
    "edge_global": [
        (g0(), False),                                                              # one step inside p1's ends
        (g0(p1=(-100, 100), a1=(B + 10500, B + 100000), w4=M4 - 2**29), True),       # interior
        (g0(p1=(-90, 110), a1=(B + 20500, B + 110999), w4=M4 - 2**30 - 12345), True),   # shifted
        (g0(p1=(-127, 126), a1=(B + 1, B + 126999), w4=M4 - 1), True),               # one step inside every end
        (g0(p1=(-129, 128), a1=(B - 1000, B + 128000), w4=M4 + 1), False),           # one step outside every end: clamped
        (g0(p1=(200, 300)), False),                                                 # empty: past the 1-byte image ([1, 0] in the descriptor)
        (g0(a1=(B + 1, B + 999)), False),                                           # empty: between two steps of the scale-1000 image
        (g0(p1=(-100000, 100000), a1=(B - 10**9, B + 10**12), w4=M4), False),        # past what the widths hold, both sides
        (g0(p1=(-300, 5), a1=(B + 64000, B + 10**12)), False),                       # ... one side each
    ],
    "edge_global_mn": [
        (g1(), False),
        (g1(hi=I64MIN + 1000 * 15000 + 999), True),                                 # interior, between two steps
        (g1(lo=I64MIN + 1000, hi=I64MIN + 1000 * 29999), False),                     # one step inside each end
        (g1(lo=I64MIN + 1001, hi=I64MIN + 1000 * 20000), True),                      # shifted
        (g1(lo=I64MIN + 1, hi=I64MIN + 1000 * 30001), False),                        # past the upper end: clamped
        (g1(lo=I64MIN + 4001, hi=I64MIN + 4999), False),                             # empty: between two steps
    ],
    "edge_group": [
        (gg(), False),
        (gg(a1=(B + 13000, B + 100999), w4=M4 - 2**29), True),
        (gg(a1=(B + 1000, B + 126000), w4=M4 - (2**31 - 1) + 1), True),              # one step inside every end
        (gg(a1=(B - 1, B + 127001), w4=M4 - (2**31 - 1) - 1), False),                # one step outside: clamped
        (gg(a1=(B + 50001, B + 50999)), False),                                     # empty: between two steps
    ],
}
for _q in ("q6", "q1", "q14", "q19", "q12"):
    VARIANTS[_q] = [({}, False), (CHANGES[_q], True)]
BASE = {"edge_global_mn": "edge_global"}


def rows_of(u, late):
    return [2049, 37 * 2048 + 511] if late >= 5 else [F.tile(u) + 1, 37 * F.tile(u) + 511]


_programs, _want = {}, {}


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one code-object cache for the module: a form compiles once across row counts (the cache is keyed by the source)"""
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


def base_program(name, n):
    """(text, columns) of the program the variants of `name` start from, its fact table at n rows"""
    if (name, n) not in _programs:
        base = BASE.get(name, name)
        if base in F.EDGE:
            text, cols = F.program(base, n)
            if name == "edge_global_mn":
                text = F.edge_global(1)
        else:
            full_text, full_cols = F.program(base)
            text, cols = full_text, F.sliced(full_cols, n, F.passing_row(base, full_text, full_cols))
        _programs[(name, n)] = (text, cols)
    return _programs[(name, n)]


def wanted(name, n, k, text, cols):
    """the oracle's answer for variant k, computed once and shared by the forms"""
    if (name, n, k) not in _want:
        _want[(name, n, k)] = oracle_run(text, cols)
    return _want[(name, n, k)]


def built():
    c = m.jit_counters()
    return c["compiled"] + c["from_disk"]


def run(e, text, runtime_bounds, tune=True, keep=False):
    p = e.parse(text)
    p.set_jit(True, tune=tune, runtime_bounds=runtime_bounds)
    res = p.run()["results"]
    note = p.jit_note()
    if keep:
        return res, note, p
    p.close()
    return res, note


def check_note(name, u, late, note, runtime_bounds):
    """the tuner ran the pinned form (its name carries ",rtb" with the bounds at run time), or the scan does not have it"""
    why = None if late >= 5 else F.expected_refusal(BASE.get(name, name), u, late, True)
    chosen = re.findall(r"scan 0 tuned:[^;]*-> (k_mscan_specialised<\d+,(\d+),[^>]*>)", note)
    if why:
        assert "tuned:" not in note, (name, u, late, why, note)
        return
    assert len(chosen) == 1 and int(chosen[0][1]) == u, (name, u, late, note)
    assert chosen[0][0].endswith(SUFFIX[late] + (",rtb>" if runtime_bounds else ">")), (name, u, late, note)
    assert (",rtb" in note) == runtime_bounds, note


CASES = [(name, f) for name in VARIANTS for f in FORMS + (PACKED if BASE.get(name, name) in HAS_PACKED else [])]


@pytest.mark.parametrize("name,form", CASES, ids=["%s-u%d%s" % (n, f[0], SUFFIX[f[1]].replace(",", "_") or "_eager") for n, f in CASES])
def test_plans_share_code_and_keep_their_own_bounds(name, form, jit_cache, monkeypatch):
    u, late = form
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % (u, late))
    monkeypatch.setenv("VDL_JIT_ASSUME_SELECTIVITY", "0.3")
    for n in rows_of(u, late):
        base_text, cols = base_program(name, n)
        e = F.gpu_engine(cols, True)
        first = None
        for k, (mapping, same_shape) in enumerate(VARIANTS[name]):
            text = changed(base_text, mapping)
            want = wanted(name, n, k, text, cols)
            before = built()
            got, note, plan = run(e, text, True, keep=True)
            added = built() - before
            assert got == want, (name, n, u, late, k, note)
            check_note(name, u, late, note, True)
            # the first variant of a shape may compile (at the first row count: later ones find the module's cache); no other does
            assert added == 0 or not same_shape, (name, n, u, late, k, added, note)
            if first is None:
                first = (plan, want)
            else:
                plan.close()
            constant, cnote = run(e, text, False)               # the bounds as constants: the same answer
            assert constant == want, (name, n, u, late, k, cnote)
            check_note(name, u, late, cnote, False)
        # the variants once more: every shape has been built; and plan A after all the others still answers for its own bounds
        before = built()
        for k, (mapping, _) in reversed(list(enumerate(VARIANTS[name]))):
            got, note = run(e, changed(base_text, mapping), True)
            assert got == _want[(name, n, k)], (name, n, u, late, k, note)
        assert built() == before, (name, n, u, late)
        plan, want = first
        assert plan.run()["results"] == want, (name, n, u, late)
        assert built() == before
        plan.close()
        e.close()


@pytest.mark.parametrize("query", ["q6", "q1"])
def test_a_second_literal_set_tunes_without_compiling(query, jit_cache, monkeypatch):
    """the tuner's whole candidate list over 37 tiles of 1024 rows and 511: plan B's tuning run builds nothing, and both match the oracle"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    monkeypatch.setenv("VDL_JIT_ASSUME_SELECTIVITY", "0.3")    # (which columns a form reads late does not depend on the literals)
    n = 37 * 1024 + 511
    text_a, cols = base_program(query, n)
    text_b = changed(text_a, CHANGES[query])
    e = F.gpu_engine(cols, True)
    got_a, note_a, plan_a = run(e, text_a, True, keep=True)
    assert got_a == oracle_run(text_a, cols) and "scan 0 tuned:" in note_a and ",rtb>" in note_a, note_a
    # (the tuner's staged candidate {0, 1} runs at the quickest eager u, which timing decides: A builds it at every eager u)
    for u in (4, 6):
        monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=1" % u)
        assert run(e, text_a, True)[0] == got_a
    monkeypatch.delenv("VDL_JIT_PIN")
    before = built()
    got_b, note_b = run(e, text_b, True)
    assert built() == before, (m.jit_counters(), note_b)
    assert got_b == oracle_run(text_b, cols) and "scan 0 tuned:" in note_b, note_b
    assert re.search(r"from cache: (\d+) of \1 builds of scan 0; $", note_b), note_b
    assert plan_a.run()["results"] == got_a
    plan_a.close()
    e.close()


def test_q3_front_and_dimension_scans_share_code(jit_cache, monkeypatch):
    """Q3 -- the one-pass front, its dimension scans, ORDER BY revenue desc, o_orderdate LIMIT 10 on the device -- for another date, and
    for another date and another market segment: nothing compiles, each plan's answer is the oracle's in that order"""
    import numpy as np
    import test_jit as J
    from test_order import DATE, REV, columns, expected
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    text_a, cols = J.compiled(3, 2e-3)
    date_only = {k: v for k, v in CHANGES["q3"].items() if k > 1000}
    text_b = changed(text_a, date_only)
    e = F.gpu_engine(cols, True)
    plans, before = [], None
    for text in (text_a, text_b, changed(text_a, CHANGES["q3"])):
        p = e.parse(text)
        p.set_jit(True, runtime_bounds=True)
        p.set_order([(REV, True), (DATE, False)], limit=10)
        res = p.run(as_numpy=True)
        note = p.jit_note()
        assert "front: vdl_jit_project_front<" in note and ",rtb>" in note and "not specialised" not in note, note
        want, _ = expected(oracle_run(text, cols), [(REV, True), (DATE, False)], 10)
        _, _, got = columns(res["results"])
        assert list(got) == list(want) and all(np.array_equal(got[t], want[t]) for t in want), note
        if before is not None:
            assert built() == before, (m.jit_counters(), note)
            assert re.search(r"from cache: 1 of 1 builds of front; ", note), note
        before = built()
        plans.append((p, got))
    p, got = plans[0]                                           # A after B: its own segment and date again
    _, _, again = columns(p.run(as_numpy=True)["results"])
    assert all(np.array_equal(again[t], got[t]) for t in got)
    plain = e.parse(text_b)                                     # B with the bounds as constants
    plain.set_jit(True)
    plain.set_order([(REV, True), (DATE, False)], limit=10)
    _, _, const = columns(plain.run(as_numpy=True)["results"])
    assert all(np.array_equal(const[t], plans[1][1][t]) for t in const)
    e.close()
