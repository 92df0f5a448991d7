"""The ends of int64 without a GPU: the Python model of the operators (tests/vdl_model.py) against the CPU oracle on the directed
edge programs (tests/int64_edge_cases.py) and on random programs over pool columns; the oracle's Partition under ASan + UBSan in
a stand-alone program; and the planner's form of a column-against-column comparison, which stays a fused range of the difference
whose bound scan takes the saturated difference where an operand is 8 bytes wide."""
import os
import subprocess

import numpy as np
import pytest

import int64_edge_cases as cases
import mplan2vdl_amd as m
import vdl_model as model
from conftest import ROOT
from helpers import oracle_run, prog
from test_random_programs import Gen
from vdl_model import I64_MAX, I64_MIN


def same(name, text, cols, got, want):
    """exact equality of two result dicts, with the program, the columns and the first differing slot on a mismatch"""
    if got == want:
        return
    for key in sorted(set(got) | set(want), key=lambda k: int(k[3:])):
        a, b = got.get(key), want.get(key)
        if a == b:
            continue
        va, vb = (list(a.values())[0] if a else None), (list(b.values())[0] if b else None)
        at = next((i for i, (x, y) in enumerate(zip(va or [], vb or [])) if x != y), min(len(va or []), len(vb or [])))
        line = [ln for ln in text.splitlines() if ln.startswith(key[3:] + ",")]
        raise AssertionError("%s: output %s %s differs at slot %d: oracle %s (%d values), model %s (%d values)\ncolumns: %s\n%s" % (
            name, key, line, at, (va or [None] * (at + 1))[at:at + 4], len(va or []), (vb or [None] * (at + 1))[at:at + 4], len(vb or []),
            {k: (str(v.dtype), len(v), v[:8].tolist()) for k, v in cols.items()}, text))


def test_model_pins():
    """the model's own arithmetic at the points where a restatement could go wrong"""
    B = model.BINARY
    assert model.wrap(1 << 63) == I64_MIN and model.wrap(-(1 << 63) - 1) == I64_MAX and model.wrap((1 << 64) + 5) == 5
    assert B["Divide"](I64_MIN, -1) == I64_MIN and B["Divide"](7, 0) == 0 and B["Divide"](-7, 2) == -3 and B["Divide"](7, -2) == -3
    assert B["Modulo"](I64_MIN, -1) == 0 and B["Modulo"](5, 0) == 0 and B["Modulo"](-7, 2) == -1 and B["Modulo"](7, -2) == 1
    assert B["Modulo"](I64_MIN, 3) == -2 and B["Divide"](I64_MIN, I64_MAX) == -1 and B["Modulo"](I64_MIN, I64_MAX) == -1
    assert B["BitShift"](-8, 1) == -4 and B["BitShift"](-1, 64) == -1 and B["BitShift"](I64_MIN, I64_MAX) == -1 and B["BitShift"](I64_MAX, 65) == 0
    assert B["BitShift"](1, -63) == I64_MIN and B["BitShift"](1, -64) == 0 and B["BitShift"](3, -62) == -(1 << 62) and B["BitShift"](-1, I64_MIN) == 0
    assert B["Add"](I64_MAX, 1) == I64_MIN and B["Subtract"](I64_MIN, 1) == I64_MAX and B["Multiply"](I64_MIN, -1) == I64_MIN
    assert B["Multiply"](1 << 62, 4) == 0 and B["Greater"](I64_MAX, -1) == 1 and B["Greater"](I64_MIN, 1) == 0
    v = model.rangev(I64_MAX - 1, model.Vec([0, 0, 0, 0]), 1)
    assert v.vals == [I64_MAX - 1, I64_MAX, I64_MIN, I64_MIN + 1]
    piv = model.rangec(-5, 10, 1)
    assert [model.bucket(x, piv) for x in (I64_MIN, -5, -4, 4, 5, 6, I64_MAX)] == [0, 0, 1, 9, 10, 10, 10]
    assert model.bucket(I64_MAX, model.rangec(I64_MIN, 1 << 62, 1)) == 1 << 62
    assert len(model.POOL) == 31 and model.POOL[0] == I64_MIN and model.POOL[-1] == I64_MAX


PARTITION_CASES = [([5, I64_MAX, 9, -100, 1000, I64_MAX - 1], -5, 10, [1, 2, 3, 0, 4, 5]),                  # the counting sort
                   ([5, I64_MAX, 9, I64_MIN, 1000], -5, 1 << 30, [1, 4, 2, 0, 3])]                          # the sort of (bucket, slot) pairs


@pytest.mark.parametrize("data,pmin,count,want", PARTITION_CASES)
def test_partition_clamps_a_wrapped_difference_to_the_overflow_bucket(data, pmin, count, want):
    """x - pmin of 2^63 and more wraps negative: once returned as the bucket (an index before the counting table)"""
    cols = {"t.x": np.array(data, np.int64)}
    text = prog("1,Load,t.x", "2,Project,val,Id 1,x", "3,RangeC,val,%d,%d,1" % (pmin, count), "4,Partition,val,Id 2,val,Id 3,val", "5,MaterializeCompact,Id 4")
    assert model.run(text, cols) == {"tmp5": {".val": want}}
    assert oracle_run(text, cols) == {"tmp5": {".val": want}}


def _build_partition_checker(tmp_path, sanitize):
    """(path or None, the compiler's messages)"""
    exe = str(tmp_path / ("oracle_partition" + ("_asan" if sanitize else "")))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    cmd = ["gcc", "-std=c11", "-fopenmp", "-Wall"] + flags + [os.path.join(ROOT, "tools", "sanitize", "oracle_partition_main.c"), "-o", exe, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return (exe if r.returncode == 0 else None), r.stdout + r.stderr


def test_oracle_partition_is_clean_under_sanitizers(tmp_path):
    import re

    exe, said = _build_partition_checker(tmp_path, True)
    build = "ASan + UBSan"
    if not exe:
        # only a compiler without the sanitizers' runtime libraries may fall back to the plain build (which still checks the
        # values); anything else it says about the sanitized build is a failure of this test
        assert re.search(r"cannot find .*(asan|ubsan)|lib(asan|ubsan)[^\n]*(No such file|not found)|unrecognized .*-fsanitize", said), said[-3000:]
        exe, said = _build_partition_checker(tmp_path, False)
        build = "plain (no sanitizer runtimes on this machine)"
    assert exe, "tools/sanitize/oracle_partition_main.c does not build:\n" + said[-3000:]
    print("oracle_partition_main.c build:", build)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), build + "\n" + r.stdout[-3000:] + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) >= 100


def test_oracle_equals_the_model_on_the_directed_programs():
    count = 0
    for name, text, cols in cases.directed_programs(sizes=(1, 65)):
        same(name, text, cols, oracle_run(text, cols), model.run(text, cols))
        count += 1
    assert count > 100


def test_scatter_lets_the_later_of_two_slots_win():
    """(CPU only: the engine takes Scatter positions to be unique, as every call site of the compiler makes them)"""
    cols = {"t.x": np.array([10, 20, 30, 40, 50], np.int64), "t.p": np.array([1, 1, -1, 5, 1], np.int64)}
    text = prog("1,Load,t.x", "2,Project,val,Id 1,x", "3,Load,t.p", "4,Project,val,Id 3,p", "5,Scatter,Id 2,Id 2,val,Id 4,val", "6,MaterializeCompact,Id 5")
    assert model.run(text, cols) == oracle_run(text, cols) == {"tmp6": {".val": [50]}}


def pool_program(seed, steps):
    """a program of test_random_programs.Gen with every column replaced by draws from the pool (positions: the FK column too)"""
    g = Gen(seed)
    rng = np.random.default_rng(1000 + seed)
    for k, v in list(g.cols.items()):
        g.cols[k] = model.pool_column(rng, len(v), v.dtype.type)
    if seed % 2:                                                     # every other seed: positions that hit the dimension table as well
        g.cols["t.fk"] = cases.position_column(rng, g.n["u"], g.n["t"])
    return g.build(steps)


def test_oracle_equals_the_model_on_random_programs_over_the_pool():
    for seed in range(32):
        text, cols = pool_program(seed, 10 + seed % 30)
        same("pool_program seed %d" % seed, text, cols, oracle_run(text, cols), model.run(text, cols))


# ---- the planner: a > b over two columns ------------------------------------------------------------------------------------------
def declared(cols):
    e = m.Engine(device=None)
    for k, v in cols.items():
        e.register_pointer(k, 0x10000, v.dtype.itemsize, len(v))
    return e


def code_bytes(note):
    import re
    return [int(x) for x in re.findall(r"(\d+) B of code", note)]


@pytest.mark.parametrize("form,planned", [("gt", "col 3 col0 - col1 in [1,+inf]"), ("lt", "col 3 col0 - col1 in [1,+inf]"), ("ge", "col 3 col0 - col1 in [0,+inf]")])
def test_a_comparison_of_two_columns_stays_a_fused_range_of_their_difference(form, planned, tmp_path, monkeypatch):
    """int32 against int32 (TPC-H Q4 / Q12 compare dates so): the wrap-around difference cannot wrap, the plan and its specialised
    scan are what they were.  With an 8-byte operand the plan is the same and the bound scan takes the saturated difference:
    other code (a few instructions more), built from the same plan."""
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    text, cols = cases.compare_scan(100, "i32", form)
    first, second = ("t.b", "t.a") if form == "lt" else ("t.a", "t.b")
    sizes = {}
    for wide in ((), ("t.b",), ("t.a", "t.b")):
        e = declared({k: v.astype(np.int64 if k in wide else v.dtype.type) for k, v in cols.items()})
        p = e.parse(text)
        assert p.is_fused and "  col 0 %s\n  col 1 %s\n  col 2 t.x\n  %s\n" % (first, second, planned) in p.describe(), p.describe()
        note = p.jit_check()
        assert "k_mscan_specialised<4,4,vec,global,derived>" in note, note
        sizes[wide] = code_bytes(note)[0]
        e.close()
    assert all(sizes[w] > sizes[()] for w in sizes if w), sizes


def test_a_subtract_of_the_program_keeps_its_wrap_around_value(tmp_path, monkeypatch):
    """Greater(Subtract(a, b), 0) means the sign of the wrapped difference: the same scan over narrow and over wide columns, and a
    column of its own beside the one a comparison of a and b makes"""
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    sizes = []
    for dt in (np.int32, np.int64):
        p_ = cases.Prog()
        rng = np.random.default_rng(5)
        a, b = p_.load("t.a", model.pool_column(rng, 100, dt)), p_.load("t.b", model.pool_column(rng, 100, dt))
        x = p_.load("t.x", model.pool_column(rng, 100))
        cond = p_.bin("LogicalAnd", p_.bin("Greater", p_.bin("Subtract", a, b), p_.const(0, a)), p_.ge(a, b))
        fx = p_.gather(x, p_.select(cond))
        p_.out(p_.fold("FoldSum", p_.const(0, fx), fx))
        text, cols = p_.done()
        e = declared(cols)
        p = e.parse(text)
        assert p.is_fused and "col0 - col1 in [1,+inf]" in p.describe() and "col0 - col1 in [0,+inf]" in p.describe(), p.describe()
        sizes.append(code_bytes(p.jit_check())[0])
        e.close()
    assert sizes[1] > sizes[0], sizes


def test_a_fused_front_reads_the_comparison_the_same_way(tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    sizes = []
    for width in ("i32", "i64"):
        text, cols = cases.compare_front(300, width)
        e = declared(cols)
        p = e.parse(text)
        assert not p.is_fused and "fused front" in p.describe() and "col 4 col0 - col1 in [1,+inf]" in p.describe(), p.describe()
        sizes.append(code_bytes(p.jit_check())[0])
        e.close()
    assert sizes[1] > sizes[0], sizes


def test_a_dimension_scan_keeps_the_planned_form():
    """(its columns are bound when the plan runs: what it computes over wide columns is the GPU test's to see)"""
    for width in ("i32", "i64"):
        text, cols = cases.compare_dimension(300, width)
        e = declared(cols)
        p = e.parse(text)
        assert p.is_fused and "prelude 0: bitmap of the dimension-side selection" in p.describe() and "  col 2 col0 - col1 in [1,+inf]\nscan 0 table=t" in p.describe(), p.describe()
        e.close()
