"""Wide sums (vdl_plan_set_wide_sums) without a GPU: argument checking, the switch in the environment, the
wide units built by hiprtc, the generated source and its cache key with the switch off, and the 128-bit operators of the scalar
expressions against Python ints."""
import ctypes
import glob
import os

import pytest

import mplan2vdl_amd as m
import wide_cases as wc
from mplan2vdl_amd import _lib
from mplan2vdl_amd.engine import jit_counters
from test_scan_forms import declared_engine, tpch


@pytest.fixture
def fresh_cache(tmp_path, monkeypatch):
    d = tmp_path / "jit_cache"
    d.mkdir()
    os.chmod(d, 0o700)
    monkeypatch.setenv("VDL_JIT_CACHE", str(d))
    for k in ("VDL_JIT_U", "VDL_JIT_LATE", "VDL_JIT_PIN", "VDL_WIDE_SUMS"):
        monkeypatch.delenv(k, raising=False)
    return d


def test_arguments_and_outputs_before_a_run():
    e = m.Engine(device=None)
    L = e._L
    p = e.parse(wc.GLOBAL)
    assert p.wide_sums == 0 and p.wide_note() == ""
    for bad in (-1, 3, 100):
        assert L.vdl_plan_set_wide_sums(p._h, bad) == _lib.VDL_ERR_ARG
        with pytest.raises(m.VdlError):
            p.set_wide_sums(bad)
    assert L.vdl_plan_set_wide_sums(None, 1) == _lib.VDL_ERR_ARG
    for mode in (1, 2, 0):
        p.set_wide_sums(mode)
        assert p.wide_sums == mode
    hi, n = ctypes.POINTER(ctypes.c_int64)(), ctypes.c_size_t()
    assert L.vdl_output_high(p._h, 0, ctypes.byref(hi), ctypes.byref(n)) == _lib.VDL_ERR_ARG      # before a run there is no output 0
    assert L.vdl_output_high(p._h, -1, None, None) == _lib.VDL_ERR_ARG and L.vdl_output_high(None, 0, None, None) == _lib.VDL_ERR_ARG
    assert p.collect_words() == {}
    assert _lib.VDL_ERR_OVERFLOW == 8
    e.close()


@pytest.mark.parametrize("value,mode", [("1", 1), ("2", 2), ("0", 0), ("3", 0), ("yes", 0), ("", 0)])
def test_the_switch_in_the_environment_is_read_at_parse(value, mode, monkeypatch):
    monkeypatch.setenv("VDL_WIDE_SUMS", value)
    e = m.Engine(device=None)
    p = e.parse(wc.GLOBAL)
    monkeypatch.delenv("VDL_WIDE_SUMS")
    assert p.wide_sums == mode
    assert e.parse(wc.GLOBAL).wide_sums == 0                   # (read at parse, not later)
    e.close()


@pytest.mark.parametrize("name", ["q6", "q1", "q14"])
def test_jit_check_builds_the_wide_units_without_a_device(name, fresh_cache):
    text, cols = tpch(name)
    e = declared_engine(cols)
    p = e.parse(text)
    plain = p.jit_check()
    assert ",wide" not in plain
    for mode in (1, 2):
        p.set_wide_sums(mode)
        note = p.jit_check()
        assert note.count(",wide>") == note.count("B of code") >= 1 and "not specialised" not in note, note      # the kernel name carries ,wide in modes 1 and 2
    p.set_wide_sums(0)
    assert p.jit_check() == plain
    e.close()


def test_mode_0_generates_the_source_and_the_key_of_a_plan_that_never_had_it_set(fresh_cache, tmp_path, monkeypatch):
    dump = tmp_path / "dump"
    dump.mkdir()
    monkeypatch.setenv("VDL_JIT_DUMP", str(dump))
    text, cols = wc.GROUPED, wc.grouped_cols(100)             # (a program no other test of this process builds: the counters below are its own)
    e = declared_engine(cols)
    never = e.parse(text)
    before = jit_counters()
    note = never.jit_check()
    built = jit_counters()
    assert built["compiled"] + built["from_disk"] == before["compiled"] + before["from_disk"] + 1
    units = set(glob.glob(str(dump / "*.hip")))
    assert len(units) == 1 and "#define VDL_WIDE" not in open(next(iter(units))).read().split("namespace vdl")[0]
    back = e.parse(text)
    back.set_wide_sums(1)
    back.set_wide_sums(0)
    assert back.jit_check() == note                            # the same kernel name ...
    again = jit_counters()
    # ... from the same source under the same key: found in memory, nothing compiled, no new unit dumped
    assert again["from_memory"] == built["from_memory"] + 1 and again["compiled"] == built["compiled"] and again["from_disk"] == built["from_disk"]
    assert set(glob.glob(str(dump / "*.hip"))) == units
    back.set_wide_sums(1)
    wide = back.jit_check()
    after = jit_counters()
    assert after["compiled"] == again["compiled"] + 1 and ",wide>" in wide and ",wide" not in note
    new = set(glob.glob(str(dump / "*.hip"))) - units
    assert len(new) == 1 and open(next(iter(new))).read().startswith("#define VDL_SPEC_UNROLL") and "#define VDL_WIDE 1\n" in open(next(iter(new))).read()[:400]
    e.close()


def test_jit_check_refuses_a_plan_whose_sums_are_not_the_scans(fresh_cache):
    e = m.Engine(device=None)
    p = e.parse(open(os.path.join(wc.ROOT, "tests", "golden", "q3.vdl")).read())
    p.set_wide_sums(1)
    with pytest.raises(m.VdlError) as err:
        p.jit_check()
    assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "GROUP BY tail" in str(err.value)
    e.close()


# ---- the 128-bit operators of the scalar expressions (vdl_wide_eval_bin: host only) ------------------------------------------------------
M128 = (1 << 128) - 1
ADD, SUB, MUL, DIV, MOD, SHIFT, GT, EQ = 6, 7, 9, 10, 11, 4, 8, 5


def signed128(x):
    x &= M128
    return x - (1 << 128) if x >> 127 else x


def model(op, a, b):
    """the int64 rules of DESIGN.md section 2, widened, on Python ints"""
    if op == ADD:
        return signed128(a + b)
    if op == SUB:
        return signed128(a - b)
    if op == MUL:
        return signed128(a * b)
    if op == DIV:
        if b == 0:
            return 0
        q = abs(a) // abs(b)
        return signed128(q if (a < 0) == (b < 0) else -q)      # truncation towards zero; MIN128 / -1 wraps
    if op == MOD:
        if b in (0, -1):
            return 0
        r = abs(a) % abs(b)
        return -r if a < 0 else r                              # the sign of the dividend
    if op == SHIFT:
        return a >> min(b, 127) if b >= 0 else (0 if b <= -128 else signed128(a << -b))
    return int(a > b) if op == GT else int(a == b)


def eval_bin(L, op, a, b):
    lo, hi = ctypes.c_int64(), ctypes.c_int64()
    split = lambda x: (ctypes.c_int64(signed64(x & wc.MASK)), ctypes.c_int64(signed64((x >> 64) & wc.MASK)))      # noqa: E731
    (alo, ahi), (blo, bhi) = split(a), split(b)
    assert L.vdl_wide_eval_bin(op, alo, ahi, blo, bhi, ctypes.byref(lo), ctypes.byref(hi)) == _lib.VDL_OK
    return (hi.value << 64) | (lo.value & wc.MASK)


def signed64(x):
    return x - (1 << 64) if x >> 63 else x


EDGES = [0, 1, -1, 2, -2, 7, -7, 100, wc.I64_MAX, wc.I64_MIN, wc.I64_MAX + 1, wc.I64_MIN - 1, (1 << 64) - 1, 1 << 64, -(1 << 64), 3 * wc.BIG, 3 * wc.NEG,
         (1 << 127) - 1, -(1 << 127), -(1 << 127) + 1, (1 << 126) + 12345, 127, 128, -127, -128, 63, 64]


@pytest.mark.parametrize("op", [ADD, SUB, MUL, DIV, MOD, SHIFT, GT, EQ], ids=["Add", "Subtract", "Multiply", "Divide", "Modulo", "BitShift", "Greater", "Equals"])
def test_the_128_bit_operators_against_python_ints(op):
    L = _lib.load()
    for a in EDGES:
        for b in EDGES:
            assert eval_bin(L, op, a, b) == model(op, a, b), (op, a, b)
    lo, hi = ctypes.c_int64(), ctypes.c_int64()
    assert L.vdl_wide_eval_bin(12, 0, 0, 0, 0, ctypes.byref(lo), ctypes.byref(hi)) == _lib.VDL_ERR_ARG
    assert L.vdl_wide_eval_bin(ADD, 0, 0, 0, 0, None, None) == _lib.VDL_ERR_ARG
