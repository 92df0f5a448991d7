"""Wide sums in the GROUP BY tail and the per-operator folds (vdl_plan_set_wide_sums_tail; DESIGN.md section 5.17 "The tail") without a
GPU: the join of the two half sums against Python ints, argument checking and the getter, the switch in the environment, mode 0
clearing it, vdlrun's usage check, and vdl_plan_jit_check of a plan with a GROUP BY tail."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import mplan2vdl_amd as m
import wide_cases as wc
from mplan2vdl_amd import _lib, frontend
from test_scan_forms import declared_engine

sys.path.insert(0, os.path.join(wc.ROOT, "tests", "golden"))
import make_plan_goldens as mk  # noqa: E402

MASK = wc.MASK


def join(L, sl, sh):
    lo, hi = ctypes.c_int64(), ctypes.c_int64()
    assert L.vdl_wide_join_halves(sl, sh, ctypes.byref(lo), ctypes.byref(hi)) == _lib.VDL_OK
    return lo.value, hi.value


def words_of(x):
    """a Python int as the (lo, hi) signed words of its 128-bit two's complement"""
    x &= (1 << 128) - 1
    lo, hi = x & MASK, x >> 64
    return (lo - (1 << 64) if lo >> 63 else lo), (hi - (1 << 64) if hi >> 63 else hi)


def test_the_join_of_the_half_sums_against_python_ints():
    """sl = the sum of the terms' low 32 bits (0 .. 2^63 - 1 over 2^31 terms), sh = the sum of their arithmetic high halves
    (|sh| <= 2^62): lo, hi = the words of sh * 2^32 + sl"""
    L = _lib.load()
    r = np.random.default_rng(22)
    pairs = [(int(a), int(b)) for a, b in zip(r.integers(0, 1 << 63, 10000, dtype=np.int64), r.integers(-(1 << 62), 1 << 62, 10000, dtype=np.int64))]
    pairs += [(sl, sh) for sl in (0, (1 << 63) - 1) for sh in ((1 << 62) - 1, -((1 << 62) - 1), -(1 << 62), 0)]
    pairs += [((1 << 32) - 1, -1), (1 << 32, -1), (5, 1 << 31), (5, (1 << 31) - 1), (5, -(1 << 31)), (5, -(1 << 31) - 1)]      # where (sh << 32) crosses a word
    for sl, sh in pairs:
        assert join(L, sl, sh) == words_of((sh << 32) + sl), (sl, sh)
    # the split itself: any int64 term is H * 2^32 + L, and the join of one term's halves is the term with its sign extension
    for x in (wc.I64_MAX, wc.I64_MIN, -1, 0, wc.BIG, wc.NEG, (1 << 32) - 1, 1 << 32, -(1 << 32) - 1):
        assert join(L, x & 0xFFFFFFFF, x >> 32) == (x, x >> 63), x
    lo = ctypes.c_int64()
    assert L.vdl_wide_join_halves(1, 1, None, ctypes.byref(lo)) == _lib.VDL_ERR_ARG and L.vdl_wide_join_halves(1, 1, ctypes.byref(lo), None) == _lib.VDL_ERR_ARG


def test_arguments_and_the_getter():
    e = m.Engine(device=None)
    L = e._L
    p = e.parse(wc.GLOBAL)
    assert p.wide_sums_tail is False and L.vdl_plan_wide_sums_tail(p._h) == 0
    assert L.vdl_plan_set_wide_sums_tail(None, 1) == _lib.VDL_ERR_ARG and L.vdl_plan_wide_sums_tail(None) == 0
    p.set_wide_sums(1, tail=True)
    assert p.wide_sums == 1 and p.wide_sums_tail is True and p.wide_sums_sharded is False
    p.set_wide_sums(2)                                          # every call passes the switch down: a plain one switches it off again
    assert p.wide_sums == 2 and p.wide_sums_tail is False
    p.set_wide_sums(0, tail=True)                               # the switch says how a WIDE plan runs: it does not outlive mode 0
    assert p.wide_sums == 0 and p.wide_sums_tail is False
    dev, n = ctypes.POINTER(ctypes.c_int64)(), ctypes.c_size_t()
    assert L.vdl_output_high_device(p._h, 0, ctypes.byref(dev), ctypes.byref(n)) == _lib.VDL_ERR_ARG      # before a run there is no output 0
    assert L.vdl_output_high_device(None, 0, None, None) == _lib.VDL_ERR_ARG and L.vdl_output_high_device(p._h, -1, None, None) == _lib.VDL_ERR_ARG
    assert p.high_device() == {}
    e.close()


def test_mode_0_clears_the_switch():
    e = m.Engine(device=None)
    L = e._L
    p = e.parse(wc.GLOBAL)
    assert L.vdl_plan_set_wide_sums_tail(p._h, 1) == 0 and L.vdl_plan_wide_sums_tail(p._h) == 0      # in mode 0 there is nothing to switch ...
    assert L.vdl_plan_set_wide_sums(p._h, 1) == 0 and L.vdl_plan_wide_sums_tail(p._h) == 0          # ... and nothing waits for the mode
    assert L.vdl_plan_set_wide_sums(p._h, 2) == 0 and L.vdl_plan_set_wide_sums_tail(p._h, 1) == 0 and L.vdl_plan_wide_sums_tail(p._h) == 1
    assert L.vdl_plan_set_wide_sums(p._h, 1) == 0 and L.vdl_plan_wide_sums_tail(p._h) == 1          # (between the wide modes it stays)
    assert L.vdl_plan_set_wide_sums(p._h, 0) == 0 and L.vdl_plan_wide_sums_tail(p._h) == 0
    assert L.vdl_plan_set_wide_sums(p._h, 1) == 0 and L.vdl_plan_wide_sums_tail(p._h) == 0          # ... and does not come back with the mode
    e.close()


@pytest.mark.parametrize("wide,tail,want", [("1", "1", True), ("2", "1", True), ("1", "0", False), ("1", "yes", False), ("0", "1", False), (None, "1", False)])
def test_the_switch_in_the_environment_is_read_at_parse(wide, tail, want, monkeypatch):
    monkeypatch.delenv("VDL_WIDE_SUMS", raising=False)
    if wide is not None:
        monkeypatch.setenv("VDL_WIDE_SUMS", wide)
    monkeypatch.setenv("VDL_WIDE_TAIL", tail)
    e = m.Engine(device=None)
    p = e.parse(wc.GLOBAL)
    monkeypatch.delenv("VDL_WIDE_TAIL")
    monkeypatch.delenv("VDL_WIDE_SUMS", raising=False)
    assert p.wide_sums_tail is want
    assert e.parse(wc.GLOBAL).wide_sums_tail is False           # (read at parse, not later)
    e.close()


def test_vdlrun_wide_tail_needs_a_wide_mode(monkeypatch):
    monkeypatch.delenv("VDL_WIDE_SUMS", raising=False)
    exe = os.path.join(wc.ROOT, "mplan2vdl_amd", "bin", "vdlrun")
    out = subprocess.run([exe, "--wide-tail", "--describe"], input=wc.GLOBAL.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert out.returncode == 2 and out.stderr.decode().startswith("usage: vdlrun --wide-tail needs --wide-sums or --checked-sums"), out.stderr.decode()
    for mode in ("--wide-sums", "--checked-sums"):
        ok = subprocess.run([exe, mode, "--wide-tail", "--describe"], input=wc.GLOBAL.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert ok.returncode == 0, ok.stderr.decode()


def test_jit_check_of_a_plan_with_a_group_by_tail(tmp_path, monkeypatch):
    """Q3: with the tail switch on, jit_check builds the front and prelude units on a device-less context; they hold no sums, so no
    unit carries ,wide.  With it off the refusal stands."""
    d = tmp_path / "jit_cache"
    d.mkdir()
    os.chmod(d, 0o700)
    monkeypatch.setenv("VDL_JIT_CACHE", str(d))
    text, _, cols = mk.build(3, False, frontend.load_metadata(mk.META))
    e = declared_engine(cols)
    p = e.parse(text)
    assert not p.is_fused
    plain = p.jit_check()
    assert "front" in plain and ",wide" not in plain
    for mode in (1, 2):
        p.set_wide_sums(mode)
        with pytest.raises(m.VdlError) as err:
            p.jit_check()
        assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "GROUP BY tail" in str(err.value)
        p.set_wide_sums(mode, tail=True)
        note = p.jit_check()
        assert note == plain and ",wide" not in note and "not specialised" not in note, note
    e.close()
