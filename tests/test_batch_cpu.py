"""Batched runs (vdl_run_batch, Engine.run_batch) without a GPU: vdl_batch_jit_check groups plans over declared columns, builds
the batch kernels for gfx950 by hiprtc and fills the notes (Plan.batch_note), so the grouping rules, the cut of a group into
batches and the builds are checked here; the answers are checked on the device (test_batch.py).

Q6's literal sets shift the date, discount and quantity constants and keep every range's shape; a plan with specialisation off, a
grouped plan (Q1) and a Q6 whose date range has lost its lower bound (another shape) run alone beside them, each with its reason."""
import os
import re
import subprocess

import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib
from conftest import ROOT, golden
from test_jit_bounds_cpu import SHAPES, changed, program

VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
NOTE = re.compile(r"^batch (\d+): slot (\d+) of (\d+), (k_mscan_specialised<[^>]*,batch(\d+),rtb>)$")


def literal_set(k):
    """Q6's constants shifted by k steps inside the columns' domains: the year's two ends, the discount's centre, the quantity's limit"""
    return {728294: 728294 + 30 * k, 728659: 728659 + 30 * k, 6: 2 + k % 7, 24: 24 + k}


def q6_plans(e, text, count, jit=True):
    plans = [e.parse(changed(text, literal_set(k))) for k in range(count)]
    for p in plans:
        p.set_jit(jit)
    return plans


def slots(notes):
    """[(batch, slot, width, kernel)] of the notes of batched plans; every name carries its batch's width"""
    out = []
    for note in notes:
        mo = NOTE.match(note)
        assert mo, note
        assert mo.group(3) == mo.group(5), note
        out.append((int(mo.group(1)), int(mo.group(2)), int(mo.group(3)), mo.group(4)))
    return out


@pytest.fixture
def q6(tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    text, e = program("q6")
    yield text, e
    e.close()


@pytest.mark.parametrize("width", [2, 8])
def test_q6_literal_sets_build_as_one_batch(q6, width):
    text, e = q6
    plans = q6_plans(e, text, width)
    before = m.jit_counters()["compiled"]
    notes = e.batch_jit_check(plans)
    assert notes == [p.batch_note() for p in plans]
    got = slots(notes)
    assert [(b, q, k) for b, q, k, _ in got] == [(0, q, width) for q in range(width)], notes
    assert len({name for _, _, _, name in got}) == 1
    assert m.jit_counters()["compiled"] == before + 1           # one code object for the batch, whatever its literals
    again = q6_plans(e, text, width)[::-1]                      # other plans, other order: nothing compiles
    assert slots(e.batch_jit_check(again)) == got
    assert m.jit_counters()["compiled"] == before + 1


def test_the_packed_form_builds_when_pinned(tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("VDL_JIT_PIN", "u=2,late=6")
    text, e = program("q6_packed")
    plans = [e.parse(changed(text, literal_set(k))) for k in range(3)]
    for p in plans:
        p.set_jit(True, tune=True)
    got = slots(e.batch_jit_check(plans))
    assert [(b, q, k) for b, q, k, _ in got] == [(0, 0, 3), (0, 1, 3), (0, 2, 3)]
    assert got[0][3].startswith("k_mscan_specialised<4,2,") and ",packed,batch3,rtb>" in got[0][3], got
    e.close()


def test_plans_that_cannot_share_run_alone_with_their_reason(q6):
    text, e = q6
    import test_jit as J
    q1_text, q1_cols = J.compiled(1, 1e-4)
    for k, v in q1_cols.items():
        if k not in ("lineitem.l_shipdate", "lineitem.l_discount", "lineitem.l_quantity", "lineitem.l_extendedprice"):
            e.register_pointer(k, 0x10000, v.dtype.itemsize, 600000)
    a, b = q6_plans(e, text, 2)
    q1 = e.parse(q1_text)
    q1.set_jit(True)
    off = q6_plans(e, text, 3, jit=False)[2]
    one_sided = e.parse(changed(text, SHAPES["one_sided"]))
    one_sided.set_jit(True)
    notes = e.batch_jit_check([q1, a, off, one_sided, b])
    assert notes[0] == "alone: grouped scans are not batched"
    assert notes[2] == "alone: specialisation is off"
    assert notes[3] == "alone: its filter shapes differ from every other plan's"
    assert [(x[0], x[1], x[2]) for x in slots([notes[1], notes[4]])] == [(0, 0, 2), (0, 1, 2)]
    # a plan of a batch checked on its own afterwards has no partner; one that is not fused says so
    assert e.batch_jit_check([a]) == ["alone: no other plan of the call can share a scan"]
    a.set_fusion(False)
    assert e.batch_jit_check([a, b])[0] == "alone: the plan is not fused"


def test_a_group_wider_than_the_cap_is_cut_into_batches(q6):
    text, e = q6
    plans = q6_plans(e, text, 11)
    got = slots(e.batch_jit_check(plans))
    assert [(b, q, k) for b, q, k, _ in got] == [(0, q, 8) for q in range(8)] + [(1, q, 3) for q in range(3)]
    nine = e.batch_jit_check(plans[:9])
    assert nine[8] == "alone: the one plan left over when its group was cut into batches of 8", nine
    assert [(x[0], x[1], x[2]) for x in slots(nine[:8])] == [(0, q, 8) for q in range(8)]


def test_seven_aggregates_cap_the_batch_at_four(tmp_path, monkeypatch):
    """edge_global keeps a count and six accumulators per slot: 4 x 7 <= 32 < 5 x 7"""
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    import test_scan_forms as F
    text, cols = F.program("edge_global", 5000)
    e = F.declared_engine(cols)
    plans = [e.parse(text) for _ in range(6)]
    for p in plans:
        p.set_jit(True)
    got = slots(e.batch_jit_check(plans))
    assert [(b, q, k) for b, q, k, _ in got] == [(0, q, 4) for q in range(4)] + [(1, 0, 2), (1, 1, 2)]
    e.close()


def test_argument_errors(q6):
    text, e = q6
    L = _lib.load()
    import ctypes
    a, b = q6_plans(e, text, 2)
    for fn in (L.vdl_run_batch, L.vdl_batch_jit_check):
        arr = (ctypes.c_void_p * 2)(a._h, b._h)
        assert fn(e._c, arr, 0) == _lib.VDL_ERR_ARG
        assert fn(e._c, arr, -1) == _lib.VDL_ERR_ARG
        assert fn(e._c, None, 2) == _lib.VDL_ERR_ARG
        assert fn(e._c, (ctypes.c_void_p * 2)(a._h, None), 2) == _lib.VDL_ERR_ARG
        assert b"plan 1 is null" in L.vdl_last_error(e._c)
        assert fn(e._c, (ctypes.c_void_p * 3)(a._h, b._h, a._h), 3) == _lib.VDL_ERR_ARG
        assert b"plans 0 and 2 are the same plan" in L.vdl_last_error(e._c)
    with pytest.raises(m.VdlError):
        e.run_batch([])
    # a context without a device cannot run a batch, and says so as vdl_run does
    with pytest.raises(m.VdlError) as err:
        e.run_batch([a, b])
    assert err.value.code == _lib.VDL_ERR_DEVICE


def test_vdlrun_batch_needs_jit_and_one_gpu(tmp_path):
    other = tmp_path / "b.vdl"
    other.write_text(golden("q6.vdl"))
    text = golden("q6.vdl").encode()
    r = subprocess.run([VDLRUN, "--rows", "1000", "--batch", str(other)], input=text, capture_output=True, timeout=120)
    assert r.returncode == 2 and r.stderr.startswith(b"usage: vdlrun") and b"--jit" in r.stderr and r.stdout == b""
    r = subprocess.run([VDLRUN, "--jit", "--gpus", "2", "--rows", "1000", "--batch", str(other)], input=text, capture_output=True, timeout=120)
    assert r.returncode == 3 and b"--batch is not served with --gpus" in r.stderr and r.stdout == b""
    r = subprocess.run([VDLRUN, "--jit", "--rows", "1000", "--batch", str(tmp_path / "missing.vdl")], input=text, capture_output=True, timeout=120)
    assert r.returncode == 1 and b"cannot read" in r.stderr
