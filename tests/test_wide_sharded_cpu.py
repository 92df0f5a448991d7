"""Wide sums in sharded runs (vdl_plan_set_wide_sums_sharded; DESIGN.md section 5.17 "Sharded runs") without a GPU: the merge rule of
the ranks' (lo, hi) partial words on the host -- vdl_comm_merge_host_wide, the definition k_merge_words_wide shares -- against Python
integer arithmetic, its argument checks, the switch and its environment variable, and the CLI's refusal without --wide-sharded."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
import wide_cases as wc
from mplan2vdl_amd import _lib

I64_MAX, I64_MIN, MASK = wc.I64_MAX, wc.I64_MIN, wc.MASK
NONE, SUM, MIN, MAX, FIRST = _lib.REDUCE_NONE, _lib.REDUCE_SUM, _lib.REDUCE_MIN, _lib.REDUCE_MAX, _lib.REDUCE_FIRST
SPECIAL = np.array([0, 1, -1, I64_MAX, I64_MIN, 1 << 62, -(1 << 62)], dtype=np.int64)
VDLRUN = os.path.join(wc.ROOT, "mplan2vdl_amd", "bin", "vdlrun")
P64 = ctypes.POINTER(ctypes.c_int64)


def signed(x, bits=64):
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def draw(rng, n):
    """n int64 words: the special values and random ones, about half each"""
    out = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    pick = rng.random(n) < 0.5
    out[pick] = rng.choice(SPECIAL, int(pick.sum()))
    return out


def blocks(rng, world, nw, stride, failing=()):
    """`world` blocks of `stride` words: raw, resolved, status, high words (and whatever the stride leaves behind them)"""
    g = draw(rng, world * stride).reshape(world, stride)
    g[:, 2 * nw] = 0
    for r in failing:
        g[r, 2 * nw] = 3 + r
    return g


def plain_merge(world, ops, g, stride):
    """vdl_comm_merge_host over the same blocks: it reads their first 2 * n_words + 1 words"""
    L = _lib.load()
    nw = len(ops)
    out, status = np.zeros(nw, np.int64), np.zeros(2, np.int64)
    c_ops = (ctypes.c_int32 * max(nw, 1))(*ops)
    flat = np.ascontiguousarray(g.reshape(-1))
    assert L.vdl_comm_merge_host(world, nw, c_ops, flat.ctypes.data_as(P64), stride, out.ctypes.data_as(P64), status.ctypes.data_as(P64)) == _lib.VDL_OK
    return out, (int(status[0]), int(status[1]))


@pytest.mark.parametrize("world", range(1, 9))
@pytest.mark.parametrize("nw", [0, 1, 300])
def test_the_host_merge_against_python_integers(world, nw):
    rng = np.random.default_rng(1000 * world + nw)
    for extra, failing in ((0, ()), (5, (world - 1,)), (0, tuple(r for r in (2, 5) if r < world))):
        stride = 3 * nw + 1 + extra
        ops = [int(x) for x in rng.choice([NONE, SUM, MIN, MAX, FIRST], nw)]
        g = blocks(rng, world, nw, stride, failing)
        lo, hi, status = m.comm_merge_host_wide(world, ops, g.reshape(-1), stride_words=stride if extra else 0)
        want_lo, want_status = plain_merge(world, ops, g, stride)
        assert np.array_equal(lo, want_lo)
        assert status == want_status == ((3 + min(failing), min(failing)) if failing else (0, -1))
        for i, op in enumerate(ops):
            if op in (NONE, SUM):
                exact = sum((int(g[r, 2 * nw + 1 + i]) << 64) | (int(g[r, i]) & MASK) for r in range(world))
                assert (int(hi[i]) << 64) | (int(lo[i]) & MASK) == signed(exact, 128), (i, op)
            else:
                assert int(hi[i]) == int(lo[i]) >> 63, (i, op)


def one(world, op, raw, high, resolved=None):
    """the merged (lo, hi) of one word whose rank r holds (raw[r], high[r])"""
    g = np.zeros((world, 4), np.int64)
    g[:, 0] = [signed(x) for x in raw]
    g[:, 1] = g[:, 0] if resolved is None else resolved
    g[:, 3] = high
    lo, hi, status = m.comm_merge_host_wide(world, [op], g.reshape(-1))
    assert status == (0, -1)
    return int(lo[0]), int(hi[0])


def test_directed_carries():
    for k in (0, 1, 12345):                                    # two ranks in [2^63, 2^64): the carry comes from the merge alone
        assert one(2, SUM, [(1 << 63) + k, (1 << 63) + k], [0, 0]) == (2 * k, 1)
    for world in range(1, 9):                                  # every rank holds -1
        assert one(world, SUM, [-1] * world, [-1] * world) == (-world, -1)
    assert one(2, SUM, [0, 0], [1, -1]) == (0, 0)              # +2^64 against -2^64
    assert one(3, SUM, [0, 5, 0], [1, 0, -1]) == (5, 0)
    assert one(3, SUM, [I64_MIN, I64_MIN, I64_MIN], [-1, -1, -1]) == (signed(3 * I64_MIN), (3 * I64_MIN) >> 64)
    # MIN / MAX / FIRST ignore the ranks' high words and deliver the sign extension of what they merge
    assert one(3, MIN, [5, -7, 9], [123, 456, 789]) == (-7, -1)
    assert one(3, MAX, [5, -7, 9], [123, 456, 789]) == (9, 0)
    assert one(3, MAX, [-5, -7, -9], [0, 0, 0]) == (-5, -1)
    assert one(3, FIRST, [40, 20, 30], [1, 1, 1], resolved=[111, -222, 333]) == (-222, -1)      # the rank with the smallest row id
    assert one(2, FIRST, [I64_MAX, I64_MAX], [0, 0], resolved=[7, 8]) == (0, 0)                 # no rank has a row in the group


def test_argument_errors():
    L = _lib.load()
    nw, world = 3, 2
    g = np.zeros(world * (3 * nw + 1), np.int64)
    ops = (ctypes.c_int32 * nw)(SUM, MIN, FIRST)
    lo, hi, st = np.zeros(nw, np.int64), np.zeros(nw, np.int64), np.zeros(2, np.int64)
    a = lambda x: x.ctypes.data_as(P64)                        # noqa: E731
    call = L.vdl_comm_merge_host_wide
    assert call(world, nw, ops, a(g), 3 * nw + 1, a(lo), a(hi), a(st)) == _lib.VDL_OK
    assert call(world, nw, ops, a(g), 0, a(lo), a(hi), None) == _lib.VDL_OK            # 0 = exactly 3 * n_words + 1
    for stride in (3 * nw, 2 * nw + 1, 1, -1):
        assert call(world, nw, ops, a(g), stride, a(lo), a(hi), a(st)) == _lib.VDL_ERR_ARG
    assert call(world, nw, ops, a(g), 0, None, a(hi), None) == _lib.VDL_ERR_ARG
    assert call(world, nw, ops, a(g), 0, a(lo), None, None) == _lib.VDL_ERR_ARG
    assert call(world, nw, None, a(g), 0, a(lo), a(hi), None) == _lib.VDL_ERR_ARG
    assert call(world, nw, ops, None, 0, a(lo), a(hi), None) == _lib.VDL_ERR_ARG
    assert call(0, nw, ops, a(g), 0, a(lo), a(hi), None) == _lib.VDL_ERR_ARG
    assert call(world, -1, ops, a(g), 0, a(lo), a(hi), None) == _lib.VDL_ERR_ARG
    assert call(world, 0, None, None, 0, None, None, None) == _lib.VDL_OK              # no words, no status: nothing to read
    assert call(world, 0, None, None, 0, None, None, a(st)) == _lib.VDL_ERR_ARG        # a status needs the blocks
    with pytest.raises(m.VdlError):
        m.comm_merge_host_wide(world, [SUM] * nw, g, stride_words=3 * nw)
    with pytest.raises(ValueError):
        m.comm_merge_host_wide(world + 1, [SUM] * nw, g)


def test_the_switch_round_trips_and_goes_with_the_mode(monkeypatch):
    monkeypatch.delenv("VDL_WIDE_SHARDED", raising=False)
    monkeypatch.delenv("VDL_WIDE_SUMS", raising=False)
    e = m.Engine(device=None)
    L = e._L
    p = e.parse(wc.GLOBAL)
    assert p.wide_sums_sharded is False
    assert L.vdl_plan_set_wide_sums_sharded(None, 1) == _lib.VDL_ERR_ARG and L.vdl_plan_wide_sums_sharded(None) == 0
    for mode in (1, 2):
        p.set_wide_sums(mode, sharded=True)
        assert p.wide_sums == mode and p.wide_sums_sharded is True
        p.set_wide_sums(mode)                                  # every call passes the switch down
        assert p.wide_sums == mode and p.wide_sums_sharded is False
    p.set_wide_sums(1, sharded=True)
    p.set_wide_sums(0)
    assert p.wide_sums == 0 and p.wide_sums_sharded is False
    p.set_wide_sums(0, sharded=True)                           # the switch says how a WIDE plan is sharded
    assert p.wide_sums_sharded is False
    assert L.vdl_plan_set_wide_sums_sharded(p._h, 1) == _lib.VDL_OK and L.vdl_plan_set_wide_sums(p._h, 1) == _lib.VDL_OK
    assert p.wide_sums_sharded is True
    assert L.vdl_plan_set_wide_sums(p._h, 0) == _lib.VDL_OK    # mode 0 through the C interface clears it too
    assert p.wide_sums_sharded is False
    e.close()


@pytest.mark.parametrize("value,on", [("1", True), ("0", False), ("2", False), ("yes", False), ("", False)])
def test_the_switch_in_the_environment_is_read_at_parse(value, on, monkeypatch):
    monkeypatch.setenv("VDL_WIDE_SHARDED", value)
    monkeypatch.setenv("VDL_WIDE_SUMS", "1")
    e = m.Engine(device=None)
    p = e.parse(wc.GLOBAL)
    monkeypatch.delenv("VDL_WIDE_SHARDED")
    monkeypatch.delenv("VDL_WIDE_SUMS")
    assert p.wide_sums == 1 and p.wide_sums_sharded is on
    assert e.parse(wc.GLOBAL).wide_sums_sharded is False       # (read at parse, not later)
    e.close()


@pytest.mark.parametrize("option", ["--wide-sums", "--checked-sums"])
def test_vdlrun_with_gpus_refuses_wide_sums_without_the_switch(option, monkeypatch):
    monkeypatch.delenv("VDL_WIDE_SHARDED", raising=False)
    q1 = open(os.path.join(wc.ROOT, "tests", "golden", "q1.vdl")).read()
    r = subprocess.run([VDLRUN, "--gpus", "2", "--rows", "1000", option], input=q1.encode(), capture_output=True, timeout=120)
    err = r.stderr.decode()
    assert r.returncode != 0 and r.stdout == b"", err
    assert "add-with-carry" in err and "--wide-sharded" in err, err


def test_refusals_come_from_the_plan_alone():
    """no device and no communicator: every refusal is decided before either is asked for, so every rank decides the same"""
    e = m.Engine(device=None)

    def refused(p, call, *needles):
        p.set_wide_sums(2, sharded=True)
        with pytest.raises(m.VdlError) as err:
            call(p)
        msg = str(err.value)
        assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and all(s in msg for s in needles), msg

    q3 = e.parse(open(os.path.join(wc.ROOT, "tests", "golden", "q3.vdl")).read())
    q3.set_sharded_table("lineitem")
    refused(q3, lambda p: p.run_sharded(), "vdl_run_sharded", "exchange route", "k_group_fold")
    off = e.parse(wc.GLOBAL)
    off.set_fusion(False)
    off.set_sharded_table("t")
    refused(off, lambda p: p.run_sharded_begin(1), "vdl_run_sharded_begin", "fusion is off", "k_fold_global")
    direct = e.parse(wc.GLOBAL)
    for name, call in (("vdl_run_local", lambda p: p.run_local(1 << 20)), ("vdl_finalize", lambda p: p.finalize(1 << 20)),
                       ("vdl_finalize_begin", lambda p: p.finalize_begin(1 << 20, 0)), ("vdl_finalize_end", lambda p: p.finalize_end(0)),
                       ("vdl_resolve_first", lambda p: p.resolve_first(1 << 20))):
        refused(direct, call, name, "leaves the collectives to its caller")
    direct.set_wide_sums(1)                                    # switch off: the refusal every sharded entry point has given since wide sums exist
    with pytest.raises(m.VdlError) as err:
        direct.run_sharded()
    assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "vdl_run_sharded" in str(err.value) and "add-with-carry" in str(err.value)
    e.close()
