"""ORDER BY / LIMIT in sharded runs, the device-free part: vdl_order_merge_host -- the rule k_ord_merge applies to the ranks' gathered
candidates -- is exactly np.lexsort over (u_1, .., u_K, run, index); the switch vdl_plan_set_order_sharded lifts the refusal of
vdl_run_sharded* and of nothing else; the exchange route refuses limits it cannot merge before it needs a device; vdlrun takes
--order-sharded; the merge kernel is part of the library build.  Every comparison is exact."""
import os
import re
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib, engine
from conftest import ROOT

VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
WORLDS = [1, 2, 3, 5, 8]


def golden(name):
    return open(os.path.join(ROOT, "tests", "golden", name)).read()


def sorted_runs(rng, counts, kinds):
    """One block of order words per key over all candidates, run after run, every run ascending under the words (ties in its own order)"""
    n = int(sum(counts))
    cols = []
    for kind in kinds:
        if kind == "wide":
            c = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
        elif kind == "ends":
            c = rng.choice(np.array([0, 1, U64_MAX - np.uint64(1), U64_MAX], dtype=np.uint64), size=n)
        elif kind == "few":
            c = rng.integers(0, 3, size=n, dtype=np.uint64)
        else:                                         # "equal"
            c = np.full(n, 7, dtype=np.uint64)
        cols.append(c)
    at = 0
    for cnt in counts:
        order = np.lexsort(tuple(c[at:at + cnt] for c in cols[::-1])) if cols else np.arange(cnt)
        for c in cols:
            c[at:at + cnt] = c[at:at + cnt][order]
        at += cnt
    return cols


def reference(counts, cols, limit):
    run = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    idx = np.concatenate([np.arange(c, dtype=np.int64) for c in counts]) if len(counts) else np.zeros(0, np.int64)
    order = np.lexsort(tuple([idx, run] + cols[::-1]))
    if limit > 0:
        order = order[:limit]
    return run[order], idx[order]


def run_lengths(rng, world):
    """includes 0, 1 and 4096 wherever the world has room for them"""
    base = [4096, 0, 1, 17, 4096, 300, 0, 2049]
    counts = [base[(r + world) % len(base)] for r in range(world)]
    if world == 1:
        counts = [4096]
    return counts, [int(x) for x in rng.integers(0, 200, size=world)]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("kinds", [("wide",), ("few",), ("equal",), ("ends",), ("equal", "wide"), ("equal", "few"), ("few", "ends", "wide"), ()])
def test_merge_host_equals_lexsort_over_words_run_and_index(world, kinds):
    rng = np.random.default_rng(100 * world + len(kinds) + sum(len(k) for k in kinds))
    big, small = run_lengths(rng, world)
    for counts in (big, small, [0] * world, [1] * world):
        cols = sorted_runs(rng, counts, kinds)
        total = int(sum(counts))
        for limit in sorted({1, 10, max(total - 1, 1), total + 5, 0}):
            run, idx = engine.order_merge_host(counts, cols, limit)
            want_run, want_idx = reference(counts, cols, limit)
            assert len(run) == (min(limit, total) if limit else total)
            assert np.array_equal(run, want_run) and np.array_equal(idx, want_idx), (world, kinds, counts, limit)


def test_merge_host_ties_come_out_in_run_then_index_order():
    counts = [3, 0, 2, 4]
    cols = [np.full(9, 5, dtype=np.uint64)]
    run, idx = engine.order_merge_host(counts, cols, 0)
    assert run.tolist() == [0, 0, 0, 2, 2, 3, 3, 3, 3] and idx.tolist() == [0, 1, 2, 0, 1, 0, 1, 2, 3]
    run, idx = engine.order_merge_host(counts, [], 4)           # no keys: the ranks' rows one after the other
    assert run.tolist() == [0, 0, 0, 2] and idx.tolist() == [0, 1, 2, 0]
    # a tie between a lower and a higher rank at the cut: the lower rank's row is the one that stays
    run, idx = engine.order_merge_host([2, 2], [np.array([1, 9, 1, 9], dtype=np.uint64)], 3)
    assert list(zip(run.tolist(), idx.tolist())) == [(0, 0), (1, 0), (0, 1)]


def test_merge_host_at_the_ends_of_the_word_range():
    w = np.array([0, U64_MAX, 0, 0, U64_MAX, U64_MAX], dtype=np.uint64)
    run, idx = engine.order_merge_host([2, 1, 3], [w], 0)
    assert list(zip(run.tolist(), idx.tolist())) == [(0, 0), (1, 0), (2, 0), (0, 1), (2, 1), (2, 2)]


def test_merge_host_rejects_bad_arguments():
    L = _lib.load()
    import ctypes
    p64, pu64 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64)
    cnt = (ctypes.c_int64 * 2)(2, 1)
    w = (ctypes.c_uint64 * 3)(1, 2, 1)
    run, idx, got = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)(), ctypes.c_int64()
    args = (ctypes.cast(cnt, p64), ctypes.cast(w, pu64))
    assert L.vdl_order_merge_host(2, 1, *args, 0, run, idx, ctypes.byref(got)) == _lib.VDL_OK and got.value == 3
    assert list(zip(run, idx)) == [(0, 0), (1, 0), (0, 1)]
    assert L.vdl_order_merge_host(0, 1, *args, 0, run, idx, None) == _lib.VDL_ERR_ARG
    assert L.vdl_order_merge_host(129, 1, *args, 0, run, idx, None) == _lib.VDL_ERR_ARG
    assert L.vdl_order_merge_host(2, 9, *args, 0, run, idx, None) == _lib.VDL_ERR_ARG
    assert L.vdl_order_merge_host(2, 1, *args, -1, run, idx, None) == _lib.VDL_ERR_ARG
    assert L.vdl_order_merge_host(2, 1, ctypes.cast(cnt, p64), None, 0, run, idx, None) == _lib.VDL_ERR_ARG
    cnt[1] = -1
    assert L.vdl_order_merge_host(2, 1, *args, 0, run, idx, None) == _lib.VDL_ERR_ARG


# ---- the switch ---------------------------------------------------------------------------------------------------------------------

def test_the_switch_lifts_the_refusal_of_run_sharded_and_of_nothing_else():
    e = m.Engine(device=None)
    p = e.parse(golden("q3.vdl"))
    p.set_sharded_table("lineitem")
    p.set_order([("revenue", True)], limit=10, sharded=True)
    assert p.sharded_route() == ("exchange", True)              # every rank ends with the merged rows
    for call in (lambda: p.run_sharded(), lambda: p.run_sharded_begin(0)):
        with pytest.raises(m.VdlError) as ei:
            call()
        assert "disjoint result rows" not in str(ei.value), str(ei.value)
    with pytest.raises(m.VdlError) as ei:
        p.run_sharded()
    assert ei.value.code in (_lib.VDL_ERR_DEVICE, _lib.VDL_ERR_ARG), str(ei.value)       # for want of a device or a communicator
    for call in (lambda: p.exchange_begin(2), lambda: p.run_local(0x1000)):
        with pytest.raises(m.VdlError) as ei:
            call()
        assert ei.value.code == _lib.VDL_ERR_UNSUPPORTED and "vdl_run_sharded" in str(ei.value) and "collectives" in str(ei.value), str(ei.value)
    # every set_order passes its `sharded` down: a plain one switches the merged order off again
    p.set_order([("revenue", True)], limit=10)
    assert p.sharded_route() == ("exchange", False)
    with pytest.raises(m.VdlError) as ei:
        p.run_sharded()
    assert ei.value.code == _lib.VDL_ERR_UNSUPPORTED and "disjoint result rows" in str(ei.value) and "not built" in str(ei.value)
    # a fold plan under the switch: accepted, fails for want of a device
    q6 = e.parse(golden("q6.vdl"))
    q6.set_order([("revenue", True)], limit=1, sharded=True)
    assert q6.sharded_route() == ("fold", True)
    with pytest.raises(m.VdlError) as ei:
        q6.run_sharded()
    assert ei.value.code == _lib.VDL_ERR_DEVICE, str(ei.value)
    e.close()


@pytest.mark.parametrize("limit", [0, 5000, 4097])
def test_the_exchange_route_refuses_a_limit_it_cannot_merge_before_it_needs_a_device(limit):
    e = m.Engine(device=None)
    p = e.parse(golden("q3.vdl"))
    p.set_sharded_table("lineitem")
    p.set_order([("revenue", True), "o_orderdate__orders__o_orderdate"], limit=limit, sharded=True)
    with pytest.raises(m.VdlError) as ei:
        p.run_sharded()
    msg = str(ei.value)
    assert ei.value.code == _lib.VDL_ERR_UNSUPPORTED and "4096" in msg and "exchange route" in msg and ("limit %d" % limit) in msg, msg
    assert p.sharded_route() == ("exchange", False)
    p.set_order([("revenue", True)], limit=4096, sharded=True)
    with pytest.raises(m.VdlError) as ei:
        p.run_sharded()
    assert ei.value.code != _lib.VDL_ERR_UNSUPPORTED, str(ei.value)
    e.close()


# ---- vdlrun -----------------------------------------------------------------------------------------------------------------------

def test_vdlrun_takes_order_sharded_and_keeps_refusing_without_it():
    args = ["--gpus", "2", "--order-by", "revenue:desc,tmp115:asc", "--limit", "10"]
    r = subprocess.run([VDLRUN] + args + ["--order-sharded", "--describe"], input=golden("q3.vdl"), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout != "", r.stderr
    r = subprocess.run([VDLRUN] + args + ["--rows", "1000"], input=golden("q3.vdl"), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == "" and "disjoint result rows" in r.stderr
    r = subprocess.run([VDLRUN, "--no-such-option"], input="", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--order-sharded" in r.stderr
    head = open(os.path.join(ROOT, "mplan2vdl_amd", "csrc", "vdlrun.cpp")).read().split("#include")[0]
    assert "--order-sharded" in head


# ---- the build ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["k_ord_merge", "k_ord_block"])
def test_the_merge_kernels_are_built_for_gfx950_and_their_resource_report_is_in_the_design(kernel):
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and kernel.encode() in blob
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    row = re.search(r"^\|\s*`?%s`?\s*\|(.*)$" % kernel, design, flags=re.M)
    assert row, "DESIGN.md has no resource row for " + kernel
    cells = [c.strip() for c in row.group(1).strip().strip("|").split("|")]
    assert len(cells) >= 5 and cells[3] == "0", (kernel, cells)           # VGPRs, SGPRs, LDS, scratch = 0, occupancy
    assert "vdl_plan_set_order_sharded" in open(os.path.join(ROOT, "include", "vdl.h")).read()
