"""Sharded batches (vdl_run_batch_sharded, Engine.run_batch_sharded) without a GPU: the host twin of the batch merge against the
one-plan twin, plan by plan; the layout of a mixed call pinned by hand; the argument errors; the option rules of `vdlrun
--batch-sharded`.  The answers are checked on the device (test_batch_sharded.py).

A rank's block is the concatenation, in call order, of one segment per shared plan: [raw n_words][the words with FIRST entries
resolved, only where the plan has a FIRST word][status].  vdl_comm_merge_host reads a one-plan block [raw][resolved][status], so a
plan's segments are copied into such blocks (the resolved half of a plan without FIRST words is filled with other values: no
operator but FIRST may read it) and both twins must give the same words and the same {status, rank}."""
import ctypes
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib
from conftest import golden
from test_batch_cpu import VDLRUN, literal_set
from test_jit_bounds_cpu import changed

I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1
P64 = ctypes.POINTER(ctypes.c_int64)
# (n_words, has FIRST words): heights 8, 3, 579, 33, 3, 7 -- neither the words nor the heights are monotone
PLANS = [(7, False), (2, False), (289, True), (16, True), (2, False), (3, True)]
FAILED = 2                          # the plan whose status word is set, on a middle rank


def blocks(world, rng):
    """(n_words, offsets, ops per plan, gathered, block words, status rank)"""
    n_words, offsets, ops, at = [], [], [], 0
    for nw, first in PLANS:
        o = rng.integers(1, 4, nw)                              # SUM / MIN / MAX
        if first:
            o[rng.choice(nw, max(1, nw // 4), replace=False)] = _lib.REDUCE_FIRST
        n_words.append(nw)
        offsets.append(at)
        ops.append([int(x) for x in o])
        at += (2 if first else 1) * nw + 1
    g = rng.integers(I64MIN, I64MAX, size=world * at, dtype=np.int64, endpoint=True)
    ends = rng.choice(len(g), len(g) // 8, replace=False)
    g[ends] = rng.choice([I64MIN, I64MAX, I64MIN + 1, I64MAX - 1, 0, -1], len(ends))      # sums wrap, MIN / MAX meet the identities
    bad_rank = world // 2
    for q, (nw, first) in enumerate(PLANS):
        for r in range(world):
            base = r * at + offsets[q]
            for i, op in enumerate(ops[q]):
                if op == _lib.REDUCE_FIRST:                     # a global row id, or INT64_MAX where the rank has no row of the group
                    g[base + i] = I64MAX if rng.random() < 0.3 else int(rng.integers(0, 1 << 40))
            g[base + (2 if first else 1) * nw] = 4 if (q == FAILED and r == bad_rank) else 0
    return n_words, offsets, ops, g, at, bad_rank


def one_plan(world, nw, ops, block):
    """vdl_comm_merge_host over blocks [raw][resolved][status] of 2 nw + 1 words"""
    L = _lib.load()
    flat = np.ascontiguousarray(block, dtype=np.int64)
    out, status = np.zeros(nw, np.int64), np.zeros(2, np.int64)
    c_ops = (ctypes.c_int32 * nw)(*ops)
    assert L.vdl_comm_merge_host(world, nw, c_ops, flat.ctypes.data_as(P64), 2 * nw + 1, out.ctypes.data_as(P64), status.ctypes.data_as(P64)) == _lib.VDL_OK
    return out, (int(status[0]), int(status[1]))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_the_batch_twin_equals_the_one_plan_twin_plan_by_plan(world):
    rng = np.random.default_rng(100 + world)
    n_words, offsets, ops, g, B, bad_rank = blocks(world, rng)
    got, status = m.comm_merge_host_batch(world, n_words, offsets, ops, g, B)
    assert len(got) == len(PLANS) and [len(x) for x in got] == n_words
    for q, (nw, first) in enumerate(PLANS):
        single = np.empty((world, 2 * nw + 1), np.int64)
        for r in range(world):
            seg = g[r * B + offsets[q]: r * B + offsets[q] + (2 if first else 1) * nw + 1]
            single[r, :nw] = seg[:nw]
            single[r, nw:2 * nw] = seg[nw:2 * nw] if first else rng.integers(I64MIN, I64MAX, nw, dtype=np.int64)
            single[r, 2 * nw] = seg[-1]
        want, want_status = one_plan(world, nw, ops[q], single.reshape(-1))
        assert np.array_equal(got[q], want), q
        assert status[q] == want_status == ((4, bad_rank) if q == FAILED else (0, -1)), (q, status[q], want_status)
    # a FIRST word took the value of the rank with the smallest row id; sums wrapped
    q = 2
    i = ops[q].index(_lib.REDUCE_FIRST)
    ids = [int(g[r * B + offsets[q] + i]) for r in range(world)]
    assert int(got[q][i]) == int(g[ids.index(min(ids)) * B + offsets[q] + PLANS[q][0] + i])
    i = ops[0].index(_lib.REDUCE_SUM) if _lib.REDUCE_SUM in ops[0] else None
    if i is not None:
        total = sum(int(g[r * B + offsets[0] + i]) for r in range(world))
        assert int(got[0][i]) == (total + (1 << 63)) % (1 << 64) - (1 << 63)


def test_the_twin_refuses_segments_outside_the_block():
    with pytest.raises(m.VdlError):
        m.comm_merge_host_batch(1, [2], [1], [[1, 1]], np.zeros(3, np.int64), 3)          # 1 + 3 > 3
    with pytest.raises(m.VdlError):
        m.comm_merge_host_batch(1, [2], [0], [[1, 4]], np.zeros(4, np.int64), 4)          # a FIRST word: 2 * 2 + 1 > 4
    got, status = m.comm_merge_host_batch(1, [2], [0], [[1, 4]], np.array([5, 0, 6, 7, 0], np.int64), 5)
    assert got[0].tolist() == [5, 7] and status == [(0, -1)]


@pytest.fixture
def mixed(tmp_path, monkeypatch):
    """one context without a device over the declared columns of Q6, the global edge program, Q1 and Q3"""
    import test_jit as J
    import test_jit_bounds as JB
    import test_packed_images_cpu as P
    import test_scan_forms as F
    from mplan2vdl_amd import datagen
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    e = m.Engine(device=None)
    seen = set()

    def declare(cols):
        for k, v in cols.items():
            if k not in seen:
                e.register_pointer(k, 0x10000, v.dtype.itemsize, len(v))
                seen.add(k)

    for k in datagen.Q6_COLUMNS:
        e.register_pointer(k, 0x10000, 8, 600000)
        seen.add(k)
    edge_text, edge_cols = F.program("edge_global", 5000)
    declare(edge_cols)
    q1_text, q1_cols = J.compiled(1, 1e-4)
    declare(q1_cols)
    q3_text, q3_cols = J.compiled(3, 1e-4)
    declare(q3_cols)
    texts = {"q6": P.q6(), "edge": changed(edge_text, JB.VARIANTS["edge_global"][1][0]), "q1": q1_text, "q3": q3_text}
    yield e, texts
    e.close()


def test_the_layout_of_a_mixed_call(mixed):
    e, texts = mixed
    plans = [e.parse(changed(texts["q6"], literal_set(0))), e.parse(texts["edge"]), e.parse(texts["q1"]), e.parse(changed(texts["q6"], literal_set(1))),
             e.parse(texts["q3"]), e.parse(changed(texts["q6"], literal_set(2)))]
    for p in plans:
        p.set_jit(True)
    plans[4].set_sharded_table("lineitem")
    assert plans[2].partial_spec()[0] == 257 and _lib.REDUCE_FIRST in plans[2].partial_spec()[1]
    off, h, B = e.batch_sharded_layout(plans)
    # Q6: count + one sum + status; the edge program: count + six aggregates + status; Q1: 257 words twice (FIRST words) + status
    assert h == [3, 8, 2 * 257 + 1, 3, 0, 3]
    assert off == [0, 3, 11, 526, -1, 529] and B == 532
    notes = [p.batch_sharded_note() for p in plans]
    assert notes[0] == "collective 0: words [0,3) of 532" and notes[2] == "collective 0: words [11,526) of 532" and notes[5] == "collective 0: words [529,532) of 532"
    assert notes[4] == "own: exchange route", notes
    # classification follows the plan alone: fusion off is an own plan on the fold route, wide sums are own where the gate lets them through
    plans[1].set_fusion(False)
    plans[1].set_sharded_table("t")
    plans[0].set_wide_sums(1, sharded=True)
    off, h, B = e.batch_sharded_layout(plans)
    assert off == [-1, -1, 0, 515, -1, 518] and B == 521
    assert plans[0].batch_sharded_note() == "own: fold route" and plans[1].batch_sharded_note() == "own: fold route"
    # a wide plan the gate refuses, and an order without its switch, fail the call up front with the plan's index
    plans[0].set_wide_sums(1, sharded=False)
    with pytest.raises(m.VdlError) as err:
        e.batch_sharded_layout(plans)
    assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "] plan 0: vdl_batch_sharded_layout: wide sums are on" in str(err.value) and "add-with-carry" in str(err.value)
    plans[0].set_wide_sums(0)
    field = "revenue"
    plans[3].set_order([(field, True)], limit=1)
    with pytest.raises(m.VdlError) as err:
        e.batch_sharded_layout(plans)
    assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "] plan 3: an order is set on this plan" in str(err.value)
    plans[3].set_order([(field, True)], limit=1, sharded=True)
    assert e.batch_sharded_layout(plans)[0][3] >= 0


def test_argument_errors(mixed):
    e, texts = mixed
    L = _lib.load()
    a, b = e.parse(texts["q6"]), e.parse(changed(texts["q6"], literal_set(1)))
    off, h, B = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)(), ctypes.c_int64()
    calls = [lambda arr, n: L.vdl_run_batch_sharded(e._c, arr, n), lambda arr, n: L.vdl_batch_sharded_layout(e._c, arr, n, off, h, ctypes.byref(B))]
    for call in calls:
        arr = (ctypes.c_void_p * 2)(a._h, b._h)
        assert call(arr, 0) == _lib.VDL_ERR_ARG
        assert call(arr, -1) == _lib.VDL_ERR_ARG
        assert call(None, 2) == _lib.VDL_ERR_ARG
        assert call((ctypes.c_void_p * 2)(a._h, None), 2) == _lib.VDL_ERR_ARG
        assert b"plan 1 is null" in L.vdl_last_error(e._c)
        assert call((ctypes.c_void_p * 3)(a._h, b._h, a._h), 3) == _lib.VDL_ERR_ARG
        assert b"plans 0 and 2 are the same plan" in L.vdl_last_error(e._c)
    assert b"vdl_batch_sharded_layout" in L.vdl_last_error(e._c)
    with pytest.raises(m.VdlError):
        e.run_batch_sharded([])
    # no communicator on the context: the words of every sharded entry point
    with pytest.raises(m.VdlError) as err:
        e.run_batch_sharded([a, b])
    assert err.value.code == _lib.VDL_ERR_ARG and "no communicator on this context" in str(err.value)
    assert a.batch_sharded_note() == ""                        # (nothing was classified)


def test_vdlrun_batch_sharded_option_rules(tmp_path):
    other = tmp_path / "b.vdl"
    other.write_text(golden("q6.vdl"))
    text = golden("q6.vdl").encode()

    def run(*args):
        return subprocess.run([VDLRUN, "--rows", "1000", *args], input=text, capture_output=True, timeout=120)

    for args in (("--jit", "--batch", str(other), "--batch-sharded"),                      # no --gpus
                 ("--jit", "--gpus", "2", "--batch-sharded"),                               # no --batch
                 ("--gpus", "2", "--batch", str(other), "--batch-sharded")):                # no --jit
        r = run(*args)
        assert r.returncode == 2 and r.stderr.startswith(b"usage: vdlrun") and r.stdout == b"", (args, r.stderr)
    assert b"--batch-sharded needs --gpus N, --batch FILE and --jit" in run("--jit", "--batch", str(other), "--batch-sharded").stderr
    # without the switch --gpus refuses --batch as it always did
    r = run("--jit", "--gpus", "2", "--batch", str(other))
    assert r.returncode == 3 and b"--batch is not served with --gpus" in r.stderr and r.stdout == b""
    r = run("--bogus")
    assert r.returncode == 2 and b"[--batch-sharded]" in r.stderr
