"""ORDER BY / LIMIT, the device-free part: vdl_order_host is exactly np.lexsort with the position as the last key; an order
specification is checked against the program text when it is set (host-only context); vdlrun rejects a malformed --order-by
before it needs a device; the order kernels are part of the library build.  Every comparison is exact."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib, engine
from conftest import ROOT

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")


def lexsort_reference(keys, descending, limit):
    """The order of the issue: keys as signed int64, key by key, each ascending or descending, ties by position.  A descending key
    is complemented (~k reverses the signed order and exists for INT64_MIN; negation does not)."""
    m_rows = len(keys[0])
    cols = [~k if d else k for k, d in zip(keys, descending)]
    order = np.lexsort(tuple([np.arange(m_rows, dtype=np.int64)] + cols[::-1]))
    return order[:limit] if limit > 0 else order


def limits_for(m_rows):
    return sorted({0, 1, 10, max(m_rows - 1, 0), m_rows, m_rows + 5})


SIZES = [0, 1, 2, 63, 64, 65, 1000, 100003]


def draw(rng, kind, m_rows):
    if kind == "wide":
        return rng.integers(I64_MIN, I64_MAX, size=m_rows, dtype=np.int64, endpoint=True)
    if kind == "edges":
        return rng.choice(np.array([I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1, I64_MAX - 1], dtype=np.int64), size=m_rows)
    if kind == "few":
        return rng.integers(0, 3, size=m_rows, dtype=np.int64, endpoint=True)
    if kind == "equal":
        return np.full(m_rows, 42, dtype=np.int64)
    return rng.integers(-1000, 1000, size=m_rows, dtype=np.int64)


@pytest.mark.parametrize("m_rows", SIZES)
@pytest.mark.parametrize("n_keys", [1, 2, 3, 4])
def test_order_host_equals_lexsort(m_rows, n_keys):
    rng = np.random.default_rng(1000 * n_keys + m_rows)
    directions = list(itertools.product([0, 1], repeat=n_keys)) if n_keys <= 3 else [(0, 1, 1, 0), (1, 0, 0, 1)]
    for kinds in (["small"] * n_keys, ["wide"] * n_keys, ["edges"] * n_keys, ["few"] * n_keys, (["few", "edges", "wide", "small"] * 2)[:n_keys]):
        keys = [draw(rng, kind, m_rows) for kind in kinds]
        for desc in directions:
            for limit in limits_for(m_rows):
                got = engine.order_host(keys, desc, limit)
                want = lexsort_reference(keys, desc, limit)
                assert got.dtype == np.int64 and len(got) == (min(limit, m_rows) if limit else m_rows)
                assert np.array_equal(got, want), (kinds, desc, limit, m_rows)


def test_order_host_sign_flip_and_complement_at_the_int64_ends():
    k = np.array([0, I64_MIN, -1, I64_MAX, I64_MIN, 0, I64_MAX, -1], dtype=np.int64)
    assert engine.order_host([k], [0], 0).tolist() == [1, 4, 2, 7, 0, 5, 3, 6]
    assert engine.order_host([k], [1], 0).tolist() == [3, 6, 0, 5, 2, 7, 1, 4]        # INT64_MIN last, not first: no negation
    assert engine.order_host([k], [1], 3).tolist() == [3, 6, 0]


def test_order_host_many_ties_on_every_key():
    """Two keys drawn from {0..3} over 100 003 rows: each of the 16 pairs occurs ~6 250 times, far more than any limit used."""
    rng = np.random.default_rng(7)
    m_rows = 100003
    keys = [draw(rng, "few", m_rows), draw(rng, "few", m_rows)]
    assert min(np.unique(keys[0] * 4 + keys[1], return_counts=True)[1]) > 5000
    for desc in itertools.product([0, 1], repeat=2):
        for limit in (1, 10, 4096, 0):
            assert np.array_equal(engine.order_host(keys, desc, limit), lexsort_reference(keys, desc, limit))


def test_order_host_all_equal_column_keeps_positions():
    k = draw(None, "equal", 1000)
    assert np.array_equal(engine.order_host([k], [1], 0), np.arange(1000))
    assert np.array_equal(engine.order_host([k, k], [0, 1], 17), np.arange(17))


def test_order_host_rejects_bad_arguments():
    L = _lib.load()
    out = (ctypes.c_int64 * 4)()
    k = (ctypes.c_int64 * 4)(3, 1, 2, 0)
    keys = (ctypes.POINTER(ctypes.c_int64) * 9)(*[ctypes.cast(k, ctypes.POINTER(ctypes.c_int64))] * 9)
    desc = (ctypes.c_int * 9)()
    assert L.vdl_order_host(1, keys, desc, 4, 0, out) == _lib.VDL_OK and list(out) == [3, 1, 2, 0]
    assert L.vdl_order_host(9, keys, desc, 4, 0, out) == _lib.VDL_ERR_ARG
    assert L.vdl_order_host(1, keys, desc, 4, -1, out) == _lib.VDL_ERR_ARG
    assert L.vdl_order_host(1, keys, desc, -4, 0, out) == _lib.VDL_ERR_ARG
    assert L.vdl_order_host(0, None, None, 4, 2, out) == _lib.VDL_OK and list(out)[:2] == [0, 1]       # no keys: program order


# ---- the specification is checked against the program text: no device, no run ------------------------------------------------------

Q3_FIELDS = {"l_orderkey__lineitem__l_orderkey": "tmp93", "revenue": "tmp110", "o_orderdate__orders__o_orderdate": "tmp115",
             "o_shippriority__orders__o_shippriority": "tmp120"}


def golden(name):
    return open(os.path.join(ROOT, "tests", "golden", name)).read()


def program_outputs(text):
    """(field, tmpN) of every MaterializeCompact, read off the text: the Project it materialises names the field"""
    lines = {}
    for line in text.splitlines():
        parts = line.split(";;")[0].strip().split(",")
        if len(parts) >= 2 and parts[0].isdigit():
            lines[int(parts[0])] = parts
    outs = []
    for lid, parts in sorted(lines.items()):
        if parts[1] == "MaterializeCompact":
            src = lines[int(parts[2].split()[1])]
            assert src[1] == "Project"
            outs.append((src[2], "tmp%d" % lid))
    return outs


def test_set_order_accepts_q3_and_q1_fields_by_name_and_by_tmp():
    e = m.Engine(device=None)
    assert dict(program_outputs(golden("q3.vdl"))) == Q3_FIELDS
    for name in ("q3.vdl", "q1.vdl"):
        p = e.parse(golden(name))
        outs = program_outputs(golden(name))
        assert len(outs) >= 4
        assert p.order_note() == ""
        for field, tmp in outs:
            p.set_order([field])
            p.set_order([(tmp, True)], limit=5)
        p.set_order([(f, k % 2 == 1) for k, (f, _) in enumerate(outs[:8])], limit=10)
        p.set_order([outs[0][0], (outs[1][1], True)])
        p.set_order([], limit=3)                     # no keys: the first rows in program order
        p.set_order([])                              # clears
        assert p.order_note() == ""
    e.close()


def test_set_order_rejects_unknown_duplicate_too_many_and_negative_limit():
    e = m.Engine(device=None)
    p = e.parse(golden("q3.vdl"))
    with pytest.raises(m.VdlError) as ei:
        p.set_order(["revenue", ("o_totalprice", True)], limit=10)
    assert ei.value.code == _lib.VDL_ERR_ARG and "o_totalprice" in str(ei.value)
    with pytest.raises(m.VdlError) as ei:
        p.set_order(["revenue", ("revenue", True)])
    assert ei.value.code == _lib.VDL_ERR_ARG and "revenue" in str(ei.value) and "twice" in str(ei.value)
    with pytest.raises(m.VdlError) as ei:
        p.set_order(["revenue", "tmp110"])            # the same output under its two names
    assert ei.value.code == _lib.VDL_ERR_ARG and "tmp110" in str(ei.value)
    with pytest.raises(m.VdlError) as ei:
        p.set_order(["revenue"], limit=-1)
    assert ei.value.code == _lib.VDL_ERR_ARG and "-1" in str(ei.value)
    q1 = e.parse(golden("q1.vdl"))
    outs = program_outputs(golden("q1.vdl"))
    assert len(outs) >= 9
    with pytest.raises(m.VdlError) as ei:
        q1.set_order([f for f, _ in outs[:9]])
    assert ei.value.code == _lib.VDL_ERR_ARG and "9" in str(ei.value)
    q1.set_order([f for f, _ in outs[:8]])            # eight are fine
    # a refused specification leaves the one before it in place, and needs no device either way: running still fails for want of one
    with pytest.raises(m.VdlError) as ei:
        p.run()
    assert ei.value.code == _lib.VDL_ERR_DEVICE
    e.close()


def test_sharded_entry_points_refuse_an_ordered_plan_before_they_need_a_device():
    e = m.Engine(device=None)
    p = e.parse(golden("q3.vdl"))
    p.set_order([("revenue", True)], limit=10)
    for call in (lambda: p.run_sharded(), lambda: p.run_sharded_begin(0), lambda: p.exchange_begin(2), lambda: p.run_local(0x1000)):
        with pytest.raises(m.VdlError) as ei:
            call()
        assert ei.value.code == _lib.VDL_ERR_UNSUPPORTED, str(ei.value)
        assert "disjoint result rows" in str(ei.value) and "not built" in str(ei.value)
    p.set_order([])
    with pytest.raises(m.VdlError) as ei:
        p.run_sharded()
    assert ei.value.code != _lib.VDL_ERR_UNSUPPORTED or "disjoint result rows" not in str(ei.value)
    e.close()


# ---- vdlrun ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [["--order-by", ""], ["--order-by", "revenue:down"], ["--order-by", "revenue,,o_orderdate"], ["--order-by", ":desc"],
                                  ["--order-by"], ["--limit", "-3"], ["--limit", "ten"], ["--limit"]])
def test_vdlrun_rejects_malformed_order_arguments_with_usage(args):
    r = subprocess.run([VDLRUN] + args, input=golden("q3.vdl"), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage: vdlrun" in r.stderr and "--order-by" in r.stderr and "--limit" in r.stderr
    assert r.stdout == ""


def test_vdlrun_refuses_order_with_gpus_before_it_starts_any_rank():
    r = subprocess.run([VDLRUN, "--gpus", "2", "--rows", "1000", "--order-by", "revenue:desc", "--limit", "10"], input=golden("q3.vdl"),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    assert "disjoint result rows" in r.stderr and "not built" in r.stderr


def test_vdlrun_checks_order_fields_against_the_program_without_a_device():
    r = subprocess.run([VDLRUN, "--describe", "--order-by", "nosuchfield"], input=golden("q3.vdl"), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "nosuchfield" in r.stderr
    r = subprocess.run([VDLRUN, "--describe", "--order-by", "revenue:desc,tmp115:asc", "--limit", "10"], input=golden("q3.vdl"), capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr


# ---- the build -------------------------------------------------------------------------------------------------------------------

ORDER_KERNELS = ["k_ord_minmax", "k_ord_hist", "k_ord_pick", "k_ord_close", "k_ord_stage", "k_ord_rank", "k_ord_gather", "k_ord_sortkey",
                 "k_ord_compose"]


def test_order_kernels_are_built_for_gfx950_and_their_resource_report_is_in_the_design():
    mk = open(os.path.join(ROOT, "mplan2vdl_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJ\s*:=.*vdl_order\.o", mk, flags=re.M) and "vdl_order.hip" in mk
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for k in ORDER_KERNELS:
        assert k.encode() in blob, k                  # the kernels' (mangled) names sit in the library's code object
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in ORDER_KERNELS:
        row = re.search(r"^\|\s*`?%s`?\s*\|(.*)$" % k, design, flags=re.M)
        assert row, "DESIGN.md has no resource row for " + k
        cells = [c.strip() for c in row.group(1).strip().strip("|").split("|")]
        assert len(cells) >= 5 and cells[3] == "0", (k, cells)        # VGPRs, SGPRs, LDS, scratch = 0, occupancy
