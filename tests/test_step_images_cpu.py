"""Step images without a GPU (vdl_column_image.h Steps): a step image declared on a device-less engine makes Q3's front build in the
form that decodes it (",stp"), still folded; the same plan without the declaration does not; the pipe end takes --encode-steps; and
the ingest kernel is in the library's gfx950 code object."""
import os
import re
import struct
import subprocess

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib, datagen
from mplan2vdl_amd._lib import parse_step_columns
from conftest import ROOT, golden

VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
JOIN_INDEX = "lineitem.lineitem_orders"
# Q3's columns as the scans meet them at SF100: byte-image widths for the columns nobody filters (a filtered column keeps its catalog
# width here -- its image has a base, which a declared pointer cannot carry, and the plan's dates do not fit 2 bytes without it),
# and the join index at 4 bytes: 150 M orders
NARROW = {"lineitem.l_discount": 1, "lineitem.l_extendedprice": 4, "lineitem.l_orderkey": 4, "orders.o_shippriority": 1,
          "orders.orders_customer": 4, "customer.c_mktsegment": 1, JOIN_INDEX: 4}
CODE_LIMIT = 64 << 10                        # tests/test_jit.py: a descriptor that did not fold is several times this


def code_bytes(note):
    return [int(x) for x in re.findall(r"(\d+) B of code", note)]


def declared_q3(steps, base=40000):
    e = m.Engine(device=None)
    for k, v in datagen.q3_tables(5000).items():
        if k in datagen.Q3_COLUMNS:
            e.register_pointer(k, 0x10000, NARROW.get(k, v.dtype.itemsize), len(v))
    if steps:
        e.declare_steps(JOIN_INDEX, base)
    return e


def front_line(note):
    line = [x for x in note.split("; ") if x.startswith("front: ")]
    assert len(line) == 1 and "not specialised" not in line[0], note
    return line[0]


def test_step_column_lists_parse():
    assert parse_step_columns("") == {}
    assert parse_step_columns("front.select: lineitem.lineitem_orders:s; front.take: lineitem.lineitem_orders:s a.b:s") == {
        "front.select": [JOIN_INDEX], "front.take": [JOIN_INDEX, "a.b"]}


def test_a_declared_step_image_builds_the_front_that_decodes_it(tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    e = declared_q3(steps=True)
    assert e.steps_info(JOIN_INDEX) == (True, 40000, (4 * 5000 + 63) // 64)
    p = e.parse(golden("q3.vdl"))
    note = p.jit_check()
    assert ",stp" in front_line(note), note
    assert code_bytes(note) and max(code_bytes(note)) < CODE_LIMIT, note          # the descriptor still folds
    steps, images = p.step_columns(), p.image_columns()
    assert JOIN_INDEX in steps.get("front.select", []) and JOIN_INDEX in steps.get("front.take", []), steps
    assert all(JOIN_INDEX not in cols for cols in images.values()), images
    # ... with run-time bounds too
    p.set_jit(False, runtime_bounds=True)
    note = p.jit_check()
    assert ",stp,rtb>" in front_line(note) and max(code_bytes(note)) < CODE_LIMIT, note
    # leaving the step images unbound gives the front it was
    e.set_step_images(False)
    p.set_jit(False, runtime_bounds=False)
    note = p.jit_check()
    assert ",stp" not in note and p.step_columns() == {}, (note, p.step_columns())
    e.close()


def test_the_same_plan_without_the_declaration_has_no_step_form(tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    e = declared_q3(steps=False)
    assert e.steps_info(JOIN_INDEX) == (False, 0, 0)
    p = e.parse(golden("q3.vdl"))
    note = p.jit_check()
    assert ",stp" not in note and "front: " in note, note
    assert p.step_columns() == {}
    e.close()


def test_step_images_are_declared_only_without_a_device_and_on_known_columns():
    import pytest

    e = m.Engine(device=None)
    with pytest.raises(m.VdlError):
        e.declare_steps("no.such_column", 0)
    e.register_pointer("t.empty", 0x10000, 8, 0)
    with pytest.raises(m.VdlError):
        e.declare_steps("t.empty", 0)                     # a step image needs a first row
    with pytest.raises(m.VdlError):
        e.encode_steps("t.empty")                         # building one needs a device
    e.close()


def test_vdlrun_describe_accepts_encode_steps():
    text = golden("q3.vdl")
    r = subprocess.run([VDLRUN, "--describe", "--encode-steps"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run([VDLRUN, "--describe"], input=text, capture_output=True, text=True, timeout=60)
    assert r.stdout == plain.stdout and "fused front" in r.stdout


def bundle_entries(blob):
    """[(target id, bytes)] of every clang offload bundle inside `blob`"""
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, at = [], blob.find(magic)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", blob, at + len(magic))
        pos = at + len(magic) + 8
        for _ in range(count):
            off, size, idlen = struct.unpack_from("<QQQ", blob, pos)
            ident = blob[pos + 24:pos + 24 + idlen].decode()
            out.append((ident, blob[at + off:at + off + size]))
            pos += 24 + idlen
        at = blob.find(magic, at + len(magic))
    return out


def test_the_ingest_kernel_is_in_the_gfx950_code_object():
    blob = open(_lib.LIB_PATH, "rb").read()
    device = [code for ident, code in bundle_entries(blob) if ident.endswith("gfx950")]
    assert device, "no gfx950 code object in the library"
    assert any(b"k_image_steps" in code and code[:4] == b"\x7fELF" for code in device)
