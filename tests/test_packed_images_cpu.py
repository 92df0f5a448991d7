"""Bit-packed column images without a GPU: the rules of csrc/vdl_column_image.h (bit width, range mapping onto [0, 2^bits - 1],
factor composition, the stripe layout) against brute force under ASan + UBSan, the layout's index math against a numpy packer, and
the packed form of the specialised global aggregate scan built by hiprtc over declared packed columns for every bit width."""
import os
import re
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import datagen
from conftest import ROOT

CSRC = os.path.join(ROOT, "mplan2vdl_amd", "csrc")
STRIPE, LANES, VALUES = 2048, 64, 32


def pack_numpy(e, bits):
    """the packed image (uint32 dwords) of stored values e' (non-negative, < 2^bits) in lane-transposed stripes of 2048 rows: row
    2048 s + 64 j + l is value j of lane l; lane l's 32 values are a bit stream of `bits` dwords, dword k at (s bits + k) 64 + l"""
    e = np.asarray(e, dtype=np.uint64)
    stripes = (len(e) + STRIPE - 1) // STRIPE
    v = np.zeros(stripes * STRIPE, dtype=np.uint64)
    v[:len(e)] = e
    v = v.reshape(stripes, VALUES, LANES)                       # [s][j][l]
    words = np.zeros((stripes, bits, LANES), dtype=np.uint64)
    for j in range(VALUES):
        o = j * bits
        k, sh = o // 32, o % 32
        words[:, k, :] |= (v[:, j, :] << np.uint64(sh)) & np.uint64(0xFFFFFFFF)
        if sh + bits > 32:
            words[:, k + 1, :] |= v[:, j, :] >> np.uint64(32 - sh)
    return words.reshape(-1).astype(np.uint32)


def unpack_naive(words, bits, n):
    """row by row, bit by bit, from the layout's index math as written in include/vdl.h"""
    out = np.zeros(n, dtype=np.int64)
    for i in range(n):
        s, j, l = i // STRIPE, (i % STRIPE) // LANES, i % LANES
        x = 0
        for b in range(bits):
            pos = j * bits + b
            dw = (s * bits + pos // 32) * LANES + l
            x |= ((int(words[dw]) >> (pos % 32)) & 1) << b
        out[i] = x
    return out


def _build(tmp_path, sanitize):
    exe = str(tmp_path / ("packed_image" + ("_asan" if sanitize else "")))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    cmd = ["g++", "-std=c++17", "-Wall"] + flags + ["-I", CSRC, os.path.join(ROOT, "tools", "sanitize", "packed_image_main.cpp"), "-o", exe]
    return exe if subprocess.call(cmd) == 0 else None


def test_packed_rules_match_brute_force_under_sanitizers(tmp_path):
    exe = _build(tmp_path, True) or _build(tmp_path, False)
    assert exe, "the checker of the packed rules in vdl_column_image.h does not build"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 1000000


@pytest.mark.parametrize("bits", range(1, 33))
def test_numpy_packer_follows_the_layout(bits):
    """every value comes back from the documented index math; the image is whole stripes, zero past the last row"""
    r = np.random.default_rng(bits)
    n = STRIPE + 2 * LANES + 5
    e = r.integers(0, 1 << bits, n, dtype=np.uint64)
    e[:2] = [0, (1 << bits) - 1]
    words = pack_numpy(e, bits)
    assert len(words) == 2 * bits * LANES
    assert (unpack_naive(words, bits, n) == e.astype(np.int64)).all()
    assert (unpack_naive(words, bits, 2 * STRIPE)[n:] == 0).all()


# the byte-image widths of the generated Q6 columns (test_column_images_cpu.py) and their packed images at SF100 (bits, base, scale)
Q6_WIDTHS = {"lineitem.l_shipdate": 2, "lineitem.l_discount": 1, "lineitem.l_quantity": 1, "lineitem.l_extendedprice": 4}
Q6_PACKED = {"lineitem.l_shipdate": (12, 727564, 1), "lineitem.l_discount": (4, 0, 1), "lineitem.l_quantity": (6, 100, 100),
             "lineitem.l_extendedprice": (24, 90091, 1)}


def test_generated_q6_columns_have_the_packed_images_the_rules_choose():
    for name, (bits, base, scale) in Q6_PACKED.items():
        s = datagen.LINEITEM[name]
        lo, hi = s.add + s.mul * s.lo, s.add + s.mul * s.hi
        step = s.mul if s.mul % 10 == 0 else 1
        assert (lo, step) == (base, scale), name
        assert ((hi - lo) // step).bit_length() == bits and bits < 8 * Q6_WIDTHS[name], name


def code_bytes(note):
    return [int(x) for x in re.findall(r"(\d+) B of code", note)]


def packed_engine(cols, widths, bits, packed_base=None):
    """columns declared (no device) at `widths`, each with a packed image of `bits` bits"""
    e = m.Engine(device=None)
    for k, n in cols.items():
        e.register_pointer(k, 0x10000, widths[k], n)
        base, scale = (packed_base or {}).get(k, (0, 1))
        e.declare_packed(k, bits, base, scale)
    return e


def q6():
    return open(os.path.join(ROOT, "tests", "golden", "q6.vdl")).read()


def edge():
    from test_scan_forms import program
    text, cols = program("edge_global", 5000)
    return text, {k: len(v) for k, v in cols.items()}, {k: v.dtype.itemsize for k, v in cols.items()}


def test_q6_is_not_refused_the_packed_form(tmp_path, monkeypatch):
    """Q6 over its SF100 packed images: both packed forms build, name the packed columns with their bits, and are not refused"""
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    e = m.Engine(device=None)
    for k in datagen.Q6_COLUMNS:
        e.register_pointer(k, 0x10000, Q6_WIDTHS[k], 600000)
        e.declare_packed(k, *Q6_PACKED[k])
    p = e.parse(q6())
    monkeypatch.setenv("VDL_JIT_LATE", "5")
    note = p.jit_check()
    assert "not specialised" not in note, note
    assert "k_mscan_specialised<4,2,vec,global,img,packed,late> (packed: l_discount:4 l_quantity:6 l_shipdate:12) (late)" in note, note
    monkeypatch.setenv("VDL_JIT_LATE", "6")
    note = p.jit_check()
    assert "not specialised" not in note, note
    assert "k_mscan_specialised<4,2,vec,global,img,packed> (packed: l_discount:4 l_quantity:6 l_shipdate:12 l_extendedprice:24)" in note, note
    e.close()


@pytest.mark.parametrize("bits", range(1, 33))
def test_packed_forms_build_for_every_bit_width(bits, tmp_path, monkeypatch):
    """Q6 (filters packed, the price late; and its census build) and edge_global (every column packed) over declared packed images
    of `bits` bits: built by hiprtc, under 64 KB of code (census: 96 KB)"""
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    e = packed_engine({k: 600000 for k in datagen.Q6_COLUMNS}, Q6_WIDTHS, bits,
                      {k: (base, scale) for k, (_, base, scale) in Q6_PACKED.items()})
    p = e.parse(q6())
    monkeypatch.setenv("VDL_JIT_LATE", "5")
    note = p.jit_check()
    assert ",packed,late>" in note and code_bytes(note) and max(code_bytes(note)) < 64 << 10, (bits, note)
    monkeypatch.setenv("VDL_JIT_CENSUS", "1")
    note = p.jit_check()
    assert ",packed,late>" in note and max(code_bytes(note)) < 96 << 10, (bits, note)
    monkeypatch.delenv("VDL_JIT_CENSUS")
    e.close()
    text, ns, widths = edge()
    e = packed_engine(ns, widths, bits)
    p = e.parse(text)
    monkeypatch.setenv("VDL_JIT_LATE", "6")
    note = p.jit_check()
    assert ",packed>" in note and max(code_bytes(note)) < 64 << 10, (bits, note)
    assert re.search(r"\(packed: (\S+:%d ?){7}\)" % bits, note), (bits, note)
    e.close()


def test_packed_form_is_refused_outside_global_scans_over_table_columns(tmp_path, monkeypatch):
    """grouped scans (Q1) are refused the packed form, and say why"""
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    widths = {"lineitem.l_shipdate": 2, "lineitem.l_discount": 1, "lineitem.l_quantity": 1, "lineitem.l_extendedprice": 4,
              "lineitem.l_tax": 1, "lineitem.l_returnflag": 1, "lineitem.l_linestatus": 1}
    e = packed_engine({k: 60000 for k in datagen.Q1_COLUMNS}, widths, 8)
    p = e.parse(open(os.path.join(ROOT, "tests", "golden", "q1.vdl")).read())
    monkeypatch.setenv("VDL_JIT_LATE", "5")
    note = p.jit_check()
    assert "not specialised (the packed form serves global aggregate scans only, not grouped scans)" in note, note
    e.close()
