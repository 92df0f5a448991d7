"""Frame-of-reference column images without a GPU: the rules of csrc/vdl_column_image.h (width choice, range rewrite, factor
composition) against brute force under ASan + UBSan, and the specialised scans over the widths images have -- 1-, 2- and
4-byte columns, read with the tile and late in pairs -- built by hiprtc with their code size checked as test_jit.py does."""
import os
import re
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import datagen
from conftest import ROOT

CSRC = os.path.join(ROOT, "mplan2vdl_amd", "csrc")
# the image widths of the generated lineitem columns (vdl_column_image.h: choose over their min, max and decimal trailing zeros)
IMAGE_WIDTHS = {"lineitem.l_shipdate": 2, "lineitem.l_discount": 1, "lineitem.l_quantity": 1, "lineitem.l_extendedprice": 4,
                "lineitem.l_tax": 1, "lineitem.l_returnflag": 1, "lineitem.l_linestatus": 1}


def _build(tmp_path, sanitize):
    exe = str(tmp_path / ("column_image" + ("_asan" if sanitize else "")))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    cmd = ["g++", "-std=c++17", "-Wall"] + flags + ["-I", CSRC, os.path.join(ROOT, "tools", "sanitize", "column_image_main.cpp"), "-o", exe]
    return exe if subprocess.call(cmd) == 0 else None


def test_image_rules_match_brute_force_under_sanitizers(tmp_path):
    exe = _build(tmp_path, True) or _build(tmp_path, False)       # (a compiler without the sanitizer runtimes still checks the rules)
    assert exe, "the checker of vdl_column_image.h does not build"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 1000000


def test_generated_lineitem_columns_have_the_widths_the_rules_choose():
    """the widths IMAGE_WIDTHS assumes, from the generator's ranges (every row of a large column takes every value)"""
    for name, w in IMAGE_WIDTHS.items():
        s = datagen.LINEITEM[name]
        lo, hi = s.add + s.mul * s.lo, s.add + s.mul * s.hi
        pure = next(k for k in (1, 2, 4, 8) if -(1 << (8 * k - 1)) <= lo and hi < (1 << (8 * k - 1)))
        span = (hi - lo) // (s.mul if s.mul % 10 == 0 else 1)
        affine = next(k for k in (1, 2, 4, 8) if span < (1 << (8 * k - 1)))
        assert min(pure, affine) == w, name


def code_bytes(note):
    return [int(x) for x in re.findall(r"(\d+) B of code", note)]


def narrow_engine(names, n=60000):
    """columns declared at their image widths (no device: address, width, length only)"""
    e = m.Engine(device=None)
    for k in names:
        e.register_pointer(k, 0x10000, IMAGE_WIDTHS[k], n)
    return e


@pytest.mark.parametrize("query", ["q6", "q1"])
def test_specialised_scans_over_image_widths_build_without_a_gpu(query, tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    text = open(os.path.join(ROOT, "tests", "golden", query + ".vdl")).read()
    e = narrow_engine(datagen.Q6_COLUMNS if query == "q6" else datagen.Q1_COLUMNS)
    p = e.parse(text)
    note = p.jit_check()
    assert "k_mscan_specialised<" in note and code_bytes(note) and max(code_bytes(note)) < 64 << 10, note
    monkeypatch.setenv("VDL_JIT_ASSUME_SELECTIVITY", "0.2")
    # staged forms: one filter column with the tile (the 1-byte filter columns then read late in i8x2 pairs), every filter with the
    # tile (only the aggregate inputs late), and the census build of each
    for late in ("1", "2", "4"):
        monkeypatch.setenv("VDL_JIT_LATE", late)
        staged = p.jit_check()
        assert "(late)" in staged and max(code_bytes(staged)) < 64 << 10, (late, staged)
        monkeypatch.setenv("VDL_JIT_CENSUS", "1")
        census = p.jit_check()
        assert "(late)" in census and max(code_bytes(census)) < 96 << 10, (late, census)
        monkeypatch.delenv("VDL_JIT_CENSUS")
    monkeypatch.delenv("VDL_JIT_LATE")
    e.close()
