"""Bit-packed column images on the GPU: the bytes the ingest pass writes against a numpy packer for every bit width, the packed form
of the specialised global aggregate scan (forced) against the oracle at stripe edges, under a row offset, and with images off, and
its census against a numpy count of the lines it reads."""
import os
import re

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import datagen
from conftest import ROOT
from helpers import oracle_run
from test_packed_images_cpu import pack_numpy
from test_scan_forms import BOUNDS, edge_global, program

STRIPE = 2048
SIZES = [1, 63, 2047, 2048, 2049, 37 * 2048 + 1999]
PACKED_FORMS = (5, 6)                     # VDL_JIT_LATE: filter columns packed + aggregate inputs late; every column packed


def q6_text():
    return open(os.path.join(ROOT, "tests", "golden", "q6.vdl")).read()


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


def span_column(bits, n, seed):
    """an int64 column of negative values base + 10 e with e over exactly [0, 2^bits - 1]: its byte image is affine (scale 10)"""
    r = np.random.default_rng(seed)
    e = r.integers(0, 1 << bits, n, dtype=np.int64)
    e[:2] = [0, (1 << bits) - 1]
    return np.int64(-7000000003) + np.int64(10) * e, e


@pytest.mark.gpu
def test_packed_bytes_match_the_numpy_packer_for_every_bit_width():
    """bits 1..31: the packed image of a column spanning exactly 2^bits - 1 steps is the numpy packer's, its base is the column's
    minimum and its scale the byte image's.  32 bits: no byte image is wider than 4 bytes and a packed image must be narrower
    than its byte image, so a 32-bit span has none (the 32-bit form is built over declared images in test_packed_images_cpu.py)"""
    e = m.Engine(device=0)
    n = 3 * STRIPE + 77
    for bits in range(1, 33):
        name = "t.b%d" % bits
        v, stored = span_column(bits, n, bits)
        e.upload(name, v)
        e.encode(name)
        pb, pbase, pscale = e.packed_info(name)
        if bits == 32:                                          # (a span of 2^32 - 1 steps has no byte image either)
            assert pb == 0, (bits, e.image_info(name), e.packed_info(name))
            continue
        w, base, scale = e.image_info(name)
        assert scale == 10 and base == int(v.min()), (bits, e.image_info(name))
        assert (pb, pbase, pscale) == (bits, int(v.min()), 10), (bits, e.packed_info(name))
        got = e.download_packed(name)
        want = pack_numpy(stored, bits)
        assert got.shape == want.shape and np.array_equal(got, want), bits
        e.drop(name)
    e.close()


def run_forced(e, text, late, row_offset=0):
    """one run with the packed form forced (VDL_JIT_LATE=5 | 6 and set_jit without tuning): (results, note)"""
    os.environ["VDL_JIT_LATE"] = str(late)
    try:
        p = e.parse(text)
        if row_offset:
            p.set_row_offset(row_offset)
        p.set_jit(True)
        res = p.run()
        note = p.jit_note()
        p.close()
    finally:
        del os.environ["VDL_JIT_LATE"]
    return res["results"], note


def gpu_engine(cols):
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
    return e


def q6_columns(n, seed):
    """Q6's columns over n rows, with rows that pass its filters spread through the table and the last row passing"""
    cols = {k: datagen.generate(datagen.LINEITEM[k], 0, n, seed=seed) for k in datagen.Q6_COLUMNS}
    r = np.random.default_rng(seed)
    keep = r.random(n) < 0.2
    keep[-1] = True
    cols["lineitem.l_shipdate"][keep] = r.integers(728294, 728659, int(keep.sum())).astype(cols["lineitem.l_shipdate"].dtype)
    cols["lineitem.l_discount"][keep] = r.integers(5, 8, int(keep.sum()))
    cols["lineitem.l_quantity"][keep] = 100 * r.integers(1, 24, int(keep.sum()))
    return cols


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_q6_packed_form_matches_the_oracle(n, jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    text = q6_text()
    cols = q6_columns(n, 100 + n)
    want = oracle_run(text, cols)
    e = gpu_engine(cols)
    for late in PACKED_FORMS:
        got, note = run_forced(e, text, late)
        assert re.search(r",img,packed(,late)?>", note), (n, late, note)
        assert got == want, (n, late, note)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_edge_global_packed_form_matches_the_oracle(n, jit_cache, monkeypatch):
    """the edge table's global program (bound set 0) with the packed form forced: where a filter column has no packed image (w8
    has no image at all) the form is refused and the scan runs unpacked, with the same answer"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    text, cols = program("edge_global", n)
    want = oracle_run(text, cols)
    e = gpu_engine(cols)
    for late in PACKED_FORMS:
        got, note = run_forced(e, text, late)
        assert got == want, (n, late, note)
        if late == 5:
            assert ",img,packed,late>" in note, (n, note)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bounds", range(len(BOUNDS)))
def test_packed_filters_at_the_domain_ends_match_the_oracle(bounds, jit_cache, monkeypatch):
    """bounds below the minimum, above the maximum, single values and empty ranges (the bound sets of test_scan_forms.py)"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    n = 37 * STRIPE + 1999
    _, cols = program("edge_global", n)
    text = edge_global(bounds)
    want = oracle_run(text, cols)
    e = gpu_engine(cols)
    for late in PACKED_FORMS:
        got, note = run_forced(e, text, late)
        assert got == want, (bounds, late, note)
    e.close()


@pytest.mark.gpu
def test_q6_packed_form_over_generated_rows(jit_cache, monkeypatch):
    """4096 stripes and 3 rows, generated on the device (packed at ingest), in both packed forms and tuned"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    n = 4096 * STRIPE + 3
    text = q6_text()
    e = m.Engine(device=0)
    for k in datagen.Q6_COLUMNS:
        e.generate(datagen.LINEITEM[k], 0, n)
    assert e.packed_info("lineitem.l_shipdate") == (12, 727564, 1)
    assert e.packed_info("lineitem.l_discount") == (4, 0, 1)
    assert e.packed_info("lineitem.l_quantity") == (6, 100, 100)
    want = oracle_run(text, {k: e.download(k) for k in datagen.Q6_COLUMNS})
    for late in PACKED_FORMS:
        got, note = run_forced(e, text, late)
        assert ",packed" in note and got == want, (late, note)
    monkeypatch.setenv("VDL_JIT_PACKED", "only")
    p = e.parse(text)
    p.set_jit(True, tune=True)
    got = p.run()["results"]
    note = p.jit_note()
    p.close()
    assert re.search(r"tuned:[^;]*-> k_mscan_specialised<[^>]*,img,packed(,late)?> \(packed: ", note), note
    assert got == want, note
    e.close()


@pytest.mark.gpu
def test_row_offset_and_images_off(jit_cache, monkeypatch):
    """a rank's shard (row offset: the packed image starts at the shard's first row) gives the oracle's answer; with images off no
    packed form exists and the scan reads the catalog columns"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    n = 5 * STRIPE + 321
    text = q6_text()
    cols = q6_columns(n, 7)
    want = oracle_run(text, cols)
    e = gpu_engine(cols)
    for late in PACKED_FORMS:
        got, note = run_forced(e, text, late, row_offset=123457)
        assert ",packed" in note and got == want, (late, note)
    e.set_column_images(False)
    for late in PACKED_FORMS:
        got, note = run_forced(e, text, late)
        assert got == want, (late, note)
        assert ",packed" not in note and ",img" not in note and "column images are off" in note, note
    monkeypatch.setenv("VDL_JIT_PACKED", "only")
    p = e.parse(text)
    p.set_jit(True, tune=True)
    got = p.run()["results"]
    note = p.jit_note()
    p.close()
    assert got == want and ",packed" not in note, note
    e.close()


@pytest.mark.gpu
def test_packed_census_counts_the_packed_bytes_and_the_late_lines(jit_cache, monkeypatch):
    """vdl_plan_scan_traffic of the packed form: every packed image in whole stripes (padding included), plus 128 B per line of the
    price's 4-byte image (32 rows) in which a row passes every filter"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    n = 301 * STRIPE + 1001
    text = q6_text()
    e = m.Engine(device=0)
    for k in datagen.Q6_COLUMNS:
        e.generate(datagen.LINEITEM[k], 0, n)
    cols = {k: e.download(k) for k in datagen.Q6_COLUMNS}
    os.environ["VDL_JIT_LATE"] = "5"
    try:
        p = e.parse(text)
        p.set_jit(True)
        assert p.run()["results"] == oracle_run(text, cols)
        moved, detail = p.scan_traffic()
        note = p.jit_note()
        p.close()
    finally:
        del os.environ["VDL_JIT_LATE"]
    assert ",packed,late>" in note, note
    d, disc, q = (cols["lineitem." + c] for c in ("l_shipdate", "l_discount", "l_quantity"))
    live = (d >= 728294) & (d <= 728658) & (disc >= 5) & (disc <= 7) & (q < 2400)
    stripes = (n + STRIPE - 1) // STRIPE
    eager = sum(stripes * 64 * e.packed_info(k)[0] * 4 for k in ("lineitem.l_shipdate", "lineitem.l_discount", "lineitem.l_quantity"))
    padded = np.zeros((n + 31) // 32 * 32, dtype=bool)
    padded[:n] = live
    late = 128 * int(padded.reshape(-1, 32).any(axis=1).sum())
    print("census", moved, "numpy", eager + late, detail)
    assert moved == eager + late, (moved, eager, late, detail)
    e.close()
