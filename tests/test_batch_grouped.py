"""Grouped batches on the GPU (Engine.set_batch_grouped + Engine.run_batch): plans whose one scan is a GROUP BY and that differ in
their literals alone are answered by ONE pass -- every row goes to the table of its pass class, the set of plans whose filters it
passes, and the classes are folded into the plans' tables once per block -- and every plan's results equal the oracle's for its own
text, bit for bit.

Every case pins 2 row pairs per lane (VDL_JIT_GROUP_U) and runs over byte images and over the columns themselves, at one row more
than a tile (1025) and at 37 tiles and 511 rows (several tiles per block, a partial one at the end).  group16 and its tables are
test_batch_grouped_cpu.py's; edge_group (256 groups: two plans fit, three do not) and Q1 (four plans at two replicas) those of
test_scan_forms.py / test_jit_bounds.py."""
import io
import json
import os
import re
import subprocess

import pytest

import test_batch_grouped_cpu as G
import test_jit_bounds as JB
import test_scan_forms as F
from mplan2vdl_amd import datagen
from conftest import golden
from helpers import lineitem, oracle_run
from test_batch_cpu import slots
from test_jit_bounds_cpu import changed
from test_pipe_end import VDLRUN, reference_shape

pytestmark = pytest.mark.gpu

U = 2
ROWS = {"1tile": F.tile(U) + 1, "37tiles": 37 * F.tile(U) + 511}
SHAPES = [(images, size) for images in (True, False) for size in ROWS]
IDS = ["%s-%s" % ("img" if images else "noimg", size) for images, size in SHAPES]
_cols, _want = {}, {}


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


@pytest.fixture
def pinned(jit_cache, monkeypatch):
    def pin(width=None):
        monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
        monkeypatch.setenv("VDL_JIT_GROUP_U", str(U))
        monkeypatch.delenv("VDL_JIT_PIN", raising=False)
        if width:
            monkeypatch.setenv("VDL_BATCH_WIDTH", str(width))
        else:
            monkeypatch.delenv("VDL_BATCH_WIDTH", raising=False)
    return pin


def table(n, oob=False):
    if (n, oob) not in _cols:
        _cols[(n, oob)] = G.columns(n, oob)
    return _cols[(n, oob)]


def wanted(n, bounds, oob=False):
    """the oracle's answer for one literal set of group16, computed once"""
    if (n, bounds, oob) not in _want:
        _want[(n, bounds, oob)] = oracle_run(G.group16(bounds), table(n, oob))
    return _want[(n, bounds, oob)]


def engine(cols, images):
    e = F.gpu_engine(cols, images)
    e.set_batch_grouped(True)
    return e


def parse_all(e, texts):
    plans = [e.parse(t) for t in texts]
    for p in plans:
        p.set_jit(True, runtime_bounds=True)                   # (run-time bounds: the plans that run alone share their code too)
    return plans


def results(replies):
    return [r["results"] for r in replies]


def check_kernel(notes, images, width):
    got = slots(notes)
    assert [(q, k) for _, q, k, _ in got] == [(q, width) for q in range(width)] and len({b for b, _, _, _ in got}) == 1, notes
    name = got[0][3]
    assert re.match(r"k_mscan_specialised<\d+,%d,(no)?vec,grouped" % U, name) and name.endswith(",batch%d,rtb>" % width), name
    assert (",img" in name) == images, name


def empty(res):
    return all(v == [] for entry in res.values() for v in entry.values())


def filled(res):
    return all(v for entry in res.values() for v in entry.values())


def test_group16_literal_sets_have_pairwise_different_answers():
    """giving every slot the bounds of slot 0 must fail: five sets, five answers, at both sizes"""
    for n in ROWS.values():
        want = [wanted(n, s) for s in G.SETS[:5]]
        assert len({json.dumps(w, sort_keys=True) for w in want}) == 5 and all(filled(w) for w in want)
        assert empty(wanted(n, G.EMPTY))


@pytest.mark.parametrize("images,size", SHAPES, ids=IDS)
@pytest.mark.parametrize("width", [2, 3, 4])
def test_group16_batches_of_two_three_and_four(width, images, size, pinned):
    pinned(width)
    n = ROWS[size]
    cols = table(n)
    sets = G.SETS[:width]
    want = [wanted(n, s) for s in sets]
    e = engine(cols, images)
    if images:
        assert e.image_info("t.g")[0] == 1 and e.image_info("t.f") == (1, G.B, 1000) and e.image_info("t.h") == (2, 0, 1)
    plans = parse_all(e, G.texts_of(sets))
    assert results(e.run_batch(plans)) == want
    check_kernel([p.batch_note() for p in plans], images, width)
    assert all(0 < p.batch_code_bytes() < 64 << 10 for p in plans)
    assert results(e.run_batch(plans[::-1])) == want[::-1]                 # the slots follow the call's order
    assert [s[1] for s in slots([p.batch_note() for p in plans])] == list(range(width))[::-1]
    e.close()


@pytest.mark.parametrize("images,size", SHAPES, ids=IDS)
def test_edge_group_is_a_batch_of_two_and_one_alone(images, size, pinned):
    """256 groups: three class tables fit LDS, seven do not; wrapping sums, MIN / MAX near the int64 ends and the FoldChoose key per slot"""
    pinned()
    n = ROWS[size]
    base, cols = JB.base_program("edge_group", n)
    texts = [changed(base, mp) for mp, _ in JB.VARIANTS["edge_group"][:3]]
    want = [JB.wanted("edge_group", n, k, t, cols) for k, t in enumerate(texts)]
    assert len({json.dumps(w, sort_keys=True) for w in want}) == 3
    e = engine(cols, images)
    plans = parse_all(e, texts)
    got = results(e.run_batch(plans))
    notes = [p.batch_note() for p in plans]
    assert got == want, notes
    check_kernel(notes[:2], images, 2)
    assert notes[2] == G.LEFT_OVER % 2
    e.close()


@pytest.mark.parametrize("images,size", SHAPES, ids=IDS)
def test_four_q1_cutoffs_share_one_pass(images, size, pinned):
    pinned()
    n = ROWS[size]
    base, cols = JB.base_program("q1", n)
    texts = [changed(base, {729999: 729999 - 60 * k}) if k else base for k in range(4)]
    want = [JB.wanted("q1_cutoff", n, k, t, cols) for k, t in enumerate(texts)]
    e = engine(cols, images)
    plans = parse_all(e, texts)
    got = results(e.run_batch(plans))
    notes = [p.batch_note() for p in plans]
    assert all(x.startswith("batch ") and ",grouped" in x for x in notes), notes
    assert got == want, notes
    assert all(0 < p.batch_code_bytes() < 64 << 10 for p in plans)
    e.close()


@pytest.mark.parametrize("images,size", SHAPES, ids=IDS)
def test_rows_outside_the_pivots_send_one_plan_back_alone(images, size, pinned):
    """g is 16..19 only where f's e is 122 or more: one slot's range reaches there, two slots' ranges do not"""
    pinned()
    n = ROWS[size]
    cols = table(n, oob=True)
    assert ((cols["t.g"] > 15) == (cols["t.f"] >= G.B + 1000 * G.OOB_FROM)).all() and (cols["t.g"] > 15).any()
    sets = [G.SETS[0], G.REACHES_OOB, G.SETS[1]]
    want = [wanted(n, s, oob=True) for s in sets]
    e = engine(cols, images)
    plans = parse_all(e, G.texts_of(sets))
    got = results(e.run_batch(plans))
    notes = [p.batch_note() for p in plans]
    assert notes[1].startswith("alone: rerun after batch 0: ") and "outside the Partition pivots" in notes[1], notes
    assert [(q, k) for _, q, k, _ in slots([notes[0], notes[2]])] == [(0, 3), (2, 3)], notes
    assert got == want
    assert plans[1].batch_code_bytes() == 0 and plans[0].batch_code_bytes() > 0
    e.close()


def test_the_rerun_plan_in_slot_zero_leaves_its_partners_their_timing(pinned):
    """every plan profiled, the plan that meets rows outside the pivots first: its partners carry the batch kernel's time (not 0), the
    rerun plan says that its fused plan was abandoned and carries no batch timing"""
    pinned()
    n = ROWS["37tiles"]
    cols = table(n, oob=True)
    sets = [G.REACHES_OOB, G.SETS[0], G.SETS[1]]
    want = [wanted(n, s, oob=True) for s in sets]
    e = engine(cols, True)
    plans = parse_all(e, G.texts_of(sets))
    for p in plans:
        p.set_profiling(True)
    got = e.run_batch(plans)
    assert results(got) == want
    assert plans[0].batch_note().startswith("alone: rerun after batch 0: ")
    for k in (1, 2):
        times = [v for label, v in got[k]["timings"].items() if "BatchedScan" in label]
        assert len(times) == 1 and times[0] > 0, got[k]["timings"]
    assert not any("BatchedScan" in label or "FusedScan" in label for label in got[0]["timings"]), got[0]["timings"]
    assert any(label.startswith("fusedPlanAbandoned: ") and "outside the Partition pivots" in label for label in got[0]["timings"]), got[0]["timings"]
    e.close()


@pytest.mark.parametrize("images,size", SHAPES, ids=IDS)
def test_edge_group_variants_of_other_shapes_run_alone(images, size, pinned):
    """all five variants in one call.  Over images variant 3 -- every bound one step outside an image: open sides -- has a shape no
    other plan has and runs alone with the words a global plan gets; over the columns themselves its bounds are ordinary ones.  Every
    plan is batched or alone, no batch is wider than 2, and every answer is the oracle's -- variant 4's range is empty"""
    pinned()
    n = ROWS[size]
    base, cols = JB.base_program("edge_group", n)
    texts = [changed(base, mp) for mp, _ in JB.VARIANTS["edge_group"]]
    want = [JB.wanted("edge_group", n, k, t, cols) for k, t in enumerate(texts)]
    e = engine(cols, images)
    plans = parse_all(e, texts)
    got = results(e.run_batch(plans))
    notes = [p.batch_note() for p in plans]
    for k in range(5):
        assert got[k] == want[k], (k, notes)
    assert empty(got[4]) and filled(got[3])
    batched = [x for x in notes if x.startswith("batch ")]
    assert all(k == 2 for _, _, k, _ in slots(batched)) and len(batched) % 2 == 0 and all(x.startswith("alone: ") for x in notes if x not in batched), notes
    if images:
        assert notes[3] == "alone: its filter shapes differ from every other plan's", notes
    e.close()


@pytest.mark.parametrize("images,size", SHAPES, ids=IDS)
def test_a_set_that_keeps_no_row_beside_two_that_do(images, size, pinned):
    pinned()
    n = ROWS[size]
    sets = [G.SETS[0], G.EMPTY, G.SETS[1]]
    want = [wanted(n, s) for s in sets]
    e = engine(table(n), images)
    plans = parse_all(e, G.texts_of(sets))
    got = results(e.run_batch(plans))
    assert got == want
    assert empty(got[1]) and filled(got[0]) and filled(got[2])
    check_kernel([p.batch_note() for p in plans], images, 3)
    e.close()


@pytest.mark.parametrize("images,size", SHAPES, ids=IDS)
def test_run_alone_afterwards_batch_again_and_timing(images, size, pinned):
    pinned()
    n = ROWS[size]
    sets = G.SETS[:3]
    want = [wanted(n, s) for s in sets]
    e = engine(table(n), images)
    plans = parse_all(e, G.texts_of(sets))
    plans[0].set_profiling(True)
    first = e.run_batch(plans)
    assert results(first) == want
    labels = list(first[0]["timings"])
    assert len(labels) == 1 and labels[0].startswith("timeInMicrosecondsForBatchedScan_k_mscan_specialised<") and ",grouped" in labels[0] and \
        labels[0].endswith(",batch3,rtb>"), labels
    assert first[1]["timings"] == {}
    for k in (1, 2, 0):
        assert plans[k].batch_note().startswith("batch 0: slot %d of 3" % k)
        assert plans[k].run()["results"] == want[k]
        assert plans[k].batch_note() == "" and plans[k].batch_code_bytes() == 0
    assert results(e.run_batch(plans)) == want                  # the batch again, after the plans were bound for themselves
    assert [p.batch_note()[:21] for p in plans] == ["batch 0: slot %d of 3," % k for k in range(3)]
    e.close()


def test_vdlrun_batch_grouped_end_to_end(tmp_path):
    """`vdlrun --jit --batch-grouped --batch FILE --batch FILE` over Q1: three reply lines equal to the oracle's; without the flag the
    notes say what they always said"""
    rows = 5000
    texts = [changed(golden("q1.vdl"), {729999: 729999 - 60 * k}) if k else golden("q1.vdl") for k in range(3)]
    args = [VDLRUN, "--jit", "--rows", str(rows)]
    for k in (1, 2):
        path = tmp_path / ("q1_%d.vdl" % k)
        path.write_text(texts[k])
        args += ["--batch", str(path)]
    r = subprocess.run(args + ["--batch-grouped"], input=texts[0].encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 3
    cols = lineitem(datagen.Q1_COLUMNS, rows)
    want = [oracle_run(t, cols) for t in texts]
    assert len({json.dumps(w, sort_keys=True) for w in want}) == 3
    for k, line in enumerate(lines):
        reply = json.load(io.StringIO(line))
        reference_shape(reply["results"])
        assert reply["results"] == want[k], k
    notes = re.findall(r"vdlrun: batch: (.*)", r.stderr.decode())
    assert [(q, k) for _, q, k, _ in slots(notes)] == [(0, 3), (1, 3), (2, 3)] and all(",grouped" in x for x in notes), r.stderr.decode()[-2000:]
    off = subprocess.run(args, input=texts[0].encode(), capture_output=True, timeout=600)
    assert off.returncode == 0 and off.stdout.decode().splitlines() == lines
    assert re.findall(r"vdlrun: batch: (.*)", off.stderr.decode()) == ["alone: grouped scans are not batched"] * 3
