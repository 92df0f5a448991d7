"""Batched runs on the GPU (Engine.run_batch, vdl_run_batch): plans that differ in their literals alone are answered by ONE pass
over the columns -- one kernel that tests every tile against each plan's bounds, with a count and accumulators per plan -- and every
plan's results equal the oracle's for its own text, bit for bit.

Every case pins one form the batch kernel has (VDL_JIT_PIN: the eager tile form, over byte images and over the columns themselves,
and the every-column packed form) at the smallest row counts at which its tile logic branches: one row more than a tile or a
stripe, and 37 tiles or stripes and 511 rows (several tiles per block, a partial one at the end).  The programs and their variants
are those of test_scan_forms.py / test_jit_bounds.py: the global edge program (wrapping sums, MIN / MAX near the int64 ends, bounds
at the ends of the images, ranges that are empty in an image's domain) and Q6 with its date, discount and quantity constants
shifted inside the columns' domains."""
import io
import json
import os
import re
import subprocess

import pytest

import mplan2vdl_amd as m
import test_jit_bounds as JB
import test_scan_forms as F
from mplan2vdl_amd import datagen, resolve
from conftest import ROOT, golden
from helpers import lineitem, oracle_run
from test_batch_cpu import NOTE, literal_set, slots
from test_jit_bounds_cpu import changed
from test_pipe_end import META, VDLRUN, reference_shape

pytestmark = pytest.mark.gpu

# (u, late, images): eager over byte images and over the columns themselves, every column packed
FORMS = [(2, 0, True), (2, 0, False), (2, 6, True)]
CASES = [(f, big) for f in FORMS for big in (False, True)]
IDS = ["u%d%s%s-%s" % (u, "_packed" if late else "_eager", "" if images else "_noimg", "37tiles" if big else "1tile") for (u, late, images), big in CASES]
EMPTY = (5, 6)                     # edge_global's variants whose range is empty in an image's domain


def rows_of(u, late, big):
    return JB.rows_of(u, late)[1 if big else 0]


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


@pytest.fixture
def pinned(jit_cache, monkeypatch):
    def pin(u, late):
        monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
        monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % (u, late))
        monkeypatch.setenv("VDL_JIT_ASSUME_SELECTIVITY", "0.3")
    return pin


def parse_all(e, texts):
    plans = [e.parse(t) for t in texts]
    for p in plans:
        p.set_jit(True, tune=True, runtime_bounds=True)        # (run-time bounds: the plans that run alone share their code too)
    return plans


def results(replies):
    return [r["results"] for r in replies]


def check_kernel(notes, u, late, images, width):
    """the notes name one batch of `width` slots in order, run by the pinned form"""
    got = slots(notes)
    assert [(q, k) for _, q, k, _ in got] == [(q, width) for q in range(width)] and len({b for b, _, _, _ in got}) == 1, notes
    name = got[0][3]
    assert re.match(r"k_mscan_specialised<\d+,%d,(no)?vec,global" % u, name), name
    assert (",packed,batch" in name) == (late == 6) and (",img" in name) == images, name


def built():
    c = m.jit_counters()
    return c["compiled"] + c["from_disk"]


@pytest.mark.parametrize("form,big", CASES, ids=IDS)
def test_edge_global_variants_share_a_batch_of_four(form, big, pinned):
    """variants 0-3 have one shape: one batch of 4 (seven words per slot cap the width at 4), every answer its own"""
    u, late, images = form
    pinned(u, late)
    n = rows_of(u, late, big)
    base, cols = JB.base_program("edge_global", n)
    texts = [changed(base, mp) for mp, _ in JB.VARIANTS["edge_global"][:4]]
    want = [JB.wanted("edge_global", n, k, t, cols) for k, t in enumerate(texts)]
    assert len({json.dumps(w, sort_keys=True) for w in want}) == 4          # a kernel that gave every slot slot 0's bounds would fail
    e = F.gpu_engine(cols, images)
    plans = parse_all(e, texts)
    assert results(e.run_batch(plans)) == want
    check_kernel([p.batch_note() for p in plans], u, late, images, 4)
    assert results(e.run_batch(plans[::-1])) == want[::-1]                 # the slots follow the call's order
    e.close()


@pytest.mark.parametrize("form,big", CASES, ids=IDS)
def test_edge_global_mixed_shapes_in_one_call(form, big, pinned):
    """all nine variants: several shapes (bounds clamped at an image's end are open sides), so several batches and plans that run
    alone, in one call; the variants with an empty range return no row while their neighbours return theirs"""
    u, late, images = form
    pinned(u, late)
    n = rows_of(u, late, big)
    base, cols = JB.base_program("edge_global", n)
    texts = [changed(base, mp) for mp, _ in JB.VARIANTS["edge_global"]]
    want = [JB.wanted("edge_global", n, k, t, cols) for k, t in enumerate(texts)]
    e = F.gpu_engine(cols, images)
    plans = parse_all(e, texts)
    got = results(e.run_batch(plans))
    notes = [p.batch_note() for p in plans]
    for k in range(len(texts)):
        assert got[k] == want[k], (k, notes[k])
    for k in EMPTY:
        assert all(v == [] for entry in got[k].values() for v in entry.values()), (k, got[k])
    for k in (EMPTY[0] - 1, EMPTY[-1] + 1):
        assert all(v for entry in got[k].values() for v in entry.values()), (k, got[k])
    batched = [x for x in notes if NOTE.match(x)]
    alone = [x for x in notes if x.startswith("alone: ")]
    assert len(batched) + len(alone) == len(notes), notes
    assert len({NOTE.match(x).group(1) for x in batched}) >= 2 and alone, notes
    assert all(int(NOTE.match(x).group(3)) <= 4 for x in batched), notes
    by_batch = {}
    for x in batched:
        mo = NOTE.match(x)
        by_batch.setdefault(mo.group(1), []).append((int(mo.group(2)), int(mo.group(3))))
    assert all(v == [(q, len(v)) for q in range(len(v))] for v in by_batch.values()), notes
    e.close()


@pytest.mark.parametrize("form,big", CASES, ids=IDS)
@pytest.mark.parametrize("width", [2, 3, 8])
def test_q6_literal_sets(width, form, big, pinned):
    u, late, images = form
    pinned(u, late)
    n = rows_of(u, late, big)
    base, cols = JB.base_program("q6", n)
    texts = [changed(base, literal_set(k)) for k in range(width)]
    want = [JB.wanted("q6_batch", n, k, t, cols) for k, t in enumerate(texts)]
    assert len({json.dumps(w, sort_keys=True) for w in want}) == width       # pairwise different: slot 0's bounds in every slot must fail
    e = F.gpu_engine(cols, images)
    plans = parse_all(e, texts)
    assert results(e.run_batch(plans)) == want
    check_kernel([p.batch_note() for p in plans], u, late, images, width)
    e.close()


def test_repeat_run_alone_afterwards_order_and_timing(pinned):
    u, late = 2, 0
    pinned(u, late)
    n = rows_of(u, late, True)
    base, cols = JB.base_program("q6", n)
    texts = [changed(base, literal_set(k)) for k in range(3)]
    want = [JB.wanted("q6_batch", n, k, t, cols) for k, t in enumerate(texts)]
    e = F.gpu_engine(cols, True)
    plans = parse_all(e, texts)
    field = next(iter(next(iter(want[2].values())))).lstrip(".")
    plans[2].set_order([(field, True)], limit=1)
    plans[0].set_profiling(True)
    first = e.run_batch(plans)
    second = e.run_batch(plans)
    assert results(first) == want and results(second) == want
    # one timing per profiled plan of the batch, under a label that is not the per-query one
    labels = list(first[0]["timings"])
    assert len(labels) == 1 and labels[0].startswith("timeInMicrosecondsForBatchedScan_k_mscan_specialised<") and ",batch3,rtb>" in labels[0], labels
    assert first[1]["timings"] == {} and not any("FusedScan" in k for r in first for k in r["timings"])
    assert plans[2].order_note().startswith("host m=1 rows=1"), plans[2].order_note()
    assert plans[0].order_note() == ""
    # a plan of a finished batch, run on its own: its own answer, through its own kernel, and no batch note
    for k in (1, 2, 0):
        assert plans[k].batch_note().startswith("batch 0: slot %d of 3" % k)
        assert plans[k].run()["results"] == want[k]
        assert plans[k].batch_note() == ""
    assert "FusedScan" in "".join(plans[0].run()["timings"])
    assert results(e.run_batch(plans)) == want                  # and the batch again, after the plans were bound for themselves
    assert [p.batch_note()[:21] for p in plans] == ["batch 0: slot %d of 3," % k for k in range(3)]
    e.close()


@pytest.mark.parametrize("late", [0, 6])
def test_a_second_batch_of_the_same_shape_compiles_nothing(late, pinned):
    u = 2
    pinned(u, late)
    n = rows_of(u, late, False)
    base, cols = JB.base_program("q6", n)
    e = F.gpu_engine(cols, True)
    first = parse_all(e, [changed(base, literal_set(k)) for k in range(3)])
    e.run_batch(first)
    before = built()
    texts = [changed(base, literal_set(k)) for k in (5, 7, 6)]
    later = parse_all(e, texts)
    got = results(e.run_batch(later))
    assert built() == before, m.jit_counters()
    assert got == [oracle_run(t, cols) for t in texts]
    assert [NOTE.match(p.batch_note()).group(4) for p in later] == [NOTE.match(p.batch_note()).group(4) for p in first]
    e.close()


def test_a_plan_that_cannot_share_runs_alone_in_the_same_call(pinned):
    """Q6 with specialisation off and Q6 with a one-sided date range beside two Q6s that batch: four answers from one call"""
    from test_jit_bounds_cpu import SHAPES
    pinned(2, 0)
    n = rows_of(2, 0, False)
    base, cols = JB.base_program("q6", n)
    texts = [changed(base, literal_set(0)), changed(base, literal_set(3)), changed(base, SHAPES["one_sided"]), changed(base, literal_set(1))]
    e = F.gpu_engine(cols, True)
    plans = parse_all(e, texts)
    plans[1].set_jit(False)
    got = results(e.run_batch(plans))
    assert got == [oracle_run(t, cols) for t in texts]
    notes = [p.batch_note() for p in plans]
    assert notes[1] == "alone: specialisation is off" and notes[2] == "alone: its filter shapes differ from every other plan's", notes
    assert [(q, k) for _, q, k, _ in slots([notes[0], notes[3]])] == [(0, 2), (1, 2)]
    e.close()


def test_vdlrun_batch_end_to_end(tmp_path):
    """`vdlrun --jit --batch FILE --batch FILE`: one reply per line, stdin's first, each decoded as the pipe's last stage does"""
    rows = 5000
    texts = [changed(golden("q6.vdl"), literal_set(k)) for k in range(3)]
    args = [VDLRUN, "--jit", "--rows", str(rows)]
    for k in (1, 2):
        path = tmp_path / ("q6_%d.vdl" % k)
        path.write_text(texts[k])
        args += ["--batch", str(path)]
    r = subprocess.run(args, input=texts[0].encode(), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 3
    cols = lineitem(datagen.Q6_COLUMNS, rows)
    dictionary = resolve.load_dictionary(os.path.join(META, "dictionary.csv"))
    for k, line in enumerate(lines):
        reply = json.load(io.StringIO(line))
        reference_shape(reply["results"])
        assert reply["results"] == oracle_run(texts[k], cols), k
        names, decoded = resolve.decode(reply, dictionary)
        assert len(names) == 1 and len(decoded) == 1
    notes = re.findall(r"vdlrun: batch: (.*)", r.stderr.decode())
    assert [(q, k) for _, q, k, _ in slots(notes)] == [(0, 3), (1, 3), (2, 3)], r.stderr.decode()[-2000:]
    # without --batch the reply is the one line it always was
    one = subprocess.run([VDLRUN, "--jit", "--rows", str(rows)], input=texts[0].encode(), capture_output=True, timeout=600)
    assert one.returncode == 0 and one.stdout.decode().splitlines() == lines[:1] and b"batch" not in one.stderr
