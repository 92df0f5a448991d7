"""Sharded batches on the GPU (Engine.run_batch_sharded, vdl_run_batch_sharded): K plans in one sharded call -- the plans that fuse as
a whole on the fold route share ONE all-gather and ONE merge launch (k_merge_words_batch), whatever their number -- and every rank
holds, for every plan, exactly the oracle's answer over the WHOLE columns (JB.wanted), which is also what `p.run_sharded()` of that
plan alone leaves.

Ranks are threads of the test, one context each on device 0, meeting in the host transport (helpers.run_ranks), which is wrapped to
count the all-gathers.  run_ranks does not notice a rank that never came back, so every test asserts that no rank returned None.
Forms are pinned (VDL_JIT_PIN) as in test_batch.py and the module keeps one code-object cache.  Row counts: every rank gets one tile
(or stripe) of the pinned form plus one or two rows -- the smallest table at which a rank's scan has a full and a partial tile -- and,
once, 37 tiles and 511 rows per rank."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mplan2vdl_amd as m
import test_jit_bounds as JB
import test_scan_forms as F
from mplan2vdl_amd import _lib, catalog, frontend, shard_rows
from conftest import golden
from helpers import oracle_run, run_ranks
from test_batch_cpu import NOTE, VDLRUN, literal_set
from test_jit_bounds_cpu import changed
from test_scan_forms import B, M4

pytestmark = pytest.mark.gpu

N_DEV = torch.cuda.device_count()            # (does not initialise the GPU in this process)
FORMS = [(2, 0), (2, 6)]                      # (u, late): eager over byte images, every column packed
FORM_IDS = ["u2_eager", "u2_packed"]
WORLDS = [1, 2, 3]


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


def tile_of(u, late):
    return 2048 if late >= 5 else F.tile(u)


def rows_for(world, u, late, big=False):
    """whole-table rows: per rank one tile (stripe) and one or two rows; big: 37 tiles and 511 rows per rank"""
    per = 37 * tile_of(u, late) + 511 if big else tile_of(u, late) + 1
    return world * per + (1 if world > 1 else 0)


def open_rank(cols, tables, rank, world, rv, counts, images=True):
    """this rank's rows of the sharded tables (the others whole), uploaded and encoded; the transport counts its all-gathers"""
    mine, r0 = {}, 0
    for k, v in cols.items():
        if k.split(".")[0] in tables and not k.endswith(".heap"):
            lo, hi = shard_rows(len(v), rank, world)
            mine[k] = v[lo:hi]
            r0 = lo
        else:
            mine[k] = v
    e = m.Engine(device=0)
    for k, v in mine.items():
        e.upload(k, v)
        e.encode(k)
    e.set_column_images(images)
    ag, a2a = rv.transport(rank)

    def counted(send):
        counts[rank] += 1
        return ag(send)

    e.comm_init_host(rank, world, counted, a2a)
    return e, r0


def parse_all(e, texts, r0=0, table=None):
    plans = [e.parse(t) for t in texts]
    for p in plans:
        p.set_jit(True, tune=True, runtime_bounds=True)
        p.set_row_offset(r0)
        if table:
            p.set_sharded_table(table)
    return plans


def results(replies):
    return [r["results"] for r in replies]


def batch_and_alone(world, cols, tables, texts, images=True, alone=True):
    """per rank: (batch results, all-gathers of the call, [p.run_sharded()] results, their all-gathers, batch notes, sharded notes)"""
    counts = [0] * world

    def work(rank, rv):
        e, r0 = open_rank(cols, tables, rank, world, rv, counts, images)
        plans = parse_all(e, texts, r0)
        got = results(e.run_batch_sharded(plans))
        one = counts[rank]
        notes, snotes = [p.batch_note() for p in plans], [p.batch_sharded_note() for p in plans]
        each = [p.run_sharded()["results"] for p in plans] if alone else None
        many = counts[rank] - one
        again = results(e.run_batch_sharded(plans))                   # the buffers of the layout are reused; the plans are bound by now
        assert again == got and counts[rank] - one - many == (1 if world > 1 else 0)
        e.close()
        return got, one, each, many, notes, snotes

    out = run_ranks(world, work, timeout=240)
    assert all(r is not None for r in out), "a rank did not come back"
    return out


def check(out, want, world, separate=True):
    for rank, (got, one, each, many, notes, snotes) in enumerate(out):
        for k in range(len(want)):
            assert got[k] == want[k], (rank, k, notes[k])
        assert one == (1 if world > 1 else 0), (rank, one)              # ONE collective, whatever the number of plans
        if separate:
            assert each == got, rank
            assert many == (len(want) if world > 1 else 0), (rank, many)
        assert all(re.match(r"^collective 0: words \[\d+,\d+\) of \d+$", s) for s in snotes), snotes


def q6_case(n, width):
    base, cols = JB.base_program("q6", n)
    texts = [changed(base, literal_set(k)) for k in range(width)]
    return texts, cols, [JB.wanted("q6_batch", n, k, t, cols) for k, t in enumerate(texts)]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("width", [2, 3, 8, 9])
def test_q6_literal_sets(width, form, world, pinned):
    u, late = form
    pinned(u, late)
    texts, cols, want = q6_case(rows_for(world, u, late), width)
    assert len({json.dumps(w, sort_keys=True) for w in want}) == width
    out = batch_and_alone(world, cols, ("lineitem",), texts)
    check(out, want, world)
    for got, one, each, many, notes, snotes in out:
        batched = [NOTE.match(x) for x in notes[:8]]
        assert all(batched) and [(int(x.group(2)), int(x.group(3))) for x in batched[:width]] == [(q, min(width, 8)) for q in range(min(width, 8))], notes
        assert (",packed,batch" in batched[0].group(4)) == (late == 6), notes
        assert width < 9 or notes[8] == "alone: the one plan left over when its group was cut into batches of 8", notes
        heights = [tuple(int(x) for x in re.findall(r"\d+", s)[1:]) for s in snotes]
        assert heights == [(3 * q, 3 * q + 3, 3 * width) for q in range(width)], snotes


def test_q6_literal_sets_over_37_tiles_per_rank(pinned):
    u, late, world = 2, 0, 2
    pinned(u, late)
    texts, cols, want = q6_case(rows_for(world, u, late, big=True), 3)
    check(batch_and_alone(world, cols, ("lineitem",), texts), want, world)


def edge_case(n, variants):
    base, cols = JB.base_program("edge_global", n)
    texts = [changed(base, JB.VARIANTS["edge_global"][k][0]) for k in variants]
    return texts, cols, [JB.wanted("edge_global", n, k, t, cols) for k, t in zip(variants, texts)]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_edge_global_variants(form, world, pinned):
    """variants 0-3 (wrapping sums, MIN / MAX near the int64 ends) are one batch of four; all nine in one call are several batches, plans
    alone and ranges that are empty in an image's domain -- on every rank its own grouping, and one collective"""
    u, late = form
    pinned(u, late)
    n = rows_for(world, u, late)
    texts, cols, want = edge_case(n, range(4))
    assert len({json.dumps(w, sort_keys=True) for w in want}) == 4
    out = batch_and_alone(world, cols, ("t",), texts)
    check(out, want, world)
    for got, one, each, many, notes, snotes in out:
        assert [s.split(" of ")[0] for s in snotes] == ["collective 0: words [%d,%d)" % (8 * q, 8 * q + 8) for q in range(4)], snotes
    texts, cols, want = edge_case(n, range(9))
    out = batch_and_alone(world, cols, ("t",), texts, alone=False)
    check(out, want, world, separate=False)
    for got, one, each, many, notes, snotes in out:
        assert all(NOTE.match(x) or x.startswith("alone: ") for x in notes), notes
        for k in (5, 6):                                           # the empty ranges: no row anywhere, no output value
            assert all(v == [] for entry in got[k].values() for v in entry.values()), (k, got[k])


# edge_global's range filters per variant, as test_jit_bounds.py writes them: p1 in [.., ..], a1 in [.., ..], w4 <= ..
EDGE_BOUNDS = {0: ((-127, 126), (B + 500, B + 126000), M4 - 2**30), 1: ((-100, 100), (B + 10500, B + 100000), M4 - 2**29),
               2: ((-90, 110), (B + 20500, B + 110999), M4 - 2**30 - 12345), 3: ((-127, 126), (B + 1, B + 126999), M4 - 1)}


def edge_passes(cols, k):
    (p_lo, p_hi), (a_lo, a_hi), w_hi = EDGE_BOUNDS[k]
    p1, a1, w4 = cols["t.p1"].astype(np.int64), cols["t.a1"], cols["t.w4"]
    return (p1 >= p_lo) & (p1 <= p_hi) & (a1 >= a_lo) & (a1 <= a_hi) & (w4 <= w_hi)


def empty(res):
    return all(v == [] for entry in res.values() for v in entry.values())


@pytest.mark.parametrize("world", [2, 3])
def test_a_slot_no_row_passes_on_rank_0_merges_the_identities(world, pinned):
    """The rows are permuted (every column alike: global answers do not depend on the order) so that every row passing variant 2 lies in
    the LAST rank's range while its batch partners pass rows on every rank.  The batch finish leaves count 0 and the MIN / MAX identities
    in that slot on the other ranks, and the merge folds the last rank's words with them: counts, MIN and MAX are still exact."""
    u, late, v = 2, 0, 2
    pinned(u, late)
    n = rows_for(world, u, late)
    texts, cols, _ = edge_case(n, range(4))
    hit = edge_passes(cols, v)
    lo, hi = shard_rows(n, world - 1, world)
    assert 0 < hit.sum() <= hi - lo, (hit.sum(), hi - lo)
    perm = np.concatenate([np.nonzero(~hit)[0], np.nonzero(hit)[0]])
    cols = {k: c[perm] for k, c in cols.items()}
    want = [oracle_run(t, cols) for t in texts]
    head = {k: c[:lo] for k, c in cols.items()}
    assert empty(oracle_run(texts[v], head)) and not empty(want[v])          # the filter arithmetic above is the program's
    r0 = shard_rows(n, 0, world)
    assert all(not empty(oracle_run(texts[k], {c: x[r0[0]:r0[1]] for c, x in cols.items()})) for k in (0, 1, 3))
    out = batch_and_alone(world, cols, ("t",), texts)
    check(out, want, world)
    for got, one, each, many, notes, snotes in out:
        assert [(int(x.group(2)), int(x.group(3))) for x in map(NOTE.match, notes)] == [(q, 4) for q in range(4)], notes


def test_ranks_may_group_differently(pinned):
    """Rows sorted by the filter column a1 = B + 1000 e, e in [0, 127]: rank 0 holds e in [0, 64] and rank 1 e in [64, 127], so their
    1-byte images of a1 start at different bases.  Plan C's upper bound, B + 128000, is step 128 from rank 0's base -- past what that
    image's width holds: the bound counts as absent there, C has another shape than A and B and runs alone beside their batch of two --
    and step 64 from rank 1's base, inside its image: on rank 1 the three plans have one shape and share a batch of three.  The
    collective is the same one either way, and the answers are the oracle's."""
    u, late, world = 2, 0, 2
    pinned(u, late)
    n = rows_for(world, u, late)
    base, cols = JB.base_program("edge_global", n)
    order = np.argsort(cols["t.a1"], kind="stable")
    cols = {k: c[order] for k, c in cols.items()}
    texts = [changed(base, JB.g0()), changed(base, JB.VARIANTS["edge_global"][1][0]), changed(base, JB.g0(a1=(B + 500, B + 128000)))]
    want = [oracle_run(t, cols) for t in texts]
    assert not any(empty(w) for w in want)
    out = batch_and_alone(world, cols, ("t",), texts)
    check(out, want, world)
    notes = [o[4] for o in out]
    assert notes[0] != notes[1], notes
    widths = [sorted(int(NOTE.match(x).group(3)) if NOTE.match(x) else 1 for x in per) for per in notes]
    assert widths[0] == [1, 2, 2] and widths[1] == [3, 3, 3], notes
    assert notes[0][2].startswith("alone: its filter shapes differ"), notes


def test_more_than_256_merged_words(pinned):
    """forty edge plans (seven words each: 280) interleaved with forty Q6 plans over another table: segment heights 8, 3, 8, 3, ..; the
    merge kernel runs a second block and its lanes find their segments on both sides of the block's edge"""
    u, late, world = 2, 0, 2
    pinned(u, late)
    n = rows_for(world, u, late)
    e_texts, e_cols, e_want = edge_case(n, range(4))
    q_texts, q_cols, q_want = q6_case(n, 8)
    texts, want = [], []
    for k in range(40):
        texts += [e_texts[k % 4], q_texts[k % 8]]
        want += [e_want[k % 4], q_want[k % 8]]
    out = batch_and_alone(world, {**e_cols, **q_cols}, ("t", "lineitem"), texts, alone=False)
    check(out, want, world, separate=False)
    for got, one, each, many, notes, snotes in out:
        assert snotes[0] == "collective 0: words [0,8) of 440" and snotes[-1] == "collective 0: words [437,440) of 440", snotes
        assert all(NOTE.match(x) for x in notes), notes


META = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tpch10noorder")


def tpch_catalog(numbers, scale=1e-5, seed=3):
    """the programs of these TPC-H plans over ONE synthetic catalog (600 lineitems)"""
    cfg = frontend.load_metadata(META)
    texts, cols = [], {}
    for q in numbers:
        text = frontend.compile_plan(open(os.path.join(META, "%02d.sql.mplan" % q)).read(), cfg)
        for k, v in catalog.synth_columns(META, cfg, text, scale=scale, seed=seed).items():
            assert k not in cols or np.array_equal(cols[k], v), k
            cols[k] = v
        texts.append(text)
    return texts, cols


@pytest.mark.parametrize("world", [1, 2, 3])
def test_a_grouped_plan_and_a_partition_plan_beside_q6_sets(world, pinned):
    """Q1 (a grouped scan with FoldChoose words) shares the collective with its two-part segment; Q3 (a Partition: the exchange route)
    is an own plan and returns this rank's slice, the slices concatenating to the oracle's answer"""
    pinned(2, 0)
    (q6, q1, q3), cols = tpch_catalog([6, 1, 3])
    texts = [changed(q6, literal_set(0)), q1, changed(q6, literal_set(1)), q3, changed(q6, literal_set(2))]
    want = [oracle_run(t, cols) for t in texts]
    counts = [0] * world

    def work(rank, rv):
        e, r0 = open_rank(cols, ("lineitem",), rank, world, rv, counts)
        plans = parse_all(e, texts, r0, "lineitem")
        got = results(e.run_batch_sharded(plans))
        one = counts[rank]
        notes, snotes = [p.batch_note() for p in plans], [p.batch_sharded_note() for p in plans]
        each = [p.run_sharded()["results"] for p in plans]
        e.close()
        return got, one, each, notes, snotes

    out = run_ranks(world, work, timeout=240)
    assert all(r is not None for r in out)
    nw1 = 257
    for got, one, each, notes, snotes in out:
        assert got == each
        assert [got[k] for k in (0, 1, 2, 4)] == [want[k] for k in (0, 1, 2, 4)]
        assert snotes[1] == "collective 0: words [3,%d) of %d" % (3 + 2 * nw1 + 1, 9 + 2 * nw1 + 1), snotes
        assert snotes[3] == "own: exchange route" and notes[3] == "", (snotes, notes)
        assert notes[1] == "alone: grouped scans are not batched", notes
    # Q3's own collectives: the status / count gather of the exchange route comes on top of the batch's one
    assert all(o[1] >= (1 if world > 1 else 0) for o in out)
    whole = {k: {name: sum((o[0][3][k][name] for o in out), []) for name in v} for k, v in want[3].items()}
    assert whole == want[3] and not empty(want[3])


def test_a_failed_local_phase_fails_the_call_on_every_rank_and_hangs_nobody(pinned):
    """Rank 1's catalog lacks a column of the edge table: a bind error on the host, no device fault.  The edge plans fail there, their
    segments travel zeroed with the status set, every rank reports the LOWEST failing plan -- rank 1 with its own error, rank 0 with the
    status it read -- and the Q6 plans, over other columns, keep their answers."""
    u, late, world = 2, 0, 2
    pinned(u, late)
    n = rows_for(world, u, late)
    e_texts, e_cols, _ = edge_case(n, range(2))
    q_texts, q_cols, q_want = q6_case(n, 2)
    texts = [q_texts[0], e_texts[0], q_texts[1], e_texts[1]]
    counts = [0] * world

    def work(rank, rv):
        e, r0 = open_rank({**e_cols, **q_cols}, ("t", "lineitem"), rank, world, rv, counts)
        plans = parse_all(e, texts, r0)
        if rank == 1:
            e.drop("t.w8")
        try:
            e.run_batch_sharded(plans)
            err = None
        except m.VdlError as exc:
            err = (exc.code, str(exc))
        kept = [p.collect()["results"] for p in plans]
        e.close()
        return err, kept, counts[rank]

    out = run_ranks(world, work, timeout=240)
    assert all(r is not None for r in out)
    (err0, kept0, n0), (err1, kept1, n1) = out
    assert err0 and err0[0] == _lib.VDL_ERR_UNSUPPORTED and "plan 1: " in err0[1] and "failed on rank 1" in err0[1], err0
    assert err1 and err1[0] == _lib.VDL_ERR_COLUMN and "plan 1: " in err1[1] and "t.w8" in err1[1], err1
    assert n0 == n1 == 1
    for kept in (kept0, kept1):
        assert [kept[0], kept[2]] == q_want and kept[1] == {} and kept[3] == {}


def gpus(world):
    return pytest.param(world, marks=pytest.mark.skipif(N_DEV < world, reason="needs %d GPUs (this box has %d)" % (world, N_DEV)))


@pytest.mark.parametrize("world", [gpus(1), gpus(2)])
def test_vdlrun_batch_sharded_prints_the_one_gpu_batch(world, tmp_path):
    rows = 5000
    texts = [changed(golden("q6.vdl"), literal_set(k)) for k in range(3)]
    batch = []
    for k in (1, 2):
        path = tmp_path / ("q6_%d.vdl" % k)
        path.write_text(texts[k])
        batch += ["--batch", str(path)]
    one = subprocess.run([VDLRUN, "--jit", "--rows", str(rows)] + batch, input=texts[0].encode(), capture_output=True, timeout=600)
    assert one.returncode == 0, one.stderr.decode()[-2000:]
    many = subprocess.run([VDLRUN, "--gpus", str(world), "--jit", "--rows", str(rows)] + batch + ["--batch-sharded"], input=texts[0].encode(),
                          capture_output=True, timeout=600)
    assert many.returncode == 0, many.stderr.decode()[-2000:]
    a = [json.load(io.StringIO(x))["results"] for x in one.stdout.decode().splitlines()]
    b = [json.load(io.StringIO(x))["results"] for x in many.stdout.decode().splitlines()]
    assert len(a) == 3 and a == b and all(len(x) > 0 for x in a)
    notes = re.findall(r"vdlrun: batch-sharded: (collective 0: words \[\d+,\d+\) of 9); batch 0: slot (\d) of 3", many.stderr.decode())
    assert [int(q) for _, q in notes] == [0, 1, 2], many.stderr.decode()[-2000:]
