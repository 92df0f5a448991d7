"""Wide sums (vdl_plan_set_wide_sums) on the GPU: the exact 128-bit SUM results of the fused aggregate scans
against Python integer arithmetic over the uploaded columns (tests/wide_cases.py: terms in wrapped int64, summed as Python ints).
In every case the low words must equal what the same plan delivers with the switch off, which must equal the oracle's output.

Row counts are the smallest at which the kernels can still go wrong: one full tile + 1, and three tiles + a partial one (a grid of
three blocks and a tail).  The tile is 512 * U rows (vdl_mscan_body.h: 256 lanes x U row pairs; lane l of a block owns rows
base + 512 u + 2 l, + 1): U = 6 for the precompiled global kernel of a 3-column scan, 2 for the precompiled grouped kernel of an
8-column scan and for the specialised forms, which are pinned at VDL_JIT_U=2; the packed form takes stripes of 2048 rows per wave.
At these row counts every block runs ONE tile (the grid is rows / tile).  "two_sub_iterations" (rows 0 and 512) are two row pairs of
one lane inside one call of the row pipeline: one in-register fold.  The lane's LDS slot takes a second pair with carry where a lane
runs the pipeline twice: "tile_and_tail" (lane 0 takes row 0 with the tile and the tail row afterwards), the random cases, and
test_two_tiles_of_one_block, whose row count exceeds grid x tile so that a block walks two tiles."""
import json
import os
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
import wide_cases as wc
from helpers import Rendezvous, engine_with, oracle_run
from mplan2vdl_amd import _lib, resolve
from wide_cases import BIG, NEG, by_field

pytestmark = pytest.mark.gpu

ROOT = wc.ROOT
# (label, environment, specialised?): the precompiled kernels and every specialised form that accumulates through the body's process step
FORMS = [("precompiled", {}, False),
         ("eager", {"VDL_JIT_U": "2"}, True),
         ("staged", {"VDL_JIT_U": "2", "VDL_JIT_LATE": "1", "VDL_JIT_ASSUME_SELECTIVITY": "0.3"}, True),
         ("queue", {"VDL_JIT_U": "2", "VDL_JIT_LATE": "3", "VDL_JIT_ASSUME_SELECTIVITY": "0.3"}, True)]
PACKED = ("packed", {"VDL_JIT_U": "2", "VDL_JIT_LATE": "5"}, True)      # global scans over table columns with images on only
TILE = {"precompiled": 3072, "eager": 1024, "staged": 1024, "queue": 1024, "packed": 2048}


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


@pytest.fixture(autouse=True)
def _cache(jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)


def run(e, text, mode, jit=False, order=None):
    """(exact results by field, {field: (lo, hi)}, wide note, jit note) of one run in `mode`"""
    p = e.parse(text)
    try:
        p.set_wide_sums(mode)
        if jit:
            p.set_jit(True)
        if order:
            p.set_order(*order)
        res = p.run()
        words = {next(iter(res["results"][tmp]))[1:]: w for tmp, w in p.collect_words().items()}
        return by_field(res["results"]), words, p.wide_note(), p.jit_note()
    finally:
        p.close()


SUFFIX = {"VDL_JIT_LATE=1": ",late", "VDL_JIT_LATE=3": ",queue", "VDL_JIT_LATE=5": ",packed,late"}


def check(e, text, cols, want, jit=False, scalars=(), tag=""):
    """mode 0 == the oracle; mode 1 == `want` exactly, its low words == mode 0 (the outputs of `scalars` -- expressions over aggregates,
    evaluated over the exact values -- excepted where a sum left int64), its high words those of `want`"""
    plain, words0, note0, _ = run(e, text, 0, jit)
    assert plain == by_field(oracle_run(text, cols)), (tag, "switch off differs from the oracle")
    assert note0 == "" and all(hi is None for _, hi in words0.values()), (tag, note0)
    got, words, note, jnote = run(e, text, 1, jit)
    for k in want:
        print(tag, k, "exact", want[k], "engine", got.get(k))
    assert got == want, (tag, note, jnote)
    overflowed = any(not wc.I64_MIN <= x <= wc.I64_MAX for v in want.values() for x in v)
    for k, (lo, hi) in words.items():
        assert [int(x) for x in hi] == [x >> 64 for x in want[k]], (tag, k)
        if not (overflowed and k in scalars):
            assert [int(x) for x in lo] == plain[k], (tag, k, "low words differ from the switch-off run")
    assert note.startswith("wide: ") and "sums" in note, note
    if jit:
        form = SUFFIX.get("VDL_JIT_LATE=%s" % os.environ.get("VDL_JIT_LATE"), "")      # the form asked for is the form that ran
        assert (form + ",wide>") in jnote and "not specialised" not in jnote and "no packed form" not in jnote, jnote
        assert ",wide>" in note, note
    else:
        assert "k_mscan" in note and ",wide>" in note, note
    return got


def placements(tile, n):
    """name -> three rows; the first two (all three) take the big values.  n = tile + 1: the one row of the tail and two of the tile"""
    if n < 3 * tile:
        return {"tile_and_tail": [0, n - 1, 5]}
    return {"one_lanes_pair": [0, 1, 2 * tile + 5], "neighbouring_lanes": [0, 2, tile + 1], "two_waves": [0, 128, 300], "two_sub_iterations": [0, 512, 513],
            "first_and_last_block": [0, 2 * tile + 5, tile + 9], "partial_last_tile": [1, n - 1, n - 3]}


def with_env(monkeypatch, env):
    for k in ("VDL_JIT_U", "VDL_JIT_LATE", "VDL_JIT_ASSUME_SELECTIVITY"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def fresh(cols, images):
    e = engine_with(cols)
    if images:
        for k in cols:
            e.encode(k)
    e.set_column_images(images)
    return e


GLOBAL_FORMS = [(f, im) for f in FORMS for im in (False, True) if im is False or f[0] in ("precompiled", "eager")] + [(PACKED, True)]


@pytest.mark.parametrize("form,images", GLOBAL_FORMS, ids=["%s-%s" % (f[0], "img" if im else "noimg") for f, im in GLOBAL_FORMS])
def test_global_scans(form, images, monkeypatch):
    label, env, jit = form
    with_env(monkeypatch, env)
    tile = TILE[label]
    for n in (tile + 1, 3 * tile + 77):
        where = placements(tile, n)
        # every placement through every form; only a specialised form over IMAGES -- whose bases and scales are constants of its source, so
        # that every placement is a build of its own -- takes three of them
        names = list(where) if not (jit and images) else [k for k in where if k in ("tile_and_tail", "one_lanes_pair", "first_and_last_block", "partial_last_tile")]
        cols = wc.global_cols(n)
        e = fresh(cols, images)
        try:
            def case(tag, v, w=None, f=None):
                c = wc.global_cols(n, v, w, f)
                for k in c:
                    if not np.array_equal(c[k], cols[k]):
                        e.upload(k, c[k])
                        if images:
                            e.encode(k)
                        cols[k] = c[k]
                return check(e, wc.GLOBAL, dict(cols), wc.global_want(cols), jit, tag="%s n=%d %s" % (label, n, tag))

            for name in names:
                for value in (BIG, NEG):                       # 1., 2.: two and three rows of +2^62 + 7, of -2^62 - 5
                    for k in (2, 3):
                        v = np.zeros(n, np.int64)
                        v[where[name][:k]] = value
                        got = case("%s x%d %d" % (name, k, value), v)
                        assert got["s"] == [k * value] and not wc.I64_MIN <= got["s"][0] <= wc.I64_MAX
            # 3. out and back: three +2^62, then three -2^62 -- the sum leaves int64 on the way and ends with a clean high word
            v = np.zeros(n, np.int64)
            rows = sorted(set(where[names[0]] + where[names[-1]] + [3, 4, 6]))[:6]
            v[rows[:3]], v[rows[3:]] = 1 << 62, -(1 << 62)
            assert case("out_and_back", v)["s"] == [0]
            p = e.parse(wc.GLOBAL)
            p.set_wide_sums(2)
            if jit:
                p.set_jit(True)
            assert by_field(p.run()["results"])["s"] == [0]    # checked mode passes: an excursion is no overflow
            p.close()
            # 4., 5. random int64 terms; the product of two factors wraps per row, and so does the reference's term
            for seed in (1, 2):
                rng = np.random.default_rng(seed)
                case("random seed %d" % seed, rng.integers(wc.I64_MIN, wc.I64_MAX, n, dtype=np.int64), rng.integers(wc.I64_MIN, wc.I64_MAX, n, dtype=np.int64),
                     rng.integers(0, 20, n, dtype=np.int64))
            # 6. a range filter that excludes one of the big rows
            v, f = np.zeros(n, np.int64), np.zeros(n, np.int64)
            v[where[names[-1]]] = BIG
            f[where[names[-1]][1]] = 50
            assert case("filtered", v, np.ones(n, np.int64), f)["s"] == [2 * BIG]
        finally:
            e.close()


@pytest.mark.parametrize("jit", [False, True], ids=["precompiled", "specialised"])
def test_single_sum_plan_runs_on_the_multi_aggregate_kernel(jit, monkeypatch):
    """with the switch off this plan is k_scan's; k_scan has no wide build, so the switch routes it to k_mscan's"""
    with_env(monkeypatch, {"VDL_JIT_U": "2"} if jit else {})
    n = 3 * 3072 + 77
    cols = {k: v for k, v in wc.global_cols(n).items() if k != "t.w"}
    cols["t.v"][[0, n - 1, 3072]] = BIG
    e = engine_with(cols)
    try:
        got = check(e, wc.SINGLE, cols, wc.global_want(cols, single=True), jit, tag="single")
        assert got == {"s": [3 * BIG]}
    finally:
        e.close()


@pytest.mark.parametrize("jit", [False, True], ids=["precompiled", "specialised"])
def test_two_tiles_of_one_block(jit, monkeypatch):
    """more tiles than the grid has blocks (at most 8 per CU: 2048), so that block 0 walks tiles 0 and `grid`: the big rows lie in one
    lane's pairs of both, and the lane's LDS slot takes the second pair with carry.  The grid is read from the scan's label."""
    import re

    with_env(monkeypatch, {"VDL_JIT_U": "2"} if jit else {})
    tile = 1024 if jit else 3072
    n = 2048 * tile + 2 * tile + 77
    cols = {"t.v": np.zeros(n, np.int64), "t.f": np.zeros(n, np.int64)}
    e = engine_with(cols)
    try:
        p = e.parse(wc.SINGLE)
        p.set_wide_sums(1)
        p.set_profiling(True)
        if jit:
            p.set_jit(True)
        label = next(k for k in p.run()["timings"] if "FusedScan_" in k)
        p.close()
        grid = int(re.search(r"_grid(\d+)", label).group(1))
        assert ",wide>" in label and grid * tile + tile <= n, label
        for value in (BIG, NEG):
            cols["t.v"] = np.zeros(n, np.int64)
            cols["t.v"][[0, grid * tile, grid * tile + 1]] = value
            e.upload("t.v", cols["t.v"])
            got = check(e, wc.SINGLE, cols, wc.global_want(cols, single=True), jit, tag="two tiles of block 0, grid %d" % grid)
            assert got == {"s": [3 * value]}
    finally:
        e.close()


# ---- grouped scans: Q1's shape -------------------------------------------------------------------------------------------------------------
SCALARS =("avg_qty", "avg_price", "avg_disc")
GROUP_N = 2 * 1024 + 300                                       # two blocks of the precompiled grouped kernel (U = 2) and a partial tile


def grouped_cases():
    base = wc.grouped_cols(GROUP_N)
    g = wc.group_of(base)
    keys = sorted(set(int(x) for x in g))
    out = {"plain": base}
    c = {k: v.copy() for k, v in base.items()}                 # one group overflows, its neighbours do not: four rows of 2^62 in the second group
    c["lineitem.l_quantity"][np.nonzero(g == keys[1])[0][[0, 1, -2, -1]]] = 1 << 62
    out["one_group_overflows"] = c
    c = {k: v.copy() for k, v in base.items()}                 # 64 consecutive rows of one group: every lane of a wave hits one bucket
    c["lineitem.l_returnflag"][:128:2], c["lineitem.l_linestatus"][:128:2] = 78, 79        # (rows 0, 2, .. 126 are lanes 0 .. 63 of wave 0)
    c["lineitem.l_quantity"][:128:2] = 1 << 62
    out["a_wave_on_one_bucket"] = c
    c = {k: v.copy() for k, v in base.items()}                 # the same number of rows over the replicas (lane % replicas) and both blocks
    rows = np.arange(64) * 35 + 3
    c["lineitem.l_returnflag"][rows], c["lineitem.l_linestatus"][rows] = 78, 79
    c["lineitem.l_quantity"][rows] = 1 << 62
    out["spread_over_replicas_and_blocks"] = c
    c = {k: v.copy() for k, v in base.items()}                 # a negative group
    c["lineitem.l_quantity"][np.nonzero(g == keys[2])[0][:5]] = NEG
    c["lineitem.l_extendedprice"][np.nonzero(g == keys[2])[0][:3]] = NEG
    out["negative_group"] = c
    return out


GROUP_FORMS = [(f, False) for f in FORMS] + [(FORMS[0], True), (FORMS[1], True)]


@pytest.mark.parametrize("form,images", GROUP_FORMS, ids=["%s-%s" % (f[0], "img" if im else "noimg") for f, im in GROUP_FORMS])
def test_grouped_scans(form, images, monkeypatch):
    label, env, jit = form
    with_env(monkeypatch, env)
    for name, cols in grouped_cases().items():
        if jit and images and name not in ("one_group_overflows", "negative_group"):
            continue                                           # (with images on a specialised scan is a build per data set)
        want = wc.grouped_want(cols)
        e = fresh(cols, images)
        try:
            got = check(e, wc.GROUPED, cols, want, jit, scalars=SCALARS, tag="%s %s" % (label, name))
        finally:
            e.close()
        if name == "one_group_overflows":
            k = next(i for i, x in enumerate(want["sum_qty"]) if x > wc.I64_MAX)
            assert [i for i, x in enumerate(want["sum_qty"]) if not wc.I64_MIN <= x <= wc.I64_MAX] == [k]      # ... and its neighbours do not
            low = wc.wrapped(want)["sum_qty"][k]
            assert got["avg_qty"][k] == want["sum_qty"][k] // want["count_order"][k] != wc._div(low, want["count_order"][k])      # the exact quotient, not the wrapped sum's
            assert wc.I64_MIN <= got["avg_qty"][k] <= wc.I64_MAX
        if name in ("a_wave_on_one_bucket", "spread_over_replicas_and_blocks"):
            assert max(want["sum_qty"]) >= 64 << 62
        if name == "negative_group":
            assert min(want["sum_qty"]) < wc.I64_MIN and min(want["min_qty"]) == NEG and min(want["sum_base_price"]) < 0


def test_join_scan(monkeypatch):
    """Q14's shape at a few hundred rows: a lookup through the join index and a CASE formula as an aggregate input.  Its terms stay below
    2^40 and its rows below 2^10, so no sum can leave int64: the exact result is the oracle's, every high word its sign extension --
    through the precompiled kernel and the specialised one."""
    from test_scan_forms import passing_row, sliced, tpch

    text, full = tpch("q14")
    cols = sliced(full, 700, passing_row("q14", text, full))
    want = by_field(oracle_run(text, cols))
    assert any(len(v) for v in want.values())
    for jit in (False, True):
        with_env(monkeypatch, {"VDL_JIT_U": "2"} if jit else {})
        e = fresh(cols, True)
        try:
            got = check(e, text, cols, want, jit, tag="q14 jit=%d" % jit)
            assert got == want
        finally:
            e.close()


# ---- checked mode ------------------------------------------------------------------------------------------------------------------------------
def test_checked_mode_names_field_group_and_value():
    cases = grouped_cases()
    cols, want = cases["one_group_overflows"], wc.grouped_want(cases["one_group_overflows"])
    k = next(i for i, x in enumerate(want["sum_qty"]) if x > wc.I64_MAX)
    e = engine_with(cols)
    try:
        p = e.parse(wc.GROUPED)
        p.set_wide_sums(2)
        with pytest.raises(m.VdlError) as err:
            p.run()
        assert err.value.code == _lib.VDL_ERR_OVERFLOW == 8
        msg = str(err.value)
        assert "'sum_qty'" in msg and "group %d" % k in msg and str(want["sum_qty"][k]) in msg, msg
        assert p.collect()["results"] == {}                    # after such a failure the outputs are not delivered
        p.close()
    finally:
        e.close()
    cols = cases["plain"]                                      # the same plan over smaller data passes and delivers the mode-1 results
    e = engine_with(cols)
    try:
        assert run(e, wc.GROUPED, 2)[0] == run(e, wc.GROUPED, 1)[0] == wc.grouped_want(cols)
    finally:
        e.close()


# ---- interactions ------------------------------------------------------------------------------------------------------------------------------
def test_an_order_permutes_the_high_vectors_and_refuses_an_overflowing_key():
    cols = grouped_cases()["one_group_overflows"]
    want = wc.grouped_want(cols)
    e = engine_with(cols)
    try:
        got, words, _, _ = run(e, wc.GROUPED, 1, order=([("count_order", True)], 0))
        perm = sorted(range(len(want["count_order"])), key=lambda i: (-want["count_order"][i], i))
        assert perm != sorted(perm)                            # (the order moves rows)
        assert got == {k: [v[i] for i in perm] for k, v in want.items()}
        assert [int(x) for x in words["sum_qty"][1]] == [want["sum_qty"][i] >> 64 for i in perm] and any(int(x) for x in words["sum_qty"][1])
        cut, cut_words, _, _ = run(e, wc.GROUPED, 1, order=([("count_order", True)], 2))           # ... and the limit cuts both vectors
        assert cut == {k: [v[i] for i in perm[:2]] for k, v in want.items()} and all(len(lo) == len(hi) == 2 for lo, hi in cut_words.values())
        for mode in (1, 2):
            p = e.parse(wc.GROUPED)
            p.set_wide_sums(mode)
            p.set_order([("sum_base_price", False), ("sum_qty", True)])
            with pytest.raises(m.VdlError) as err:
                p.run()
            assert err.value.code == _lib.VDL_ERR_OVERFLOW and "sum_qty" in str(err.value), str(err.value)
            p.close()
    finally:
        e.close()


def test_run_batch_runs_a_wide_plan_alone(monkeypatch):
    with_env(monkeypatch, {})
    n = 3 * 3072 + 77
    cols = wc.global_cols(n)
    cols["t.v"][[0, 1, n - 1]] = BIG
    cols["t.f"][::7] = 11
    texts = [wc.GLOBAL, wc.GLOBAL.replace("7,RangeV,val,10,", "7,RangeV,val,12,"), wc.GLOBAL.replace("7,RangeV,val,10,", "7,RangeV,val,11,")]
    e = engine_with(cols)
    try:
        plans = [e.parse(t) for t in texts]
        for p in plans:
            p.set_jit(True)
        plans[1].set_wide_sums(1)
        res = [by_field(r["results"]) for r in e.run_batch(plans)]
        notes = [p.batch_note() for p in plans]
        assert notes[1] == "alone: wide sums are not batched", notes
        assert notes[0].startswith("batch 0: slot 0 of 2") and notes[2].startswith("batch 0: slot 1 of 2"), notes
        passing = [cols["t.f"] < k for k in (10, 12, 11)]
        for r, t, keep in zip(res, texts, passing):
            c = dict(cols)
            c["t.f"] = np.where(keep, 0, 50).astype(np.int64)
            exact = wc.global_want(c)
            assert r == (exact if t is texts[1] else wc.wrapped(exact)), notes
        assert res[1]["s"][0] > wc.I64_MAX
    finally:
        e.close()


def test_vdlrun_round_trips_a_sum_above_2_63(tmp_path):
    n = 3073
    cols = {"t.v": np.zeros(n, np.int64), "t.f": np.zeros(n, np.int64)}
    cols["t.v"][[0, n - 1]] = BIG
    with open(tmp_path / "columns.csv", "w") as f:
        for k, v in cols.items():
            f.write("%s,8,%d\n" % (k, n))
            v.tofile(str(tmp_path / (k + ".bin")))
    exe = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
    out = subprocess.run([exe, "--data", str(tmp_path), "--wide-sums"], input=wc.SINGLE.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    reply = json.loads(out.stdout)
    assert by_field(reply["results"]) == {"s": [2 * BIG]} and 2 * BIG > 1 << 63
    names, rows = resolve.decode(reply, {})
    assert [list(r) for r in rows] == [[2 * BIG]], (names, rows)
    bad = subprocess.run([exe, "--data", str(tmp_path), "--checked-sums"], input=wc.SINGLE.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert bad.returncode != 0 and str(2 * BIG) in bad.stderr.decode() and "'s'" in bad.stderr.decode(), bad.stderr.decode()


def test_keys_outside_the_pivots_are_refused_instead_of_rerun():
    """Q1 with pivots 0 .. 15 where the data's keys reach 31: with the switch off the fused scan reports the rows outside and the plan
    is rerun statement by statement (the oracle's answer); with it on that rerun -- whose sums are not the scan's -- is refused"""
    text = wc.GROUPED.replace("33,RangeC,val,0,32,1", "33,RangeC,val,0,16,1")
    assert text != wc.GROUPED
    cols = wc.grouped_cols(GROUP_N)
    assert int(wc.group_of(cols).max()) >= 16
    e = engine_with(cols)
    try:
        p = e.parse(text)
        assert p.is_fused
        out = p.run()
        assert by_field(out["results"]) == by_field(oracle_run(text, cols)) and any(k.startswith("fusedPlanAbandoned") for k in out["timings"]), out["timings"]
        for mode in (1, 2):
            p.set_wide_sums(mode)
            with pytest.raises(m.VdlError) as err:
                p.run()
            msg = str(err.value)
            assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "outside the Partition pivots" in msg and "k_group_fold" in msg, msg
            assert p.wide_note().startswith("refused: ") and p.collect()["results"] == {}
        p.set_wide_sums(0)
        assert by_field(p.run()["results"]) == by_field(out["results"])
        p.close()
    finally:
        e.close()


# ---- refusals: before any kernel runs (no column is in the catalog: a run that got as far as binding one would say VDL_ERR_COLUMN) ---------
def test_refusals_name_their_route():
    e = m.Engine(device=0)
    try:
        q3 = e.parse(open(os.path.join(ROOT, "tests", "golden", "q3.vdl")).read())       # a fused front and a GROUP BY tail
        assert not q3.is_fused
        q3.set_wide_sums(1)
        with pytest.raises(m.VdlError) as err:
            q3.run()
        assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "GROUP BY tail" in str(err.value) and "k_group_fold" in str(err.value), str(err.value)
        assert q3.wide_note().startswith("refused: ")
        off = e.parse(wc.GLOBAL)                               # fusion off: statement by statement
        off.set_fusion(False)
        off.set_wide_sums(2)
        with pytest.raises(m.VdlError) as err:
            off.run()
        assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "fusion is off" in str(err.value) and "k_fold_global" in str(err.value), str(err.value)
        ag, a2a = Rendezvous(1).transport(0)                   # a sharded run over the host transport, one rank
        e.comm_init_host(0, 1, ag, a2a)
        sh = e.parse(wc.GLOBAL)
        sh.set_wide_sums(1)
        with pytest.raises(m.VdlError) as err:
            sh.run_sharded()
        assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "vdl_run_sharded" in str(err.value) and "add-with-carry" in str(err.value), str(err.value)
    finally:
        e.close()
