"""Wide sums in sharded runs (vdl_plan_set_wide_sums_sharded; DESIGN.md section 5.17 "Sharded runs") on the GPU.  Ranks are threads of
the test, one context each on device 0, meeting in the host transport (helpers.run_ranks).  The expected value everywhere is Python
integer arithmetic over the WHOLE columns (tests/wide_cases.py), and every rank must hold exactly that.

Row counts: 3001 rows of the global program are one tile of the precompiled kernel minus a few rows on one rank and less on three;
what is under test here is the ranks' (lo, hi) partial words, the merge with carry and the finalisation, not the scans' tiles
(tests/test_wide_sums.py covers those).  The grouped program has 289 words per rank, so k_merge_words_wide runs a second block."""
import io
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import mplan2vdl_amd as m
import wide_cases as wc
from helpers import Rendezvous, engine_with, run_ranks
from mplan2vdl_amd import _lib, shard_rows
from wide_cases import BIG, NEG, by_field

pytestmark = pytest.mark.gpu

VDLRUN = os.path.join(wc.ROOT, "mplan2vdl_amd", "bin", "vdlrun")
N_DEV = torch.cuda.device_count()            # (does not initialise the GPU in this process)
SCALARS = ("avg_qty", "avg_price", "avg_disc")


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


@pytest.fixture(autouse=True)
def _env(jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    monkeypatch.setenv("VDL_JIT_U", "2")
    for k in ("VDL_JIT_LATE", "VDL_JIT_ASSUME_SELECTIVITY", "VDL_WIDE_SUMS", "VDL_WIDE_SHARDED"):
        monkeypatch.delenv(k, raising=False)


def fits(want):
    return all(wc.I64_MIN <= x <= wc.I64_MAX for v in want.values() for x in v)


def words_by_field(p, res):
    return {next(iter(res["results"][tmp]))[1:]: w for tmp, w in p.collect_words().items()}


def shard(cols, table, rank, world):
    n = len(next(v for k, v in cols.items() if k.startswith(table + ".")))
    lo, hi = shard_rows(n, rank, world)
    return lo, {k: (v[lo:hi] if k.startswith(table + ".") else v) for k, v in cols.items()}


def open_rank(cols, table, rank, world, rv):
    r0, mine = shard(cols, table, rank, world)
    e = engine_with(mine)
    e.comm_init_host(rank, world, *rv.transport(rank))
    return e, r0


def run_modes(p, want, scalars=(), tag=""):
    """the plan sharded with the switch off, in mode 1 and in mode 2, checked against the exact values `want`; the mode-2 error or None"""
    p.set_wide_sums(0)
    off = by_field(p.run_sharded()["results"])
    for k, v in wc.wrapped(want).items():                      # (a scalar over a wrapped sum is the wrapped sum's quotient, not the wrapped exact one)
        assert off[k] == v or (k in scalars and not fits(want)), (tag, k, "switch off")
    p.set_wide_sums(1, sharded=True)
    res = p.run_sharded()
    got, words = by_field(res["results"]), words_by_field(p, res)
    assert got == want, (tag, p.wide_note())
    for k, (lo, hi) in words.items():
        assert [int(x) for x in hi] == [x >> 64 for x in want[k]], (tag, k)
        if fits(want) or k not in scalars:                     # (a scalar over an overflowed sum is the exact quotient, not the wrapped sum's)
            assert [int(x) for x in lo] == off[k], (tag, k, "low words differ from the switch-off sharded run")
    p.set_wide_sums(2, sharded=True)
    try:
        checked = by_field(p.run_sharded()["results"])
    except m.VdlError as exc:
        assert p.collect()["results"] == {}, tag
        return exc
    assert checked == want, (tag, "mode 2")
    return None


# ---- the global program ---------------------------------------------------------------------------------------------------------------------
GLOBAL_N = 3001


def global_cases(world):
    """name -> whole-table columns.  Rows are planted per rank: the first, the last and the middle row of the rank's range."""
    n = GLOBAL_N
    ranges = [shard_rows(n, r, world) for r in range(world)]
    at = lambda r, k=3: [ranges[r][0], ranges[r][1] - 1, (ranges[r][0] + ranges[r][1]) // 2][:k]      # noqa: E731
    out = {}
    v = np.zeros(n, np.int64)                                  # (a) every rank's s fits, the total does not (one rank: two rows of it)
    for r in range(world):
        v[at(r, 1 if world > 1 else 2)] = BIG
    out["a_total_overflows"] = wc.global_cols(n, v)
    v = np.zeros(n, np.int64)                                  # (b) rank 0 above 2^63, the last rank below -2^63, the total fits
    v[at(0)] = BIG
    v[at(world - 1) if world > 1 else [5, 6, 7]] = NEG
    out["b_excursions"] = wc.global_cols(n, v)
    v = np.zeros(n, np.int64)                                  # (c) every rank's sum in [2^63, 2^64): its own high word is 0
    for r in range(world):
        v[at(r)] = BIG
    out["c_carry_from_the_merge"] = wc.global_cols(n, v)
    rng = np.random.default_rng(17 + world)                    # (d) every term negative
    v = -rng.integers(1, 1000, n, dtype=np.int64)
    for r in range(world):
        v[at(r)] = NEG
    out["d_all_negative"] = wc.global_cols(n, v, rng.integers(1, 5, n, dtype=np.int64))
    v, f = np.zeros(n, np.int64), np.zeros(n, np.int64)        # (e) no row passes on rank 0 / on any rank
    for r in range(world):
        v[at(r)] = BIG
    f[ranges[0][0]:ranges[0][1]] = 50
    out["e_no_row_on_rank_0"] = wc.global_cols(n, v, None, f)
    out["e_no_row_anywhere"] = wc.global_cols(n, v, None, np.full(n, 50, np.int64))
    return out


@pytest.mark.parametrize("jit", [False, True], ids=["precompiled", "specialised"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_global_scans_merge_their_pairs(world, jit):
    cases = global_cases(world)
    wants = {k: wc.global_want(c) for k, c in cases.items()}
    # what the cases are built to be
    a = wants["a_total_overflows"]["s"][0]
    assert a > wc.I64_MAX and (world == 1 or BIG <= wc.I64_MAX)
    assert wants["b_excursions"]["s"] == [3 * BIG + 3 * NEG] and 3 * BIG > wc.I64_MAX and 3 * NEG < wc.I64_MIN
    assert (1 << 63) <= 3 * BIG < (1 << 64) and wants["c_carry_from_the_merge"]["s"] == [3 * world * BIG]
    assert wants["d_all_negative"]["s"][0] < wc.I64_MIN and wants["e_no_row_anywhere"]["s"] == []
    assert wants["e_no_row_on_rank_0"]["s"] == ([] if world == 1 else [3 * (world - 1) * BIG])
    # the unsharded run's words for a total that does not fit
    e = engine_with(cases["a_total_overflows"])
    p = e.parse(wc.GLOBAL)
    p.set_wide_sums(2)
    with pytest.raises(m.VdlError) as unsharded:
        p.run()
    e.close()
    assert unsharded.value.code == _lib.VDL_ERR_OVERFLOW and str(a) in str(unsharded.value)

    def work(rank, rv):
        first = next(iter(cases.values()))
        e, r0 = open_rank(first, "t", rank, world, rv)
        lo, hi = shard_rows(GLOBAL_N, rank, world)
        p = e.parse(wc.GLOBAL)
        p.set_row_offset(r0)
        if jit:
            p.set_jit(True)
        errors, notes = {}, {}
        held = {k: v[lo:hi] for k, v in first.items()}
        for name, cols in cases.items():
            for k, v in cols.items():
                if not np.array_equal(v[lo:hi], held[k]):
                    e.upload(k, v[lo:hi])
                    held[k] = v[lo:hi]
            errors[name] = run_modes(p, wants[name], tag="%s world=%d rank=%d" % (name, world, rank))
            notes[name] = (p.wide_note(), p.jit_note())
        e.close()
        return errors, notes

    for errors, notes in run_ranks(world, work, timeout=240):
        for name, want in wants.items():
            err = errors[name]
            if fits(want):
                assert err is None, (name, err)                # mode 2 passes: a rank's own excursion is no failure
            else:
                assert isinstance(err, m.VdlError) and err.code == _lib.VDL_ERR_OVERFLOW, (name, err)
                assert str(want["s"][0]) in str(err) and "'s'" in str(err) and "group 0" in str(err), (name, err)
        assert str(errors["a_total_overflows"]) == str(unsharded.value)      # the unsharded run's text, on every rank
        assert errors["b_excursions"] is None
        for name, (note, jnote) in notes.items():
            assert note.startswith("wide: ") and note.endswith("; merged over %d rank%s" % (world, "" if world == 1 else "s")), note
            assert ",wide>" in note and (not jit or ",wide>" in jnote), (note, jnote)


# ---- the grouped program --------------------------------------------------------------------------------------------------------------------
GROUP_N = 6000


def grouped_case(world):
    """Q1-shaped rows: 2^62 planted as the price of one row per rank of ONE group (its sum_base_price fits int64 on every rank and
    passes 2^63 in the total); NEG quantities on the last rank; and one group that only rank 0 holds"""
    cols = wc.grouped_cols(GROUP_N)
    g = wc.group_of(cols)
    keys = sorted(set(int(x) for x in g))
    ranges = [shard_rows(GROUP_N, r, world) for r in range(world)]
    only0 = keys[-1]                                           # this group's rows outside rank 0 move to the first group
    move = np.nonzero(g == only0)[0]
    move = move[move >= ranges[0][1]]
    first = np.nonzero(g == keys[0])[0][0]
    for name in ("lineitem.l_returnflag", "lineitem.l_linestatus"):
        cols[name][move] = cols[name][first]
    g = wc.group_of(cols)
    for lo, hi in ranges:
        rows = np.nonzero(g[lo:hi] == keys[1])[0][[-1]] + lo
        cols["lineitem.l_extendedprice"][rows] = 1 << 62
    lo, hi = ranges[-1]
    cols["lineitem.l_quantity"][np.nonzero(g[lo:hi] == keys[2])[0][:5] + lo] = NEG
    assert set(int(x) for x in g[ranges[0][1]:]) == set(keys) - {only0} and only0 in set(int(x) for x in g[:ranges[0][1]])
    return cols, keys.index(keys[1])


@pytest.mark.parametrize("world,jit", [(2, False), (3, False), (2, True)], ids=["w2-precompiled", "w3-precompiled", "w2-specialised"])
def test_grouped_scans_merge_289_words(world, jit):
    cols, k = grouped_case(world)
    want = wc.grouped_want(cols)
    assert want["sum_base_price"][k] > wc.I64_MAX
    for r in range(world):                                     # no rank's own sum leaves int64, the total does
        assert wc.grouped_want(shard(cols, "lineitem", r, world)[1])["sum_base_price"][k] <= wc.I64_MAX
    assert [i for i, x in enumerate(want["sum_base_price"]) if x > wc.I64_MAX] == [k] and min(want["sum_qty"]) < wc.I64_MIN
    assert want["avg_price"][k] == want["sum_base_price"][k] // want["count_order"][k]

    e = engine_with(cols)                                      # the unsharded run's words for the first value that does not fit
    p = e.parse(wc.GROUPED)
    p.set_wide_sums(2)
    with pytest.raises(m.VdlError) as unsharded:
        p.run()
    e.close()

    def work(rank, rv):
        e, r0 = open_rank(cols, "lineitem", rank, world, rv)
        p = e.parse(wc.GROUPED)
        p.set_row_offset(r0)
        if jit:
            p.set_jit(True)
        n_words = p.partial_spec()[0]
        err = run_modes(p, want, scalars=SCALARS, tag="grouped world=%d rank=%d" % (world, rank))
        note = p.wide_note()
        e.close()
        return n_words, err, note

    for n_words, err, note in run_ranks(world, work, timeout=240):
        assert n_words >= 289
        assert isinstance(err, m.VdlError) and err.code == _lib.VDL_ERR_OVERFLOW and str(err) == str(unsharded.value), (err, unsharded.value)
        assert "'sum_qty'" in str(err) or "'sum_base_price'" in str(err), err
        assert "grouped" in note and note.endswith("; merged over %d ranks" % world), note


def test_an_order_permutes_the_high_vectors_on_every_rank():
    world = 2
    cols, k = grouped_case(world)
    want = wc.grouped_want(cols)
    perm = sorted(range(len(want["count_order"])), key=lambda i: (-want["count_order"][i], i))
    assert perm != sorted(perm)

    def work(rank, rv):
        e, r0 = open_rank(cols, "lineitem", rank, world, rv)
        p = e.parse(wc.GROUPED)
        p.set_row_offset(r0)
        p.set_wide_sums(1, sharded=True)
        p.set_order([("count_order", True)], sharded=True)
        res = p.run_sharded()
        out = [(by_field(res["results"]), words_by_field(p, res))]
        p.set_order([("count_order", True)], limit=2, sharded=True)
        res = p.run_sharded()
        out.append((by_field(res["results"]), words_by_field(p, res)))
        e.close()
        return out

    for (full, words), (cut, cut_words) in run_ranks(world, work, timeout=240):
        assert full == {f: [v[i] for i in perm] for f, v in want.items()}
        for f in ("sum_base_price", "sum_qty"):                # (sum_base_price leaves int64 with a high word of 0; sum_qty's is -2 in one group)
            assert [int(x) for x in words[f][1]] == [want[f][i] >> 64 for i in perm], f
        assert min(int(x) for x in words["sum_qty"][1]) == -2
        assert cut == {f: [v[i] for i in perm[:2]] for f, v in want.items()} and all(len(lo) == len(hi) == 2 for lo, hi in cut_words.values())


# ---- a join scan ----------------------------------------------------------------------------------------------------------------------------
def test_join_scan():
    """Q14's shape (tests/test_wide_sums.py::test_join_scan), lineitem sharded and part replicated: no sum can leave int64, so the exact
    result is the oracle's and every high word its sign extension -- through the precompiled kernel and the specialised one"""
    from helpers import oracle_run
    from test_scan_forms import passing_row, sliced, tpch

    text, full = tpch("q14")
    cols = sliced(full, 700, passing_row("q14", text, full))
    want = by_field(oracle_run(text, cols))
    assert any(len(v) for v in want.values())

    def work(rank, rv):
        e, r0 = open_rank(cols, "lineitem", rank, 2, rv)
        out = []
        for jit in (False, True):
            p = e.parse(text)
            p.set_sharded_table("lineitem")
            p.set_row_offset(r0)
            if jit:
                p.set_jit(True)
            assert p.is_fused and p.sharded_route() == ("fold", True)
            out.append(run_modes(p, want, tag="q14 jit=%d rank=%d" % (jit, rank)))
            p.close()
        e.close()
        return out

    for errs in run_ranks(2, work, timeout=240):
        assert errs == [None, None]


# ---- pipelined --------------------------------------------------------------------------------------------------------------------------------
def test_pipelined_queries_keep_their_own_high_words():
    """five queries over two slots, the column re-uploaded between them: consecutive queries have different high words (1 and -2), and
    the high words of query k are collected after query k + 1 has run its local phase"""
    world, n = 2, GLOBAL_N
    ranges = [shard_rows(n, r, world) for r in range(world)]
    va, vb = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for lo, hi in ranges:
        va[[lo, lo + 1, hi - 1]] = BIG
        vb[[lo, lo + 2, hi - 1]] = NEG
    sides = [wc.global_cols(n, va), wc.global_cols(n, vb)]
    wants = [wc.global_want(c) for c in sides]
    assert [w["s"][0] >> 64 for w in wants] == [1, -2]

    def work(rank, rv):
        lo, hi = ranges[rank]
        e, r0 = open_rank(sides[0], "t", rank, world, rv)
        p = e.parse(wc.GLOBAL)
        p.set_row_offset(r0)
        p.set_wide_sums(1, sharded=True)
        got = []
        for k in range(5):
            e.upload("t.v", sides[k & 1]["t.v"][lo:hi])
            p.run_sharded_begin(k & 1)
            if k:
                res = p.run_sharded_end(1 - (k & 1))
                got.append((by_field(res["results"]), words_by_field(p, res)))
        res = p.run_sharded_end(0)
        got.append((by_field(res["results"]), words_by_field(p, res)))
        e.close()
        return got

    for got in run_ranks(world, work, timeout=240):
        assert len(got) == 5
        for k, (values, words) in enumerate(got):
            assert values == wants[k & 1], k
            assert int(words["s"][1][0]) == (1, -2)[k & 1], k


# ---- one plan object through the modes --------------------------------------------------------------------------------------------------------
def test_one_plan_runs_plain_then_wide_then_plain():
    world = 2
    cols = global_cases(world)["c_carry_from_the_merge"]
    want = wc.global_want(cols)

    def work(rank, rv):
        e, r0 = open_rank(cols, "t", rank, world, rv)
        p = e.parse(wc.GLOBAL)
        p.set_row_offset(r0)
        out = [by_field(p.run_sharded()["results"])]
        p.set_wide_sums(1, sharded=True)
        out.append(by_field(p.run_sharded()["results"]))
        for k in range(2):                                     # ... and pipelined, through both slots of the resized buffers
            p.run_sharded_begin(k)
        out += [by_field(p.run_sharded_end(k)["results"]) for k in range(2)]
        p.set_wide_sums(0)
        out.append(by_field(p.run_sharded()["results"]))
        assert p.collect_words()[next(iter(p.collect_words()))][1] is None and p.wide_note() == ""
        e.close()
        return out

    for plain, wide, slot0, slot1, again in run_ranks(world, work, timeout=240):
        assert plain == again == wc.wrapped(want) and wide == slot0 == slot1 == want and not fits(want)


# ---- a failed rank ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [False, True], ids=["plain", "pipelined"])
def test_a_failed_local_phase_reaches_every_rank(pipelined):
    """as tests/test_comm_gpu.py::test_a_failed_local_phase_on_the_fold_route_reaches_every_rank, under the switch: rank 1's catalog lacks
    a column; it takes part in the gather with zeroed words -- the high words too -- and its status; both ranks raise"""
    world = 2
    cols = global_cases(world)["c_carry_from_the_merge"]
    want = wc.global_want(cols)
    errors, after = [], [None, None]

    def work(rank, rv):
        e, r0 = open_rank(cols, "t", rank, world, rv)
        lo, hi = shard_rows(GLOBAL_N, rank, world)
        p = e.parse(wc.GLOBAL)
        p.set_row_offset(r0)
        p.set_wide_sums(1, sharded=True)
        if rank == 1:
            e.drop("t.w")
        try:
            if pipelined:
                p.run_sharded_begin(0)
                p.run_sharded_end(0)
            else:
                p.run_sharded()
        except m.VdlError as exc:
            errors.append((rank, exc.code, str(exc)))
        if rank == 1:
            e.upload("t.w", cols["t.w"][lo:hi])
        after[rank] = by_field(p.run_sharded()["results"])
        e.close()

    run_ranks(world, work, timeout=240)
    assert sorted(r for r, _, _ in errors) == [0, 1], errors
    assert any(r == 0 and "failed on rank 1" in msg for r, _, msg in errors), errors
    assert any(r == 1 and code == _lib.VDL_ERR_COLUMN and "t.w" in msg for r, code, msg in errors), errors
    assert after == [want, want]


# ---- refusals with the switch on: before any kernel (no column is in the catalog: a run that got as far as binding one would say VDL_ERR_COLUMN)
def test_refusals_name_their_route():
    from mplan2vdl_amd import frontend
    from test_comm_gpu import META

    e = m.Engine(device=0)
    try:
        ag, a2a = Rendezvous(1).transport(0)
        e.comm_init_host(0, 1, ag, a2a)

        def refused(p, call, *needles):
            p.set_wide_sums(1, sharded=True)
            with pytest.raises(m.VdlError) as err:
                call(p)
            msg = str(err.value)
            assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "vdl_plan_set_wide_sums_sharded" in msg and all(s in msg for s in needles), msg
            return msg

        q3 = e.parse(open(os.path.join(wc.ROOT, "tests", "golden", "q3.vdl")).read())
        q3.set_sharded_table("lineitem")
        assert not q3.is_fused and q3.sharded_route()[0] == "exchange"
        refused(q3, lambda p: p.run_sharded(), "exchange route", "k_group_fold")
        assert q3.wide_note().startswith("refused: ")
        refused(q3, lambda p: p.run_sharded_begin(0), "vdl_run_sharded_begin", "exchange route")
        off = e.parse(wc.GLOBAL)                               # fusion off: sharded through its global folds
        off.set_fusion(False)
        off.set_sharded_table("t")
        assert off.sharded_route()[0] == "fold"
        refused(off, lambda p: p.run_sharded(), "fusion is off", "general_run_local", "k_fold_global")
        cfg = frontend.load_metadata(META)                     # TPC-H Q4: a semi-join set merged across the ranks
        q4 = e.parse(frontend.compile_plan(open(os.path.join(META, "04.sql.mplan")).read(), cfg))
        q4.set_sharded_table("lineitem")
        assert q4.is_fused and q4.sharded_route()[0] == "set"
        refused(q4, lambda p: p.run_sharded(), "set route", "semi-join")
        direct = e.parse(wc.GLOBAL)                            # the entry points that leave the collectives to their caller
        refused(direct, lambda p: p.run_local(1 << 20), "vdl_run_local", "leaves the collectives to its caller")
        refused(direct, lambda p: p.finalize_begin(1 << 20, 0), "vdl_finalize_begin", "leaves the collectives to its caller")
        refused(direct, lambda p: p.resolve_first(1 << 20), "vdl_resolve_first")
        direct.set_wide_sums(1)                                # switch off: the message of tests/test_wide_sums.py
        with pytest.raises(m.VdlError) as err:
            direct.run_sharded()
        assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "vdl_run_sharded" in str(err.value) and "add-with-carry" in str(err.value)
    finally:
        e.close()


# ---- the CLI (RCCL: one process per GPU) --------------------------------------------------------------------------------------------------------
def gpus(world):
    return pytest.param(world, marks=pytest.mark.skipif(N_DEV < world, reason="needs %d GPUs (this box has %d)" % (world, N_DEV)))


@pytest.mark.parametrize("world", [gpus(1), gpus(2)])
def test_vdlrun_wide_sharded_prints_the_one_gpu_answer(world):
    q1 = open(os.path.join(wc.ROOT, "tests", "golden", "q1.vdl")).read().encode()
    one = subprocess.run([VDLRUN, "--rows", "60175", "--wide-sums"], input=q1, capture_output=True, timeout=300)
    assert one.returncode == 0, one.stderr.decode()[-2000:]
    many = subprocess.run([VDLRUN, "--gpus", str(world), "--rows", "60175", "--wide-sums", "--wide-sharded"], input=q1, capture_output=True, timeout=300)
    assert many.returncode == 0, many.stderr.decode()[-2000:]
    a, b = json.load(io.BytesIO(one.stdout)), json.load(io.BytesIO(many.stdout))
    assert b["results"] == a["results"] and len(b["results"]) > 0      # (the refusal without --wide-sharded: tests/test_wide_sharded_cpu.py)
