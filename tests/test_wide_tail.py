"""Wide sums in the GROUP BY tail and the per-operator folds (vdl_plan_set_wide_sums_tail; DESIGN.md section 5.17 "The tail") on the GPU.

Every SUM is checked against Python integer arithmetic over the uploaded columns (tests/wide_tail_cases.py: terms in wrapped int64,
summed as Python ints per group).  In mode 1 (hi << 64) | lo must equal that value for every group, lo must equal the switch-off run
of the same plan bit for bit (which must equal the oracle), and MIN / MAX / COUNT / FIRST carry their sign extension.

Sizes straddle the folds' units: 8 entries per lane, 64 per bitmap word, 512 per wave, 2048 per block and 4096 per compaction tile of
k_group_fold; k_seg_fold's words and its 16-word fast path; k_fold_global's 2048 blocks x 2048 rows.  The values are the edges of the
split x = H * 2^32 + L and the ends of int64."""
import json
import os
import sys

import numpy as np
import pytest

import mplan2vdl_amd as m
import wide_cases as wc
import wide_tail_cases as wt
from helpers import Rendezvous, engine_with, oracle_run
from mplan2vdl_amd import _lib, frontend
from wide_cases import BIG, by_field

sys.path.insert(0, os.path.join(wc.ROOT, "tests", "golden"))
import make_plan_goldens as mk  # noqa: E402
import sql_eval  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = sorted(f for f in os.listdir(os.path.join(wc.ROOT, "tests", "golden", "plans")) if f.startswith("q") and f.endswith(".json"))


def values(results):
    """{tmpN: {".field": values}} -> {tmpN: values}"""
    return {tmp: list(next(iter(f.values()))) for tmp, f in results.items()}


def wide_run(p, mode, tail=True):
    """({tmp: exact values}, {tmp: (lo, hi)}) of one run of plan p in `mode`"""
    p.set_wide_sums(mode, tail=tail)
    res = values(p.run()["results"])
    return res, p.collect_words()


def check_words(tag, plain, res, words, sums):
    """every output of a wide run against the switch-off run `plain` and the exact sums {tmp: [..]} of its SUM outputs"""
    assert set(res) == set(plain) == set(words), tag
    for tmp in plain:
        lo, hi = words[tmp]
        assert hi is not None and len(lo) == len(hi) == len(plain[tmp]), (tag, tmp)
        assert [int(x) for x in lo] == plain[tmp], (tag, tmp, "low words differ from the switch-off run")
        got = [wt.exact(a, b) for a, b in zip(lo, hi)]
        assert got == [int(x) for x in res[tmp]], (tag, tmp)
        if tmp in sums:
            assert got == sums[tmp], (tag, tmp, "exact", sums[tmp][:4], "engine", got[:4])
        else:
            assert [int(x) for x in hi] == [x >> 63 for x in plain[tmp]], (tag, tmp, "not the sign extension")


def check_group(tag, text, meta, cols, filtered, modes=(1,)):
    want = values(oracle_run(text, cols))
    sums = wt.exact_group_sums(cols, filtered, meta)
    e = engine_with(cols)
    try:
        p = e.parse(text)
        plain = values(p.run()["results"])
        assert plain == want, (tag, "switch off differs from the oracle")
        for tmp, s in sums.items():
            assert [wt.low(x) for x in s] == plain[tmp], (tag, tmp, "the reference's low words are not the oracle's")
        for mode in modes:
            res, words = wide_run(p, mode)
            check_words((tag, mode), plain, res, words, sums)
            assert p.wide_note().startswith("tail: "), p.wide_note()
        p.close()
    finally:
        e.close()
    return sums


# ---- 1. all folds, at the kernels' edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [True, False], ids=["batch", "k_seg_fold"])
@pytest.mark.parametrize("filtered", [True, False], ids=["filtered", "all"])
def test_every_fold_at_the_kernels_edges(filtered, batch, monkeypatch):
    if not batch:
        monkeypatch.setenv("VDL_NO_GROUP_BATCH", "1")
    text, meta = wt.group_program(filtered)
    overflowed = 0
    for n in wt.SIZES:
        for shape in ("short", "mixed", "one"):
            cols = wt.group_columns(n, n * 7 + len(shape), shape)
            sums = check_group("tail_%s_%s_%d" % ("filtered" if filtered else "all", shape, n), text, meta, cols, filtered)
            overflowed += sum(not wc.I64_MIN <= x <= wc.I64_MAX for s in sums.values() for x in s)
    assert overflowed > 100                                     # (the values are such that many groups leave int64)


def test_keys_out_of_order_take_the_radix_route():
    for filtered in (True, False):
        text, meta = wt.group_program(filtered)
        for n in (9, 513, 4097, 50021):
            cols = wt.group_columns(n, n, "mixed")
            cols["t.k"] = np.random.default_rng(n).permutation(cols["t.k"])
            check_group("tail_unsorted_%d" % n, text, meta, cols, filtered)


# ---- 2. long single runs ---------------------------------------------------------------------------------------------------------------------
def long_runs():
    n = 100003
    alt = np.where(np.arange(n) % 2 == 0, wc.I64_MAX, wc.I64_MIN).astype(np.int64)
    return {"big": np.full(n, BIG, np.int64), "minus_one": np.full(n, -1, np.int64), "alternating": alt,
            "excursion": np.r_[np.full(50000, BIG, np.int64), np.full(50000, -BIG, np.int64)]}


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "k_seg_fold"])
def test_long_single_runs(batch, monkeypatch):
    if not batch:
        monkeypatch.setenv("VDL_NO_GROUP_BATCH", "1")
    text, meta = wt.group_program(False, folds=["FoldSum", "FoldChoose"])
    for name, v in long_runs().items():
        n = len(v)
        cols = {"t.k": np.full(n, 5, np.int64), "t.v": v, "t.w": np.full(n, 2, np.int32), "t.f": np.ones(n, np.int64)}
        sums = check_group("long_" + name, text, meta, cols, False, modes=(1, 2) if name in ("excursion", "minus_one") else (1,))
        total = sums[next(tmp for tmp, f, d in meta if f == "FoldSum" and d == "v")]
        assert total == [sum(v.tolist())]
        if name == "big":
            assert total[0].bit_length() >= 78                  # 100003 x (2^62 + 7): 79 bits with the sign


def test_a_run_of_whole_words_behind_a_short_one(monkeypatch):
    """an unfiltered dense key, a run of 3 and then one run of 16 full words and more, on the k_seg_fold route: the long run crosses
    waves and is carried from word to word.  At these sizes a wave holds at most four words, so this is the word-by-word path; the
    16-word fast path needs the sizes of the test below."""
    monkeypatch.setenv("VDL_NO_GROUP_BATCH", "1")
    text, meta = wt.group_program(False)
    for n in (3 + 16 * 64, 3 + 16 * 64 + 61, 3 + 40 * 64 + 7):
        cols = wt.group_columns(n, n, "one")
        cols["t.k"][3:] += 1
        check_group("whole_words_%d" % n, text, meta, cols, False)


LONG_RUN = wt.prog("1,Load,t.k", "2,Project,val,Id 1,k", "3,Load,t.v", "4,Project,val,Id 3,v",
                   "5,RangeC,val,0,1099511627776,1", "6,Partition,val,Id 2,val,Id 5,val", "7,RangeV,val,0,Id 2,1",
                   "8,Scatter,Id 2,Id 7,val,Id 6,val", "9,Scatter,Id 4,Id 7,val,Id 6,val",
                   "10,FoldSum,val,Id 8,val,Id 9,val", "11,Project,total,Id 10,val", "12,MaterializeCompact,Id 11",
                   "13,FoldChoose,val,Id 8,val,Id 8,val", "14,Project,key,Id 13,val", "15,MaterializeCompact,Id 14")


def test_a_long_run_crosses_the_fast_path_of_k_seg_fold(monkeypatch):
    """k_seg_fold runs 8192 waves, each over ceil(words / 8192) consecutive words: the first four go word by word, and only then, while
    the wave carries a run, whole words are reduced 16 or 8 at a time.  28 words per wave (14.7 M entries: a run of 3, then one run of
    all the rest) take the word-by-word trip, the 16-word form and the 8-word form in that order; both have to reduce the high halves
    beside the terms.  The exact sums against Python integers, the low words against the switch-off run."""
    monkeypatch.setenv("VDL_NO_GROUP_BATCH", "1")
    n = 28 * 8192 * 64 - 1000
    assert ((n + 63) // 64 + 8191) // 8192 == 28
    r = np.random.default_rng(28)
    v = np.array(wt.EDGE_VALUES, np.int64)[r.integers(0, len(wt.EDGE_VALUES), n)]
    k = np.full(n, 6, np.int64)
    k[:3] = 5
    want = {"total": [sum(v[:3].tolist()), sum(v[3:].tolist())], "key": [5, 6]}
    assert not wc.I64_MIN <= want["total"][1] <= wc.I64_MAX       # (millions of terms of 62 and 63 bits: the sum is far outside one word)
    e = engine_with({"t.k": k, "t.v": v})
    try:
        p = e.parse(LONG_RUN)
        plain = by_field(p.run()["results"])
        assert plain == wc.wrapped(want)
        p.set_wide_sums(1, tail=True)
        got = by_field(p.run()["results"])
        assert got == want, (got, want)
        assert "k_seg_fold" in p.wide_note(), p.wide_note()
        words = {next(iter(p.collect()["results"][tmp]))[1:]: w for tmp, w in p.collect_words().items()}
        for f, (lo, hi) in words.items():
            assert [int(x) for x in lo] == plain[f] and [int(x) for x in hi] == [x >> 64 for x in want[f]], f
        p.close()
    finally:
        e.close()


RUNS_OF_A_COLUMN = wt.prog("1,Load,t.k", "2,Project,val,Id 1,k", "3,Load,t.v", "4,Project,val,Id 3,v",
                           *["%d,%s" % (5 + 2 * i + j, body) for i, f in enumerate(wt.FOLDS)
                             for j, body in enumerate(("%s,val,Id 2,val,Id 4,val" % f, "MaterializeCompact,Id %d" % (5 + 2 * i)))])


@pytest.mark.parametrize("lens", [(3, 64, 61, 130), (1,), (65,), (2, 2, 1)], ids=["258", "1", "65", "value_returns"])
def test_runs_of_a_loaded_control_column(lens):
    """The control vector is a loaded column, the data another: no stored key whose heads could be cached, so the fold makes its heads
    on the spot and runs k_seg_fold over them, every slot an entry.  Runs of 3, 64, 61 and 130: one ends where a bitmap word ends, one
    spans three words.  In (2, 2, 1) the first control value returns: runs are not groups."""
    n = sum(lens)
    k = np.repeat(np.arange(len(lens)) + 1, lens).astype(np.int64)
    if lens == (2, 2, 1):
        k[-1] = 1
    v = np.array(wt.EDGE_VALUES, np.int64)[np.random.default_rng(n).integers(0, len(wt.EDGE_VALUES), n)]
    cols = {"t.k": k, "t.v": v}
    heads = np.r_[0, np.cumsum(lens)[:-1]]
    sums = {"tmp6": [int(x) for x in np.add.reduceat(v.astype(object), heads)]}      # (tmp6 = the MaterializeCompact of the FoldSum)
    want = values(oracle_run(RUNS_OF_A_COLUMN, cols))
    assert [wt.low(x) for x in sums["tmp6"]] == want["tmp6"] and len(want) == len(wt.FOLDS)
    e = engine_with(cols)
    try:
        p = e.parse(RUNS_OF_A_COLUMN)
        p.set_fusion(False)
        plain = values(p.run()["results"])
        assert plain == want, (lens, "switch off differs from the oracle")
        res, words = wide_run(p, 1)
        check_words(("column_runs", lens), plain, res, words, sums)
        assert "k_seg_fold" in p.wide_note(), p.wide_note()
        p.close()
    finally:
        e.close()


# ---- 3. mode 2 -------------------------------------------------------------------------------------------------------------------------------
def test_checked_mode_names_field_group_and_value():
    text, meta = wt.group_program(False, folds=["FoldSum", "FoldChoose"])
    n = 2049
    cols = wt.group_columns(n, 11, "short", values=[3, -7, 1000, 0])
    clean = {k: v.copy() for k, v in cols.items()}
    keys = sorted(set(int(x) for x in cols["t.k"]))
    g = max(range(len(keys)), key=lambda i: int((cols["t.k"] == keys[i]).sum()))      # a group of several rows
    rows = np.flatnonzero(cols["t.k"] == keys[g])
    assert len(rows) >= 2
    cols["t.v"][rows[0]] = wc.I64_MAX
    cols["t.v"][rows[-1]] = wc.I64_MAX
    cols["t.w"][rows] = 2                                       # v * (w - 1) = v: that sum leaves int64 too, behind the first one
    exact = sum(int(x) for x in cols["t.v"][rows])
    assert exact > wc.I64_MAX
    tmp_v = next(tmp for tmp, f, d in meta if f == "FoldSum" and d == "v")
    e = engine_with(cols)
    try:
        p = e.parse(text)
        name = next(iter(p.run()["results"][tmp_v]))[1:]       # the output's field
        p.set_wide_sums(2, tail=True)
        with pytest.raises(m.VdlError) as err:
            p.run()
        msg = str(err.value)
        assert err.value.code == _lib.VDL_ERR_OVERFLOW == 8
        assert "'%s'" % name in msg and "(%s)" % tmp_v in msg and "group %d:" % g in msg and str(exact) in msg, msg
        assert p.collect()["results"] == {}
        res, _ = wide_run(p, 1)                                 # mode 1 delivers it
        assert res[tmp_v][g] == exact
        p.close()
    finally:
        e.close()
    check_group("checked_clean", text, meta, clean, False, modes=(2, 1))      # the plant removed: passes and equals the oracle


# ---- 4. consumed sums ------------------------------------------------------------------------------------------------------------------------
def having_cols(n=5000, plant=False):
    r = np.random.default_rng(4)
    cols = {"t.k": np.sort(r.integers(0, 400, n)).astype(np.int64), "t.v": r.integers(-50, 120, n).astype(np.int64)}
    if plant:
        rows = np.flatnonzero(cols["t.k"] == cols["t.k"][n // 2])
        assert len(rows) >= 3
        cols["t.v"][rows[:3]] = BIG                             # 3 x (2^62 + 7): outside int64
        return cols, sum(cols["t.v"][rows].tolist())
    return cols


@pytest.mark.parametrize("batch", [True, False], ids=["batch", "k_seg_fold"])
def test_a_sum_read_by_a_comparison_is_checked(batch, monkeypatch):
    """Q18's shape: the tail's FoldSum feeds Greater against a constant, which filters the groups"""
    if not batch:
        monkeypatch.setenv("VDL_NO_GROUP_BATCH", "1")
    cols = having_cols()
    want = wt.having_want(cols)
    assert 10 < len(want["key"]) < 400
    e = engine_with(cols)
    try:
        p = e.parse(wt.HAVING)
        assert by_field(p.run()["results"]) == want == by_field(oracle_run(wt.HAVING, cols))
        for mode in (1, 2):
            res, words = wide_run(p, mode)
            assert {k[1:]: v for f in p.collect()["results"].values() for k, v in f.items()} == want, mode
            assert all(hi is not None and [int(x) for x in hi] == [int(x) >> 63 for x in lo] for lo, hi in words.values())
        p.close()
    finally:
        e.close()
    cols, planted = having_cols(plant=True)
    assert planted > wc.I64_MAX
    e = engine_with(cols)
    try:
        p = e.parse(wt.HAVING)
        for mode in (1, 2):
            p.set_wide_sums(mode, tail=True)
            with pytest.raises(m.VdlError) as err:
                p.run()
            msg = str(err.value)
            assert err.value.code == _lib.VDL_ERR_OVERFLOW and "(Id %d)" % wt.HAVING_CONSUMER in msg and "Greater" in msg and str(planted) in msg, msg
            assert p.collect()["results"] == {}
        p.close()
    finally:
        e.close()


def test_a_global_sum_read_by_a_product_is_checked():
    """Q11's shape under fusion off: a global FoldSum feeds a Multiply"""
    n = 5000
    v = np.random.default_rng(5).integers(-1000, 1000, n).astype(np.int64)
    e = engine_with({"t.v": v})
    try:
        p = e.parse(wt.SCALED)
        p.set_fusion(False)
        want = {"scaled": [3 * int(v.sum())]}
        assert by_field(p.run()["results"]) == want
        for mode in (1, 2):
            p.set_wide_sums(mode, tail=True)
            assert by_field(p.run()["results"]) == want
            assert "k_fold_global" in p.wide_note()
        p.close()
    finally:
        e.close()
    v = v.copy()
    v[[0, 77, n - 1]] = BIG
    e = engine_with({"t.v": v})
    try:
        p = e.parse(wt.SCALED)
        p.set_fusion(False)
        for mode in (1, 2):
            p.set_wide_sums(mode, tail=True)
            with pytest.raises(m.VdlError) as err:
                p.run()
            msg = str(err.value)
            assert err.value.code == _lib.VDL_ERR_OVERFLOW and "(Id %d)" % wt.SCALED_CONSUMER in msg and "Multiply" in msg and str(sum(v.tolist())) in msg, msg
            assert p.collect()["results"] == {}
        p.close()
    finally:
        e.close()


# ---- 5. k_fold_global ------------------------------------------------------------------------------------------------------------------------
def global_want(cols, single):
    keep = cols["t.f"] < 10
    if not keep.any():
        return {"s": []} if single else {"s": [], "sp": [], "mn": [], "mx": []}
    v = cols["t.v"][keep]
    out = {"s": [sum(v.tolist())]}
    if not single:
        w = cols["t.w"][keep]
        with np.errstate(over="ignore"):
            prod = v * w                                       # the per-row term wraps in int64, as the engine's does
        out.update({"sp": [sum(prod.tolist())], "mn": [int(v.min())], "mx": [int(w.max())]})
    return out


def global_cols(n, seed, pass_one_in):
    r = np.random.default_rng(seed)
    return {"t.v": np.array(wt.EDGE_VALUES, np.int64)[r.integers(0, len(wt.EDGE_VALUES), n)], "t.w": r.integers(-3, 50, n).astype(np.int64),
            "t.f": np.where(r.integers(0, pass_one_in, n) == 0, 0, 11).astype(np.int64)}


def check_global(tag, cols):
    e = engine_with(cols)
    try:
        for text, single in ((wc.GLOBAL, False), (wc.SINGLE, True)):
            want = global_want(cols, single)
            p = e.parse(text)
            p.set_fusion(False)
            plain = by_field(p.run()["results"])
            assert plain == wc.wrapped(want), (tag, single)
            p.set_wide_sums(1, tail=True)
            got = by_field(p.run()["results"])
            assert got == want, (tag, single, p.wide_note())
            words = {next(iter(p.collect()["results"][tmp]))[1:]: w for tmp, w in p.collect_words().items()}
            for k, (lo, hi) in words.items():
                assert [int(x) for x in lo] == plain[k] and [int(x) for x in hi] == [x >> 64 for x in want[k]], (tag, single, k)
            assert "k_fold_global" in p.wide_note() or not want["s"], p.wide_note()
            p.close()
    finally:
        e.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2049, 100003, 4_300_000])
def test_global_folds_with_fusion_off(n):
    """dense (most rows pass: the fold reads the column under two bitmaps) and sparse (one row in sixteen: the fold reads the entries of
    the selection); 4.3 M rows are more than 2048 blocks x 2048 rows, so that blocks take a second trip"""
    for one_in in (1, 16) if n < 4_000_000 else (1,):
        cols = global_cols(n, n + one_in, one_in)
        if one_in == 1:
            cols["t.f"][::7] = 11                               # (a filter that drops some rows)
            cols["t.f"][0] = 0
        check_global("global_%d_%d" % (n, one_in), cols)


def test_a_filter_that_keeps_nothing_returns_no_value():
    cols = global_cols(2049, 1, 1)
    cols["t.f"][:] = 11
    check_global("global_empty", cols)


# ---- 6. keys outside the pivots ----------------------------------------------------------------------------------------------------------------
def test_keys_outside_the_pivots_are_rerun_wide():
    """The program of test_wide_sums.py::test_keys_outside_the_pivots_are_refused_instead_of_rerun: with the tail switch on the
    statement-by-statement rerun delivers the exact values.  Three prices of one group are planted so that sum_disc_price -- which no
    statement reads -- leaves int64 while sum_base_price, which avg_price divides, fits."""
    text = wc.GROUPED.replace("33,RangeC,val,0,32,1", "33,RangeC,val,0,16,1")
    assert text != wc.GROUPED
    cols = wc.grouped_cols(3 * 1024 + 77)
    assert int(wc.group_of(cols).max()) >= 16
    by_key = np.argsort(wc.group_of(cols), kind="stable")      # rows in key order: the keys clamped into the last bucket still form one run each,
    cols = {k: v[by_key] for k, v in cols.items()}             # so that the rerun's groups are wc.grouped_want's
    rows = np.flatnonzero(wc.group_of(cols) == int(wc.group_of(cols)[0]))[:3]
    cols["lineitem.l_extendedprice"][rows] = 1 << 55
    cols["lineitem.l_discount"][rows] = 0
    want = wc.grouped_want(cols)
    assert any(x > wc.I64_MAX for x in want["sum_disc_price"]) and all(x <= wc.I64_MAX for x in want["sum_base_price"])
    e = engine_with(cols)
    try:
        p = e.parse(text)
        assert p.is_fused
        plain = by_field(p.run()["results"])
        assert plain == by_field(oracle_run(text, cols)) == wc.wrapped(want)
        p.set_wide_sums(1, tail=True)
        out = p.run()
        assert by_field(out["results"]) == want
        assert any(k.startswith("fusedPlanAbandoned") for k in out["timings"]), out["timings"]
        assert p.wide_note().startswith("tail: "), p.wide_note()
        p.set_wide_sums(2, tail=True)
        with pytest.raises(m.VdlError) as err:
            p.run()
        assert err.value.code == _lib.VDL_ERR_OVERFLOW and "'sum_disc_price'" in str(err.value), str(err.value)
        p.set_wide_sums(1)                                      # without the tail switch: today's refusal
        with pytest.raises(m.VdlError) as err:
            p.run()
        assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "outside the Partition pivots" in str(err.value) and "k_group_fold" in str(err.value)
        p.close()
    finally:
        e.close()


# ---- 7. the fifteen plans ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg():
    return frontend.load_metadata(mk.META)


@pytest.mark.parametrize("name", FIXTURES, ids=[f[:-5] for f in FIXTURES])
def test_every_compiled_plan_runs_checked(cfg, name):
    """mode 2 with the tail switch on reproduces the golden: nothing overflows there, every plan runs checked and no consumed-sum check
    misfires; in mode 1 every high word is the sign extension"""
    fx = json.load(open(os.path.join(wc.ROOT, "tests", "golden", "plans", name)))
    text, _, cols = mk.build(int(fx["plan"][:2]), fx["variant"] == "distinct_rangec", cfg)
    e = engine_with(cols)
    try:
        p = e.parse(text)
        p.set_wide_sums(2, tail=True)
        assert p.wide_sums_tail
        assert json.loads(json.dumps(p.run()["results"])) == fx["results"], p.wide_note()
        assert p.wide_note().startswith("wide: " if p.is_fused else "tail: "), p.wide_note()
        res, words = wide_run(p, 1)
        assert {tmp: v for tmp, v in res.items()} == values(fx["results"])
        for tmp, (lo, hi) in words.items():
            assert hi is not None and [int(x) for x in hi] == [int(x) >> 63 for x in lo], (name, tmp)
        p.close()
    finally:
        e.close()


# ---- 8. Q3 with a planted price ----------------------------------------------------------------------------------------------------------------
Q3_KEY, Q3_REV, Q3_DATE = ".l_orderkey__lineitem__l_orderkey", ".revenue", ".o_orderdate__orders__o_orderdate"


def q3_revenue(cols, key):
    """sum(l_extendedprice * (100 - l_discount)) over the lineitems of order `key` shipped after 1995-03-15 (03.sql.mplan), terms in
    wrapped int64, summed as Python ints"""
    rows = np.flatnonzero((cols["lineitem.l_orderkey"].astype(np.int64) == key) & (cols["lineitem.l_shipdate"] > 728732))
    with np.errstate(over="ignore"):
        terms = cols["lineitem.l_extendedprice"][rows] * (100 - cols["lineitem.l_discount"][rows])
    return sum(terms.tolist())


def q3_planted(cfg, scale=None):
    """(text, planted columns, {tmp: field}, golden results of the clean catalog, {position in the result: exact revenue})"""
    if scale is None:
        text, _, cols = mk.build(3, False, cfg)
    else:
        text = frontend.compile_plan(open(os.path.join(mk.META, "03.sql.mplan")).read(), cfg)
        db = sql_eval.Db(mk.META, cfg, text, scale, mk.SEED)
        loads = {ln.split(",")[2].split(";;")[0].strip() for ln in text.splitlines() if ln.split(",")[1] == "Load"}
        cols = {k: v for k, v in db.cols.items() if k in loads}
    clean = oracle_run(text, cols)
    field = {tmp: next(iter(f)) for tmp, f in clean.items()}
    by = {next(iter(f)): list(next(iter(f.values()))) for f in clean.values()}
    assert all(q3_revenue(cols, k) == r for k, r in list(zip(by[Q3_KEY], by[Q3_REV]))[:50])      # the evaluation above IS the plan's revenue
    cols = dict(cols)
    cols["lineitem.l_extendedprice"] = cols["lineitem.l_extendedprice"].copy()
    planted = {}
    for i, key in enumerate(by[Q3_KEY]):                       # the first two orders whose planted revenue leaves int64
        rows = cols["lineitem.l_orderkey"].astype(np.int64) == key
        keep = cols["lineitem.l_extendedprice"][rows].copy()
        cols["lineitem.l_extendedprice"][rows] = 1 << 62
        if wc.I64_MIN <= q3_revenue(cols, key) <= wc.I64_MAX:
            cols["lineitem.l_extendedprice"][rows] = keep
            continue
        planted[i] = q3_revenue(cols, key)
        if len(planted) == 2:
            break
    assert len(planted) == 2
    return text, cols, field, by, planted


def test_q3_with_a_planted_price(cfg):
    text, cols, field, by, planted = q3_planted(cfg)
    want = {f: list(v) for f, v in by.items()}
    for i, x in planted.items():
        want[Q3_REV][i] = x
    e = engine_with(cols)
    try:
        p = e.parse(text)
        assert not p.is_fused
        plain = {field[tmp]: v for tmp, v in values(p.run()["results"]).items()}
        assert plain == {f: [wt.low(x) for x in v] for f, v in want.items()}
        res, words = wide_run(p, 1)
        assert {field[tmp]: v for tmp, v in res.items()} == want
        assert "k_group_fold" in p.wide_note() or "k_seg_fold" in p.wide_note(), p.wide_note()
        rev_tmp = next(tmp for tmp, f in field.items() if f == Q3_REV)
        assert [int(x) for x in words[rev_tmp][0]] == plain[Q3_REV] and any(int(h) != int(l) >> 63 for l, h in zip(*words[rev_tmp]))
        # an order over an int64 key: the high vectors follow the permutation, the limit cuts both
        perm = sorted(range(len(want[Q3_KEY])), key=lambda i: (-want[Q3_KEY][i], i))
        for limit in (0, 10):
            p.set_order([(Q3_KEY[1:], True)], limit=limit)
            res, words = wide_run(p, 1)
            cut = perm[:limit] if limit else perm
            assert {field[tmp]: v for tmp, v in res.items()} == {f: [v[i] for i in cut] for f, v in want.items()}, limit
            assert all(len(lo) == len(hi) == len(cut) for lo, hi in words.values())
            assert p.order_note().startswith(("topn", "sort")), p.order_note()
        # ... and a key whose value is outside int64 cannot be ordered by
        for mode in (1, 2):
            p.set_order([("revenue", True), (Q3_DATE[1:], False)], limit=10)
            p.set_wide_sums(mode, tail=True)
            with pytest.raises(m.VdlError) as err:
                p.run()
            msg = str(err.value)
            assert err.value.code == _lib.VDL_ERR_OVERFLOW and "order key 'revenue'" in msg and any(str(x) in msg for x in planted.values()), msg
            assert p.collect()["results"] == {}
        p.close()
    finally:
        e.close()


def test_q3_high_words_stay_on_the_device_with_the_low_ones(cfg):
    """more than 65536 result rows: under set_device_outputs both vectors of every output stay in HBM, and vdl_output_high_device hands
    out memory whose copy equals vdl_output_high of a host run"""
    import torch

    text, cols, field, by, planted = q3_planted(cfg, scale=0.0125)
    assert len(by[Q3_REV]) >= 65536
    e = engine_with(cols)
    try:
        p = e.parse(text)
        res, words = wide_run(p, 1)
        rev_tmp = next(tmp for tmp, f in field.items() if f == Q3_REV)
        for i, x in planted.items():
            assert res[rev_tmp][i] == x
        assert p.high_device() == {tmp: None for tmp in words}       # a host run keeps nothing on the device
        p.set_device_outputs(True)
        p.set_wide_sums(1, tail=True)
        out = p.run()["results"]
        high = p.high_device()
        for tmp, (lo, hi) in words.items():
            dev_lo = next(iter(out[tmp].values()))
            assert isinstance(dev_lo, m.engine.DeviceValues) and high[tmp] is not None and len(high[tmp]) == len(dev_lo) == len(lo)
            assert np.array_equal(torch.as_tensor(dev_lo, device="cuda:0").cpu().numpy(), lo), tmp
            assert np.array_equal(torch.as_tensor(high[tmp], device="cuda:0").cpu().numpy(), hi), tmp
        assert all(w[1] is None for w in p.collect_words().values())      # (vdl_output_high has nothing on the host for them)
        p.set_wide_sums(2, tail=True)                           # checked: judged where the values are
        with pytest.raises(m.VdlError) as err:
            p.run()
        assert err.value.code == _lib.VDL_ERR_OVERFLOW and "'revenue'" in str(err.value), str(err.value)
        p.close()
    finally:
        e.close()


# ---- 9. switch discipline ----------------------------------------------------------------------------------------------------------------------
def test_without_the_tail_switch_the_refusals_stand_and_sharded_runs_refuse_either_way():
    e = m.Engine(device=0)
    try:
        q3 = e.parse(open(os.path.join(wc.ROOT, "tests", "golden", "q3.vdl")).read())
        off = e.parse(wc.GLOBAL)
        off.set_fusion(False)
        for mode in (1, 2):
            q3.set_wide_sums(mode)
            assert not q3.wide_sums_tail
            with pytest.raises(m.VdlError) as err:
                q3.run()
            assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "GROUP BY tail" in str(err.value) and "k_group_fold" in str(err.value), str(err.value)
            assert q3.wide_note().startswith("refused: ")
            off.set_wide_sums(mode)
            with pytest.raises(m.VdlError) as err:
                off.run()
            assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "fusion is off" in str(err.value) and "k_fold_global" in str(err.value), str(err.value)
        ag, a2a = Rendezvous(1).transport(0)                   # sharded runs over the host transport, one rank: refused whatever the switch says
        e.comm_init_host(0, 1, ag, a2a)
        for sharded in (False, True):
            q3.set_wide_sums(1, sharded=sharded, tail=True)
            q3.set_sharded_table("lineitem")
            with pytest.raises(m.VdlError) as err:
                q3.run_sharded()
            msg = str(err.value)
            assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "vdl_run_sharded" in msg, msg
            assert ("exchange route" in msg and "k_group_fold" in msg) if sharded else "add-with-carry" in msg, msg
            off.set_wide_sums(1, sharded=sharded, tail=True)
            off.set_sharded_table("t")
            with pytest.raises(m.VdlError) as err:
                off.run_sharded()
            msg = str(err.value)
            assert err.value.code == _lib.VDL_ERR_UNSUPPORTED and "vdl_run_sharded" in msg, msg
            assert "k_fold_global" in msg if sharded else "add-with-carry" in msg, msg
    finally:
        e.close()
