"""Join batches (vdl_set_batch_joins, Engine.set_batch_joins, VDL_BATCH_JOINS=1) without a GPU: vdl_batch_jit_check groups plans whose
one scan has derived columns and a prelude -- TPC-H Q14, Q12 and Q4 over declared columns --, builds the join batch kernels for gfx950
by hiprtc and fills the notes.  No prelude runs here; the answers are checked on the device (test_batch_joins.py).

Q14's eight plans shift the month; Q12's shift the receipt year and keep the ship modes of the IN list; Q4's shift the quarter, which
filters orders -- the semi-join set of its prelude is built from lineitem and has the same text for every quarter."""
import pytest

import mplan2vdl_amd as m
from test_batch_cpu import NOTE, slots
from test_jit import compiled, host_engine_with_declared
from test_jit_bounds_cpu import changed

ALONE_DERIVED = "alone: scans with derived columns are not batched"
ALONE_PRELUDE = "alone: scans with lookup tables or semi-join sets are not batched"
ALONE_GROUPED = "alone: grouped scans are not batched"
ALONE_TABLES = "alone: no other plan of the call builds the same lookup tables"
ALONE_LITERALS = "alone: its conditions' literals differ from every other plan's"


def q14_months(text, ks):
    return [changed(text, {728902: 728902 + 30 * k, 728932: 728932 + 30 * k}) if k else text for k in ks]


def q12_years(text, ks):
    return [changed(text, {728294: 728294 + 365 * k, 728659: 728659 + 365 * k}) if k else text for k in ks]


def q4_quarters(text, ks):
    return [changed(text, {728110: 728110 + 92 * k, 728202: 728202 + 92 * k}) if k else text for k in ks]


def like_pattern_changed(text, old, new):
    assert (",%s\n" % old) in text + "\n"
    return "\n".join(line[:-len(old)] + new if line.split(",")[1:2] == ["Like"] and line.endswith("," + old) else line for line in text.split("\n"))


@pytest.fixture
def tpch(tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    for name in ("VDL_BATCH_WIDTH", "VDL_BATCH_GROUPED", "VDL_BATCH_JOINS", "VDL_JIT_PIN", "VDL_JIT_U", "VDL_JIT_GROUP_U"):
        monkeypatch.delenv(name, raising=False)
    engines = []

    def make(n):
        text, cols = compiled(n, 1e-4)
        e = host_engine_with_declared(cols)
        engines.append(e)
        return text, e
    yield make
    for e in engines:
        e.close()


def parsed(e, texts, jit=True):
    plans = [e.parse(t) for t in texts]
    for p in plans:
        assert p.is_fused, p.describe()
        p.set_jit(jit)
    return plans


def test_switch_off_eight_q14_months_run_alone_and_nothing_is_built(tpch):
    text, e = tpch(14)
    plans = parsed(e, q14_months(text, range(8)))
    before = m.jit_counters()["compiled"]
    notes = e.batch_jit_check(plans)
    assert all(x.startswith("alone: ") for x in notes) and set(notes) <= {ALONE_DERIVED, ALONE_PRELUDE}, notes
    assert m.jit_counters()["compiled"] == before and [p.batch_code_bytes() for p in plans] == [0] * 8
    e.set_batch_joins(True)                                     # (three: the batch of eight is built, and counted, below)
    assert all(NOTE.match(x) for x in e.batch_jit_check(plans[:3]))
    e.set_batch_joins(False)
    assert e.batch_jit_check(plans) == notes


def test_switch_on_eight_q14_months_are_one_batch_of_one_code_object(tpch):
    text, e = tpch(14)
    e.set_batch_joins(True)
    plans = parsed(e, q14_months(text, range(8)))
    before = m.jit_counters()["compiled"]
    notes = e.batch_jit_check(plans)
    got = slots(notes)
    assert [(b, q, k) for b, q, k, _ in got] == [(0, q, 8) for q in range(8)], notes
    assert len({name for _, _, _, name in got}) == 1 and ",derived" in got[0][3] and got[0][3].endswith(",batch8,rtb>"), notes
    assert m.jit_counters()["compiled"] == before + 1
    again = parsed(e, q14_months(text, range(-8, 0)))[::-1]     # other months, another order: nothing compiles
    assert slots(e.batch_jit_check(again)) == got
    assert m.jit_counters()["compiled"] == before + 1
    assert all(0 < p.batch_code_bytes() < 96 << 10 for p in plans), [p.batch_code_bytes() for p in plans]


def test_the_environment_switches_it_on_when_the_context_opens(tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    monkeypatch.setenv("VDL_BATCH_JOINS", "1")
    text, cols = compiled(14, 1e-4)
    e = host_engine_with_declared(cols)
    monkeypatch.setenv("VDL_BATCH_JOINS", "0")                  # (read when the context opened)
    assert [(q, k) for _, q, k, _ in slots(e.batch_jit_check(parsed(e, q14_months(text, range(2)))))] == [(0, 2), (1, 2)]
    e.close()


def test_another_like_pattern_builds_other_lookup_tables(tpch):
    text, e = tpch(14)
    e.set_batch_joins(True)
    a, b = q14_months(text, range(2))
    odd = like_pattern_changed(q14_months(text, [2])[0], "PROMO%", "ECONOMY%")
    assert odd != q14_months(text, [2])[0]
    notes = e.batch_jit_check(parsed(e, [a, odd, b]))
    assert notes[1] == ALONE_TABLES, notes
    assert [(x[0], x[1], x[2]) for x in slots([notes[0], notes[2]])] == [(0, 0, 2), (0, 1, 2)], notes


def test_another_ship_mode_is_another_condition(tpch):
    text, e = tpch(12)
    e.set_batch_joins(True)
    a, b = q12_years(text, range(2))
    odd = changed(q12_years(text, [2])[0], {40: 64})            # another dictionary code in the IN list
    plans = parsed(e, [a, odd, b])
    assert e.batch_jit_check(plans) == [ALONE_GROUPED] * 3      # a grouped scan: both switches
    e.set_batch_grouped(True)
    notes = e.batch_jit_check(plans)
    assert notes[1] == ALONE_LITERALS, notes
    got = slots([notes[0], notes[2]])
    assert [(x[0], x[1], x[2]) for x in got] == [(0, 0, 2), (0, 1, 2)] and ",grouped,derived" in got[0][3], notes
    assert all(0 < p.batch_code_bytes() < 96 << 10 for p in (plans[0], plans[2]))


def test_three_q4_quarters_are_one_grouped_batch_over_one_semi_join_set(tpch):
    text, e = tpch(4)
    e.set_batch_joins(True)
    e.set_batch_grouped(True)
    plans = parsed(e, q4_quarters(text, range(3)))
    assert "semi-join set" in plans[0].describe()
    notes = e.batch_jit_check(plans)
    got = slots(notes)
    assert [(b, q, k) for b, q, k, _ in got] == [(0, q, 3) for q in range(3)], notes
    assert ",grouped,derived" in got[0][3] and len({x[3] for x in got}) == 1, notes
    assert all(0 < p.batch_code_bytes() < 96 << 10 for p in plans)


def test_the_existing_reasons_stay_with_the_switch_on(tpch):
    text, e = tpch(14)
    e.set_batch_joins(True)
    a, b, w, off, shape = q14_months(text, range(5))
    one_sided = changed(shape, {728902 + 120: -(1 << 63)})     # the month has lost its lower bound: another filter shape
    plans = parsed(e, [a, b, w, one_sided]) + parsed(e, [off], jit=False)
    plans[2].set_wide_sums(True)
    notes = e.batch_jit_check(plans)
    assert notes[2] == "alone: wide sums are not batched", notes
    assert notes[3] == "alone: its filter shapes differ from every other plan's", notes
    assert notes[4] == "alone: specialisation is off", notes
    assert [(x[0], x[1], x[2]) for x in slots(notes[:2])] == [(0, 0, 2), (0, 1, 2)], notes


def test_edge_join_literal_sets_decide_something():
    """the directed program of test_batch_joins.py (oracle and numpy alone): a pass there means something -- every set keeps rows, the K
    answers differ pairwise, some row passes exactly one set, some row none, and some row whose key lies outside the dimension would pass
    every set's own filters"""
    import json

    import numpy as np

    import test_batch_joins as T
    for n in T.ROWS.values():
        cols = T.table(n)
        want = [T.wanted(("edge", n, s), T.edge_join(s), cols) for s in T.SETS]
        assert len({json.dumps(w, sort_keys=True) for w in want}) == len(T.SETS)
        assert all(v for w in want for entry in w.values() for v in entry.values())
        assert all(v == [] for entry in T.wanted(("edge", n, T.EMPTY), T.edge_join(T.EMPTY), cols).values() for v in entry.values())
        for width in (2, 3, 8):
            got = [T.passes(cols, s) for s in T.SETS[:width]]
            counts = sum(g[1].astype(int) for g in got)
            assert all(g[1].any() for g in got) and (counts == 1).any() and (counts == 0).any()
            assert np.logical_and.reduce([g[0] for g in got])[~got[0][2]].any()
        assert set(cols["t.fk"][:6]) == {0, 63, 64, 69, -1, T.NU}
