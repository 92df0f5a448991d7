"""Step images decoded in every scan role and at both sum widths (vdl_mscan_body.h: step_tile through load_tile, the partial-tile
branches of project_select_body and project_front_body, step_load on the front's take side; vdl_bind.cpp: the binder's choice of a
32- or 64-bit sum, bind_front's renumbered select descriptor).  Every comparison is exact: the reference is the oracle on the same
program text and the same host columns, and for a column read straight back, the numpy column.  The programs, their tables and the
floors that keep a role from passing unexercised are in tests/test_step_roles_cpu.py, which checks them without a device."""
import numpy as np
import pytest

import mplan2vdl_amd as m
from helpers import check_against_oracle, oracle_run
from test_step_roles_cpu import (EDGE_N, FRONT_BATCH, FRONT_CARRY, JOIN_INDEX, K2_WIDE, K_BASES, K_WIDTHS, KINDS, PLAN_ROLES, PLANS,
                                 ROLE_FLOOR, ROLES, SEEDS, T, WIDE_FLOOR, compiled_plan, count_roles, date_cases, front_outputs,
                                 front_program, front_tables, jit_cache, named, qualifies, six_rows, stepped_program, sum_width,
                                 surviving_rows)

pytestmark = pytest.mark.gpu

STEPPED = ("t.k", "t.t_u", "t.d", "t.k2")


def stepped_engine(cols):
    """every column uploaded, with a byte image and -- where it qualifies -- a step image: what VDL_STEP_IMAGES=1 gives a caller"""
    e = m.Engine(device=0)
    for k, v in cols.items():
        e.upload(k, v)
        e.encode(k)
        e.encode_steps(k)
        assert e.steps_info(k)[0] == qualifies(v), (k, e.steps_info(k))
    return e


def run_front(e, text, jit=False, runtime_bounds=None):
    p = e.parse(text)
    p.set_jit(jit, runtime_bounds=runtime_bounds)
    got = p.run()["results"]
    note, roles = p.jit_note(), p.step_columns()
    p.close()
    return got, note, roles


# ---- 1. both sum widths and the switch between them, on the front's take side ------------------------------------------------------
@pytest.mark.parametrize("survivors", ["six_rows", "every_row"])
@pytest.mark.parametrize("base", list(K_BASES))
def test_a_take_only_stepped_column_at_both_sum_widths(base, survivors, jit_cache, monkeypatch):
    """t.k is written out and feeds the row expression t.k - k0, nothing else: it is not carried, every survivor's value comes through
    step_load.  Its first value puts it on either side of the binder's switch between the 32-bit and the 64-bit sum: both branches
    of step_sum run, over negative and positive bases.  What these cases cannot show is a switch placed a little wrong: next to
    INT32_MAX - n the 32-bit sum is still exact (no value passes INT32_MAX), so `last_32` and `first_64` pass with either width;
    a sum that is 32 bits wide where 64 are needed shows at `below_i32_min` and `two_to_40`.  (The width asserted below is this
    file's copy of the binder's rule, a premise on the column, not an observation of the binder.)"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    dtype, k0 = K_BASES[base]
    cols = front_tables(EDGE_N, k0, dtype, six_rows(EDGE_N) if survivors == "six_rows" else None)
    assert sum_width(cols["t.k"]) == K_WIDTHS[base]
    text = front_program(k0)
    rows = surviving_rows(cols)
    if survivors == "six_rows":
        assert rows.tolist() == six_rows(EDGE_N)
    else:
        assert len(rows) == EDGE_N and FRONT_BATCH * T > FRONT_CARRY       # a batch's survivors overflow the carry area
    want = oracle_run(text, cols)
    e = stepped_engine(cols)
    assert e.steps_info("t.k")[:2] == (True, k0)
    for jit in (False, True) if base in ("last_32", "first_64", "two_to_40") else (False,):
        got, note, roles = run_front(e, text, jit)
        assert got == want, (base, survivors, jit, note)
        assert "t.k" in roles.get("front.take", []) and "t.k" not in roles.get("front.select", []), roles
        assert "t.t_u" in roles.get("front.select", []) and "t.t_u" in roles.get("front.take", []), roles
        assert front_outputs(got)["k"] == np.unique(cols["t.k"][rows]).astype(np.int64).tolist()       # the column itself, read back
        if jit:
            assert ",stp>" in note and "not specialised" not in note, note
    e.close()


# ---- 2. a stepped column under a filter, in a formula, renumbered -------------------------------------------------------------------
@pytest.fixture(scope="module")
def filter_tables():
    """(columns, engine): t.k2 starts at 2^33 -- the select side sums one stepped column in 64 bits and two in 32"""
    cols = front_tables(EDGE_N, 0, k2_base=K2_WIDE)
    assert sum_width(cols["t.k2"]) == 8 and sum_width(cols["t.d"]) == 4 and sum_width(cols["t.t_u"]) == 4
    e = stepped_engine(cols)
    yield cols, e
    e.close()


@pytest.mark.parametrize("runtime_bounds", [False, True])
@pytest.mark.parametrize("case", ["inside_one_group", "from_a_groups_first_row", "wider_than_the_domain", "above_the_domain"])
def test_a_stepped_column_under_a_filter_and_in_a_formula(filter_tables, case, runtime_bounds, jit_cache, monkeypatch):
    """t.d, stepped, under a range filter in the plan's own domain; t.k2, stepped, on the left of t.k2 > t.b; both and the join index
    at their own slots of the renumbered select descriptor, each with its own base (test_step_roles_cpu.py says why slots alone
    cannot tell a wrong copy, and what does)."""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    cols, e = filter_tables
    date = date_cases(cols)[case]
    text = front_program(0, date=date, formula=True)
    rows = surviving_rows(cols, date=date, formula=True)
    want = oracle_run(text, cols)
    assert sum(front_outputs(want)["rows"]) == len(rows)
    if case == "inside_one_group":
        assert 0 < len(rows) < 31 and rows[0] // 64 == rows[-1] // 64
    elif case == "from_a_groups_first_row":
        d = cols["t.d"]
        first = int(np.nonzero(d == date[0])[0][0])
        assert first % 64 == 0 and first > T and int(np.nonzero(d == date[1])[0][-1]) == first + 63 and len(rows)
    elif case == "wider_than_the_domain":
        assert len(rows) == len(surviving_rows(cols, formula=True)) > FRONT_CARRY
    else:
        assert len(rows) == 0
    for jit in (False, True):
        got, note, roles = run_front(e, text, jit, runtime_bounds)
        assert got == want, (case, jit, runtime_bounds, note)
        assert {"t.k2", "t.d", "t.t_u"} <= set(roles.get("front.select", [])) and {"t.t_u", "t.k"} <= set(roles.get("front.take", [])), roles
        assert front_outputs(got)["k"] == np.unique(cols["t.k"][rows]).tolist()
        if jit:
            line = [x for x in note.split("; ") if x.startswith("front: ")]
            assert line and "not specialised" not in line[0] and (",stp,rtb>" if runtime_bounds else ",stp>") in line[0], note


def test_a_stepped_column_in_a_formula_of_ranges(filter_tables):
    """t.d in a list of values (a condition column: VC_FORM), its tests in the plan's own domain: a value at a group's first row, one
    inside a group, one in the partial last tile, one the column never takes"""
    cols, e = filter_tables
    d = cols["t.d"]
    in_list = [int(d[64 * 3]), int(d[64 * 3 + 30]), int(d[EDGE_N - 2]), int(d[-1]) + 5]
    text = front_program(0, in_list=in_list)
    rows = surviving_rows(cols, in_list=in_list)
    assert len(rows) >= 3 and rows[-1] >= 4 * T
    want = oracle_run(text, cols)
    got, note, roles = run_front(e, text)
    assert got == want and "t.d" in roles.get("front.select", []), (note, roles)
    assert front_outputs(got)["k"] == np.unique(cols["t.k"][rows]).tolist()


@pytest.mark.parametrize("keys,limit", [([("k", True)], 7), ([("rows", False), ("k", True)], 0), ([("rows", True)], 5)])
def test_order_and_limit_on_the_written_out_stepped_column(filter_tables, keys, limit):
    """ORDER BY / LIMIT on the device over the front's outputs: the rows, their order and the cut are those of the oracle's columns
    under numpy's lexsort (ties by position, tests/test_order.py)"""
    cols, e = filter_tables
    text = front_program(0, date=date_cases(cols)["from_a_groups_first_row"])
    want = {k: np.asarray(v, dtype=np.int64) for k, v in front_outputs(oracle_run(text, cols)).items()}
    m_rows = len(want["k"])
    assert m_rows > 10 and len(np.unique(want["rows"])) < m_rows         # the groups' row counts tie: the next key, then the position decides
    ks = [~want[f] if desc else want[f] for f, desc in keys]
    order = np.lexsort(tuple([np.arange(m_rows)] + ks[::-1]))
    if limit:
        order = order[:limit]
    p = e.parse(text)
    p.set_order(keys, limit=limit)
    got = front_outputs(p.run()["results"])
    assert "t.k" in p.step_columns().get("front.take", []), p.step_columns()
    p.close()
    for name in want:
        assert got[name] == want[name][order].tolist(), (name, keys, limit)


# ---- 5. two stepped columns of different sum width in one tile ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [T + 1, 2 * T - 1])
def test_two_sum_widths_in_one_select_pass(n, jit_cache, monkeypatch):
    """one full tile through load_tile and one partial tile (of 1 row; of T - 1 rows) through the partial-tile branch, each decoding
    t.k2 in 64 bits and t.d, t.t_u in 32: ibase is indexed per column in both"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    cols = front_tables(n, 0, k2_base=K2_WIDE)
    assert [sum_width(cols[k]) for k in STEPPED] == [4, 4, 4, 8]
    date = (int(cols["t.d"][40]), int(cols["t.d"][n - 1]))                 # up to the last row: the partial tile's rows decide
    text = front_program(0, date=date, formula=True)
    rows = surviving_rows(cols, date=date, formula=True)
    assert rows[0] >= 40 and rows[-1] >= T and (n - 1 in rows or n == 2 * T - 1)
    want = oracle_run(text, cols)
    e = stepped_engine(cols)
    for jit in (False, True):
        got, note, roles = run_front(e, text, jit)
        assert got == want, (n, jit, note)
        assert {"t.k2", "t.d", "t.t_u"} <= set(roles.get("front.select", [])) and "t.k" in roles.get("front.take", []), roles
        assert front_outputs(got)["k"] == np.unique(cols["t.k"][rows]).tolist()
    e.close()


# ---- 3. dimension and semi-join scans, with floors against vacuous passes ------------------------------------------------------------
ROLE_COUNTS = {}
# one specialised run each: semi_front's seed 1 names all four roles, join_front's seed 2 a dimension scan and both sides of a front
JIT_SEEDS = {"semi_front": 1, "join_front": 2}


def role_counts(kind):
    """runs the programs of `kind` against the oracle (once per session) and counts the roles their runs name"""
    if kind in ROLE_COUNTS:
        return ROLE_COUNTS[kind]
    counts = {}
    for seed in SEEDS[kind]:
        text, cols = stepped_program(kind, seed)
        want = oracle_run(text, cols)
        e = stepped_engine(cols)
        p = e.parse(text)
        got = p.run()["results"]
        roles = p.step_columns()
        jitted = None
        if JIT_SEEDS.get(kind) == seed:
            p.set_jit(True)
            jitted = p.run()["results"]
            assert p.step_columns() == roles and ",stp" in p.jit_note(), (roles, p.step_columns(), p.jit_note())
            p.set_jit(False)
        p.set_fusion(False)
        unfused = p.run()["results"]
        p.close()
        e.close()
        check_against_oracle("step_roles_%s_as_planned" % kind, seed, text, cols, got, want)
        check_against_oracle("step_roles_%s_statement_by_statement" % kind, seed, text, cols, unfused, want)
        if jitted is not None:
            check_against_oracle("step_roles_%s_specialised" % kind, seed, text, cols, jitted, want)
        count_roles(counts, roles, cols)
    print("programs that name a stepped column, by role (%s):" % kind, counts)
    ROLE_COUNTS[kind] = counts
    return counts


@pytest.mark.parametrize("kind", list(KINDS))
def test_random_programs_over_stepped_columns(kind, jit_cache, monkeypatch):
    """the clustered join index and the stepped, filtered dimension column in dimension scans, semi-join scans (the position column:
    decoded with the tile, taken mod N, then an atomic OR) and fronts: as planned and statement by statement, the oracle's answer"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    role_counts(kind)


def test_the_role_floors_hold_on_the_device(jit_cache, monkeypatch):
    """the floors of tests/test_step_roles_cpu.py over the same programs, as their runs bound them (a run also binds the dimension and
    semi-join scans of the plans that fuse as a whole, so it names at least what the device-less count names)"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    per_kind = {kind: role_counts(kind) for kind in KINDS}
    total = {k: sum(c.get(k, 0) for c in per_kind.values()) for k in ROLES + ("wide",)}
    assert all(total[r] >= ROLE_FLOOR for r in ROLES) and total["wide"] >= WIDE_FLOOR, (total, per_kind)


# ---- 4. the compiled plans: what each one's scans decode ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PLANS)
def test_compiled_plans_decode_what_the_binder_names(n):
    """every compiled plan over its synthetic catalog with a step image on every column that qualifies: the oracle's answer, and the
    roles the device-less binder names (PLAN_ROLES) are named by the run -- which also binds the dimension and semi-join scans of the
    plans that fuse as a whole.  Plan 4 is the semi-join over lineitem: its semi-join scan takes its positions from the join index."""
    text, cols = compiled_plan(n)
    want = oracle_run(text, cols)
    e = stepped_engine(cols)
    for jit in (False, True):
        got, note, roles = run_front(e, text, jit)
        assert got == want, (n, jit, note)
        print("plan", n, "jit", jit, roles)
        for role, names in PLAN_ROLES.get(n, {}).items():
            assert set(names) <= set(roles.get(role, [])), (n, jit, role, roles)
        if n == 4:
            assert JOIN_INDEX in named(roles, "semi"), roles
        if n in (12, 14):                                  # aggregate scans bind no step image
            assert roles == {}, roles
    e.close()
