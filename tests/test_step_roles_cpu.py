"""Step images in every scan role, without a GPU (tests/test_step_roles.py runs the same programs on one).  This file holds what
both share -- the hand-written front over synthetic tables, the random generators in their stepped mode, the compiled plans'
catalogs -- and the checks a device-less engine can make: a step image declared on it (Engine.declare_steps) is bound by the very
binder a run uses (csrc/vdl_bind.cpp: bind_prelude_scan, bind_front through Plan.jit_check), so Plan.step_columns() says which scan role of which program
would decode one.  That is what keeps the GPU tests from passing vacuously: the floors below are conditions on the programs."""
import os
import re

import numpy as np
import pytest

import mplan2vdl_amd as m
from helpers import oracle_run, prog
from test_random_joins import Gen as JoinGen
from test_random_semijoins import Gen as SemiGen
# the tile of the projection scans, the front's batch and its carry area (read from the kernels' own header), the compiled plans and
# their synthetic catalogs: one definition, tests/test_step_images.py's
from test_step_images import FRONT_BATCH, FRONT_CARRY, JOIN_INDEX, PLANS, T, compiled, synth

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    """one code-object cache for the module (tests/test_batch.py)"""
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


# ---- columns --------------------------------------------------------------------------------------------------------------------
def qualifies(v):
    """what k_image_steps accepts (vdl_column_image.h Steps): at least one row, never down, never up by more than 1"""
    if v.dtype.kind != "i" or len(v) < 1:
        return False
    d = np.diff(v.astype(np.int64))
    return bool(len(d) == 0 or (d.min() >= 0 and d.max() <= 1))


def sum_width(v):
    """the width the binder gives a stepped column: 4 where base .. base + n - 1 fits 32 signed bits, else 8"""
    return 4 if I32_MIN <= int(v[0]) <= I32_MAX - len(v) else 8


def rising(n, base, at, dtype=np.int64):
    """starts at `base`, goes up by 1 at every row of `at` (rows 1 .. n - 1)"""
    up = np.zeros(n, dtype=np.int64)
    up[sorted({int(r) for r in at if 1 <= r < n})] = 1
    return (base + np.cumsum(up)).astype(dtype)


def declared_engine(cols):
    """a device-less engine that knows `cols` by length and width, with a step image declared on every column that qualifies: what
    encode_steps() on every column leaves on a device"""
    e = m.Engine(device=None)
    for k, v in cols.items():
        e.register_pointer(k, 0x10000, v.dtype.itemsize, len(v))
        if qualifies(v):
            e.declare_steps(k, int(v[0]))
    return e


def has_front(plan):
    return (not plan.is_fused) and "\nfused front:" in plan.describe()


def roles_without_a_device(e, text):
    """step_columns() as the binder fills it.  Only a plan with a fused front binds its projection scans without a device
    (vdl_plan_jit_check); a plan that fuses as a whole binds its dimension and semi-join scans when it runs, so it reports {} here."""
    p = e.parse(text)
    try:
        if not has_front(p):
            return {}
        p.jit_check()
        return p.step_columns()
    finally:
        p.close()


def named(roles, prefix, only=None):
    """the stepped columns `roles` names under the roles that start with `prefix`"""
    return sorted({c for r, cs in roles.items() if r.startswith(prefix) for c in cs if only is None or c in only})


# ---- the hand-written front: a fact table t looking a filtered dimension u up through a clustered join index ---------------------
class Text:
    """program text in the vocabulary of tests/test_random_semijoins.py"""

    def __init__(self, names):
        self.lines, self.nid, self.c = [], 0, {}
        for name in names:
            self.c[name] = self.emit("Project,val,Id %d,%s" % (self.emit("Load," + name), name.split(".", 1)[1]))

    def emit(self, body):
        self.nid += 1
        self.lines.append("%d,%s" % (self.nid, body))
        return self.nid

    def const(self, k, ref): return self.emit("RangeV,val,%d,Id %d,0" % (k, ref))
    def pos(self, ref): return self.emit("RangeV,val,0,Id %d,1" % ref)
    def bin(self, op, a, b): return self.emit("%s,val,Id %d,val,Id %d,val" % (op, a, b))
    def gather(self, src, p): return self.emit("Gather,Id %d,Id %d,val" % (src, p))
    def select(self, pred): return self.emit("FoldSelect,val,Id %d,val,Id %d,val" % (self.pos(pred), pred))
    def scatter(self, v, p, at): return self.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (v, p, at))
    def fold(self, kind, key, v): return self.emit("%s,val,Id %d,val,Id %d,val" % (kind, key, v))


NU = 300                                   # rows of the dimension
X_PASS = 50                                # the dimension's filter: u.x < X_PASS
OUTPUTS = ("k", "rows", "a", "x")          # the front program's outputs, in program order: tmp ids in `front_outputs`


def front_program(k0, date=None, formula=False, in_list=None):
    """Q3's shape: t's rows with t.s > 0 [and t.d in `date`, and t.k2 > t.b, and t.d in `in_list`] whose row of u (through the join
    index t.t_u) has u.x < X_PASS, grouped by t.k - k0 over a domain too sparse for the grouped scan -- so the selection, the
    lookups and the row expression run as a fused front.  Written out per group: t.k, the rows, sum(t.a), sum(u.x[t.t_u]).
    t.k is read by the outputs only (take-only: every survivor's value comes through step_load); t.t_u decides and is read again by
    the outputs (carried); t.d, t.k2 decide only."""
    b = Text(["t.s", "t.k", "t.t_pkey", "t.t_u", "t.a", "t.d", "t.k2", "t.b", "u.x", "u.u_pkey"])
    c = b.c
    pred = b.bin("Greater", c["t.s"], b.const(0, c["t.s"]))
    if date is not None:
        pred = b.bin("LogicalAnd", pred, b.bin("LogicalAnd", b.bin("Greater", c["t.d"], b.const(date[0] - 1, c["t.d"])),
                                               b.bin("Greater", b.const(date[1] + 1, c["t.d"]), c["t.d"])))
    if formula:
        pred = b.bin("LogicalAnd", pred, b.bin("Greater", c["t.k2"], c["t.b"]))
    if in_list:
        t = b.bin("Equals", c["t.d"], b.const(in_list[0], c["t.d"]))
        for v in in_list[1:]:
            t = b.bin("LogicalOr", t, b.bin("Equals", c["t.d"], b.const(v, c["t.d"])))
        pred = b.bin("LogicalAnd", pred, t)
    sel = b.select(pred)
    # the dimension's rows that pass, as a validity vector and a position vector by row id (deduceMasks)
    su = b.select(b.bin("Greater", b.const(X_PASS, c["u.x"]), c["u.x"]))
    ids = b.gather(b.pos(c["u.u_pkey"]), su)
    ones = b.const(1, ids)
    valid = b.scatter(ones, b.pos(ones), ids)
    idx = b.scatter(b.pos(ids), b.pos(b.pos(ids)), ids)
    # the fact side looks both up through its join index and is cleaned (handleGatherJoin)
    fkf = b.gather(c["t.t_u"], b.gather(b.pos(c["t.t_pkey"]), sel))
    sm = b.select(b.gather(valid, fkf))
    k = b.gather(b.gather(c["t.k"], sel), sm)
    a = b.gather(b.gather(c["t.a"], sel), sm)
    x = b.gather(b.gather(c["u.x"], su), b.gather(b.gather(idx, fkf), sm))
    key = b.bin("Subtract", k, b.const(k0, k))             # a row expression over the stepped column
    part = b.emit("Partition,val,Id %d,val,Id %d,val" % (key, b.emit("RangeC,val,0,%d,1" % (1 << 30))))
    skey = b.scatter(key, b.pos(key), part)
    outs = [b.fold("FoldChoose", skey, b.scatter(k, b.pos(k), part)), b.fold("FoldCount", skey, b.scatter(a, b.pos(a), part)),
            b.fold("FoldSum", skey, b.scatter(a, b.pos(a), part)), b.fold("FoldSum", skey, b.scatter(x, b.pos(x), part))]
    for name, o in zip(OUTPUTS, outs):
        b.emit("MaterializeCompact,Id %d" % b.emit("Project,%s,Id %d,val" % (name, o)))
    return prog(*b.lines)


def front_outputs(results):
    """{output name: list} of a front program's results ({tmpN: {".name": values}})"""
    out = {}
    for v in results.values():
        (name, vals), = v.items()
        out[name.lstrip(".")] = vals
    return out


D0, K2_WIDE, T_U0 = 9000, 1 << 33, 20       # first values of t.d and (where asked for) t.k2; of the join index


def front_tables(n, k0, kdtype=np.int64, surviving=None, k2_base=7, seed=5, must_pass=None):
    """The tables of front_program.  Clustered, i.e. stepped: t.k from `k0` (up at rows 64, T and n - 1 and at every 5th row from 3:
    anchors and head bits both carry value), the join index t.t_u from T_U0, the date t.d from D0 (up at every row that starts a
    group of 64, and at every third row), t.k2 from `k2_base` (up at every other row).  Plain: t.s (1 on `surviving`, else every
    row), t.a, t.b, and u.x -- u's rows pass where `surviving` is None (every row of t survives), else every other one does, and the
    rows of u that the rows `must_pass` of t (the six edge rows, unless given) point at."""
    r = np.random.default_rng(seed)
    k2 = rising(n, k2_base, range(1, n, 2))
    s = np.ones(n, np.int32)
    if surviving is not None:
        s[:] = 0
        s[list(surviving)] = 1
    t_u = rising(n, T_U0, [64, T, n - 1] + list(range(7, n, 37)))
    x = np.full(NU, 10, np.int64)
    if surviving is not None:
        x[1::2] = 90
        x[t_u[six_rows(n) if must_pass is None else list(must_pass)]] = 10
    cols = {"t.s": s, "t.k": rising(n, k0, [64, T, n - 1] + list(range(3, n, 5)), kdtype), "t.t_pkey": np.zeros(n, np.int64),
            "t.t_u": t_u, "t.a": r.integers(-50, 50, n).astype(np.int64),
            "t.d": rising(n, D0, list(range(64, n, 64)) + list(range(1, n, 3)), np.int32), "t.k2": k2,
            # t.k2 > t.b on two rows of three, in runs that cross group and tile edges
            "t.b": k2 + np.where((np.arange(n) // 7) % 3 == 0, 5, -5), "u.x": x, "u.u_pkey": np.zeros(NU, np.int64)}
    assert cols["t.t_u"].max() < NU and all(qualifies(cols[k]) for k in ("t.k", "t.t_u", "t.d", "t.k2")) and not qualifies(cols["t.b"])
    return cols


def surviving_rows(cols, date=None, formula=False, in_list=None):
    """the rows of t that front_program keeps, from the numpy columns"""
    d = cols["t.d"].astype(np.int64)
    ok = (cols["t.s"] > 0) & (cols["u.x"][cols["t.t_u"]] < X_PASS)
    if date is not None:
        ok &= (d >= date[0]) & (d <= date[1])
    if formula:
        ok &= cols["t.k2"] > cols["t.b"]
    if in_list:
        ok &= np.isin(d, in_list)
    return np.nonzero(ok)[0]


EDGE_N = 4 * T + 65                         # two front batches, a partial last tile that is no multiple of 64


def six_rows(n):
    return [0, 63, 64, T - 1, T, n - 1]


# the first value of t.k: (numpy type, value), on both sides of the binder's switch between the sum widths
K_BASES = {"last_32": (np.int64, I32_MAX - EDGE_N), "first_64": (np.int64, I32_MAX - EDGE_N + 1), "i32_min": (np.int64, I32_MIN),
           "below_i32_min": (np.int64, I32_MIN - 1), "two_to_40": (np.int64, (1 << 40) + 5), "int16": (np.int16, -3000)}
K_WIDTHS = {"last_32": 4, "first_64": 8, "i32_min": 4, "below_i32_min": 8, "two_to_40": 8, "int16": 4}


def test_the_bases_straddle_the_switch_between_the_sum_widths():
    for name, (dtype, k0) in K_BASES.items():
        col = front_tables(EDGE_N, k0, dtype)["t.k"]
        assert col.dtype == dtype and int(col[0]) == k0 and sum_width(col) == K_WIDTHS[name], name
        up = np.nonzero(np.diff(col.astype(np.int64)))[0] + 1
        assert {64, T, EDGE_N - 1} <= set(up.tolist()) and len(up) < EDGE_N - 1          # anchors and head bits both carry value
    last = front_tables(EDGE_N, K_BASES["last_32"][1])["t.k"]
    assert int(last[-1]) <= I32_MAX - 1                    # the premise of the last 32-bit base: every value fits 32 signed bits
    assert EDGE_N > FRONT_BATCH * T and EDGE_N % T % 64 != 0 and FRONT_BATCH * T > FRONT_CARRY


# the date filters of the filtered front, as (lo, hi) in t.d's own values (t.d goes up at every group's first row)
def date_cases(cols):
    d = cols["t.d"].astype(np.int64)
    g = 64 * (T // 64 + 3)                                 # a group's first row, in the second tile
    assert d[g] == d[g - 1] + 1 and d[5 * 64 + 10] > d[5 * 64] and d[5 * 64 + 40] < d[6 * 64 - 1]
    return {"inside_one_group": (int(d[5 * 64 + 10]), int(d[5 * 64 + 40])),
            "from_a_groups_first_row": (int(d[g]), int(d[g + 64]) - 1),         # first row g, last row g + 63
            "wider_than_the_domain": (int(d[0]) - 1000, int(d[-1]) + 1000),
            "above_the_domain": (int(d[-1]) + 1, int(d[-1]) + 1000)}


FRONT_COLUMNS = ["t.k2", "t.b", "t.d", "t.s", "t.t_u", "t.k", "t.a"]     # the table columns of the filtered front, as describe() lists them


def front_slots(description):
    """{table column: its index in the fused front's column list} from Plan.describe()"""
    front = description.split("\nfused front:", 1)[1]
    return {name: int(k) for k, name in re.findall(r"\n  col (\d+) (t\.\w+)", front)}


def test_the_hand_written_program_is_a_fused_front_with_the_stepped_columns_in_their_roles(jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    for name in ("last_32", "first_64"):
        dtype, k0 = K_BASES[name]
        cols = front_tables(EDGE_N, k0, dtype, six_rows(EDGE_N) + list(range(2, EDGE_N, 5)))
        text = front_program(k0)
        want = front_outputs(oracle_run(text, cols))
        rows = surviving_rows(cols)
        assert set(six_rows(EDGE_N)) <= set(rows.tolist()) and len(rows) < (cols["t.s"] > 0).sum()       # the dimension's filter drops rows too
        assert want["k"] == np.unique(cols["t.k"][rows]).tolist() and sum(want["rows"]) == len(rows)
        e = declared_engine(cols)
        p = e.parse(text)
        assert has_front(p) and "expr0" in p.describe(), p.describe()                  # the front evaluates t.k - k0 itself
        note = p.jit_check()
        assert ",stp>" in note, note
        roles = p.step_columns()
        assert "t.k" in roles["front.take"] and "t.k" not in roles["front.select"], roles
        assert "t.t_u" in roles["front.select"] and "t.t_u" in roles["front.take"], roles
        e.close()
    # the filtered front: the stepped date under a range filter, the stepped t.k2 on the left of a two-column test
    cols = front_tables(EDGE_N, 0, k2_base=K2_WIDE)
    text = front_program(0, date=date_cases(cols)["inside_one_group"], formula=True)
    e = declared_engine(cols)
    p = e.parse(text)
    p.set_jit(False, runtime_bounds=True)
    note = p.jit_check()
    assert ",stp,rtb>" in note, note
    roles = p.step_columns()
    assert {"t.k2", "t.d", "t.t_u"} <= set(roles["front.select"]) and {"t.t_u", "t.k"} <= set(roles["front.take"]), roles
    # The select side's descriptor is renumbered (bind_front: slot j = renum[k]), so a table column's select slot differs from its take
    # slot only where a column that does not decide stands before it in the plan's list.  The planner does not make such a list today:
    # - build_projection lowers the selection's clause first (lower_filters), so every table column a filter, a condition or a cleaned
    #   lookup reads (the lookup's validity test is part of the clause: an INRANGE or a bitmap column over the index) gets its index
    #   before any column that only the outputs read; tidy_columns then sorts table columns first, those that drive a filter before
    #   the others, and keeps this order inside both classes.
    # - bind_front also lets an unfiltered lookup that nothing else range-checks decide, and its index with it -- a rule tidy_columns
    #   does not know.  But a front only gets a lookup column for a gather on the CLEANED selection, whose index the clause has already
    #   listed; a gather through an index that no select has cleaned is no atom of the selection, and the front hands the index
    #   itself over as a take-only column (tried with a second, unfiltered dimension, cleaned and not: the index stood at its filter-
    #   time place in the first program and was take-only in the second).
    # So a copy of ibase from the wrong index cannot be told from the right one by slot.  What the test pins instead is a list on
    # which a dropped or shifted copy shows: three stepped deciding columns with three different non-zero bases (K2_WIDE, D0, T_U0)
    # at slots 0, 2 and 4 with plain columns between them -- a copy dropped (ibase defaults to 0), or shifted by a slot either way,
    # decodes each of them with a wrong base: t.d from 0 instead of D0 lies wholly below every bound the date cases take from the
    # column, so the filtered cases keep no row where the oracle keeps some (`above_the_domain` keeps none either way and cannot
    # tell), and t.t_u from 0 looks up other rows of u.  Tried on a GPU with a library built without the `sdesc->ibase[j]` copy:
    # the three filtered cases of test_a_stepped_column_under_a_filter_and_in_a_formula fail with and without run-time bounds, as do
    # test_a_stepped_column_in_a_formula_of_ranges and every case of test_order_and_limit_on_the_written_out_stepped_column;
    # `above_the_domain` passes.
    slots = front_slots(p.describe())
    assert [k for k, _ in sorted(slots.items(), key=lambda kv: kv[1])] == FRONT_COLUMNS, p.describe()
    assert len({int(cols[k][0]) for k in ("t.k2", "t.d", "t.t_u")} | {0}) == 4
    e.close()


# ---- the random generators, stepped -----------------------------------------------------------------------------------------------
ROWS_MAX = 3 * T + 200                      # the fact tables: a few tiles at the most
X_BASES = (0, -50, None, 1 << 33)           # u.x's first value; None: I32_MAX - nu + 1, the first base that gets the 64-bit sum


def clustered_index(draw, nt, lo, hi):
    """nt sorted values that go up by 0 or 1: from lo to hi where the rows allow it, else a run that starts at a random value"""
    span = min(hi - lo, nt - 1)
    if span < hi - lo:                                     # too few rows for the whole range
        span = int(draw.integers(span // 2, span + 1))
        lo = int(draw.integers(lo, hi - span + 1))
    return rising(nt, lo, draw.choice(np.arange(1, max(nt, 2)), span, replace=False) if span else [])


class Stepped:
    """Mixed into a generator: the tables redrawn small (from a stream of their own: build() draws what it always drew), the fact
    join index t.t_u clustered -- still with -1 first and nu + 1 last on seed % 3 == 0 -- and u.x, which carries the dimension's
    Greater filter, a stepped int64 column whose base is one of X_BASES; the filter's constant comes from u.x's own range."""

    def redraw(self, seed, nt, nu):
        draw = np.random.default_rng([seed, 0x57e9])
        ends = seed % 3 == 0
        self.cols["t.t_u"] = clustered_index(draw, nt, -1 if ends else 0, nu + 1 if ends else nu - 1)
        base = X_BASES[int(draw.integers(0, len(X_BASES)))]
        x = rising(nu, I32_MAX - nu + 1 if base is None else base, np.nonzero(draw.integers(0, 2, nu))[0])
        self.cols["u.x"] = x
        self.x_const = int(draw.integers(x[0], x[-1] + 1))
        for k, v in list(self.cols.items()):               # every other column keeps its values, cut or tiled to the new length
            n = nt if k.startswith("t.") else nu
            if not k.endswith(".heap") and len(v) != n:
                self.cols[k] = np.resize(v, n)
        assert qualifies(self.cols["t.t_u"]) and qualifies(x) and len(x) == nu and len(self.cols["t.t_u"]) == nt

    def const(self, k, ref):
        # (the generators write exactly one constant over the LOADED u.x: the dimension filter's; gathered copies have other ids.
        # stepped_program checks that it is there whenever u.x is filtered.)
        return super().const(self.x_const if ref == self.c["u.x"] else k, ref)


def sizes(seed, short_fact=False):
    draw = np.random.default_rng([seed, 0x51e5])
    nu = int(draw.integers(2 if short_fact else 1, 3000))
    nt = int(draw.integers(1, nu)) if short_fact else int(draw.integers(max(nu, 2), ROWS_MAX))
    return nt, nu


class SteppedSemiGen(Stepped, SemiGen):
    def __init__(self, seed, short_fact=False, sparse_domain=False):
        SemiGen.__init__(self, seed, short_fact=short_fact, sparse_domain=sparse_domain)
        nt, self.nu = sizes(seed, short_fact)              # (build() takes the modulus from self.nu)
        self.redraw(seed, nt, self.nu)


class SteppedJoinGen(Stepped, JoinGen):
    """... and, with sparse_domain, a group domain too large for the grouped scan: the plan keeps a fused front and its dimension scan"""

    def __init__(self, seed, sparse_domain=False):
        self.sparse_domain = sparse_domain                  # (before the loads: emit() reads it)
        JoinGen.__init__(self, seed)
        draw = np.random.default_rng([seed, 0x51e5])
        self.redraw(seed, int(draw.integers(1, ROWS_MAX)), int(draw.integers(1, 400)))

    def emit(self, body):
        if self.sparse_domain and body == "RangeC,val,0,64,1":
            body = "RangeC,val,0,%d,1" % (1 << 30)
        return super().emit(body)


KINDS = {"semi": lambda s: SteppedSemiGen(s), "semi_front": lambda s: SteppedSemiGen(s, sparse_domain=True),
         "semi_short": lambda s: SteppedSemiGen(s, short_fact=True, sparse_domain=s % 2 == 1),
         "join": lambda s: SteppedJoinGen(s), "join_front": lambda s: SteppedJoinGen(s, sparse_domain=True)}
# the seeds of each kind: the smallest common range with which the floors hold without a device -- the three kinds that keep a front
# then name a dimension scan in exactly ROLE_FLOOR programs (test_the_role_floors_hold_without_a_device prints the counts)
SEEDS = {kind: range(16) for kind in KINDS}
ROLE_FLOOR, WIDE_FLOOR = 10, 5
ROLES = ("semi", "dim", "front.select", "front.take")


def filters_on_x(gen, text):
    """the constants that `text` compares the loaded u.x with (Greater over u.x and a RangeV)"""
    stmt = {int(ln.split(",", 1)[0]): ln.split(",") for ln in text.splitlines() if ln}
    out = []
    for f in stmt.values():
        if f[1] == "Greater":
            a, b = int(f[3].split()[1]), int(f[5].split()[1])
            for col, k in ((a, b), (b, a)):
                if col == gen.c["u.x"] and stmt[k][1] == "RangeV" and stmt[k][5] == "0":
                    out.append(int(stmt[k][3]))
    return out


def stepped_program(kind, seed):
    gen = KINDS[kind](seed)
    text, cols = gen.build()
    x = cols["u.x"]
    # every filter on u.x compares it with the constant drawn from its own range, not with the generator's 0 .. 90
    assert all(k == gen.x_const and x[0] <= k <= x[-1] for k in filters_on_x(gen, text)), (kind, seed, filters_on_x(gen, text), gen.x_const)
    return text, cols


def count_roles(counts, roles, cols):
    """one program's step_columns() into {role prefix: programs, "wide": programs that decode a 64-bit-sum column}"""
    for r in ROLES:
        counts[r] = counts.get(r, 0) + bool(named(roles, r))
    counts["wide"] = counts.get("wide", 0) + any(sum_width(cols[c]) == 8 for cs in roles.values() for c in cs)


def test_the_stepped_generators_keep_their_shape():
    ends = wide = short = filtered = 0
    for kind, seeds in SEEDS.items():
        for seed in list(seeds)[:12]:
            text, cols = stepped_program(kind, seed)
            filtered += bool(filters_on_x(KINDS[kind](seed), text))
            assert oracle_run(text, cols) is not None
            idx, x = cols["t.t_u"], cols["u.x"]
            assert qualifies(idx) and qualifies(x) and x.dtype == np.int64 and len(idx) <= ROWS_MAX
            ends += seed % 3 == 0 and idx[0] == -1 and idx[-1] == len(x) + 1
            wide += sum_width(x) == 8
            short += kind == "semi_short" and len(idx) < len(x)
            assert all(len(v) == (len(idx) if name.startswith("t.") else len(x)) for name, v in cols.items() if not name.endswith(".heap"))
    # (the generators filter u.x in a fifth to a third of their programs: 12 to 20 of these 60 -- half the lower figure is the floor)
    assert ends >= 6 and wide >= 10 and short == 12 and filtered >= 6, (ends, wide, short, filtered)


def test_the_role_floors_hold_without_a_device(jit_cache, monkeypatch):
    """Every role a stepped column can have in a dimension scan, a semi-join scan and either side of a front is named by at least
    ROLE_FLOOR of the generated programs, and WIDE_FLOOR of them decode a column that takes the 64-bit sum -- counted over the
    programs that keep a fused front, the only ones that bind their projection scans without a device.  (With a device the plans
    that fuse as a whole report their dimension and semi-join scans too: tests/test_step_roles.py counts at least these.)"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    counts, per_kind = {}, {}
    for kind in ("semi_front", "semi_short", "join_front"):
        per_kind[kind] = {}
        for seed in SEEDS[kind]:
            text, cols = stepped_program(kind, seed)
            e = declared_engine(cols)
            roles = roles_without_a_device(e, text)
            e.close()
            count_roles(per_kind[kind], roles, cols)
        for k, v in per_kind[kind].items():
            counts[k] = counts.get(k, 0) + v
    print("programs that name a stepped column, by role:", counts, per_kind)
    assert all(counts[r] >= ROLE_FLOOR for r in ROLES) and counts["wide"] >= WIDE_FLOOR, (counts, per_kind)


# ---- the compiled plans -------------------------------------------------------------------------------------------------------------
def compiled_plan(n):
    """(text, columns) of plan n over the synthetic catalog of tests/test_step_images.py::synth"""
    return compiled(n)[1], synth(n)


# plan -> {role: stepped columns} as the binder reports it without a device, with a step image on every column that qualifies
PLAN_ROLES = {3: {"dim0": ["customer.c_mktsegment"], "front.select": [JOIN_INDEX], "front.take": [JOIN_INDEX]},
              5: {"front.select": [JOIN_INDEX]},
              9: {"front.select": [JOIN_INDEX], "front.take": [JOIN_INDEX]},
              10: {"front.select": [JOIN_INDEX], "front.take": [JOIN_INDEX]}}
# (Plan 4, the semi-join over lineitem, and every other plan fuse as a whole here: they bind their dimension and semi-join scans when
# they run, and name nothing without a device.  tests/test_step_roles.py asserts plan 4's semi-join scan on the GPU.)


@pytest.mark.parametrize("n", PLANS)
def test_compiled_plans_name_these_stepped_columns_by_role(n, jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    text, cols = compiled_plan(n)
    e = declared_engine(cols)
    roles = roles_without_a_device(e, text)
    e.close()
    print("plan", n, roles)
    assert roles == PLAN_ROLES.get(n, {}), (n, roles)


def test_some_compiled_plan_decodes_a_step_image_in_a_dimension_scan():
    assert any(named(roles, "dim") for roles in PLAN_ROLES.values())
    assert all(qualifies(compiled_plan(3)[1][c]) for c in named(PLAN_ROLES[3], "dim"))
