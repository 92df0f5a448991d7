"""Lookup images without a GPU (vdl_set_lookup_images: a dimension column looked up through a join index is read from its byte
image): the rules of csrc/vdl_column_image.h applied to a looked-up value against brute force under ASan + UBSan (a stand-alone
program, tools/sanitize/lookup_image_main.cpp), and the binders and the generated code through Engine(device=None) -- columns
registered as pointers, their images declared (Engine.declare_image), every scan built by hiprtc for gfx950 (Plan.jit_check) with
Plan.lookup_columns() saying which lookup of which scan role reads an image.  The programs and catalogs of the directed tests
live here; tests/test_lookup_images.py runs them on the device against the oracle."""
import os
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from conftest import ROOT
from helpers import prog
from test_jit import code_bytes, compiled, host_engine_with_declared

CSRC = os.path.join(ROOT, "mplan2vdl_amd", "csrc")
META = os.path.join(ROOT, "tests", "golden", "tpch10noorder")
PLANS = [1, 3, 4, 5, 6, 9, 10, 11, 12, 14, 15, 16, 18, 19, 20]
# plans whose lookups must read an image over the synthetic catalog with every column encoded (the issue's floor)
MUST_LOOK_UP = (5, 9, 10, 12, 14, 19)
TPCH = {"q14": 14, "q12": 12, "q19": 19, "q3": 3}


# ---- programs in the shape the compiler emits for an FK join (tests/test_random_joins.py), written out by hand -----------------
class Builder:
    def __init__(self):
        self.lines, self.nid = [], 0

    def emit(self, body):
        self.nid += 1
        self.lines.append("%d,%s" % (self.nid, body))
        return self.nid

    def load(self, name): return self.emit("Project,val,Id %d,%s" % (self.emit("Load," + name), name.split(".", 1)[1]))
    def const(self, k, ref): return self.emit("RangeV,val,%d,Id %d,0" % (k, ref))
    def pos(self, ref): return self.emit("RangeV,val,0,Id %d,1" % ref)
    def bin(self, op, a, b): return self.emit("%s,val,Id %d,val,Id %d,val" % (op, a, b))
    def gather(self, src, p): return self.emit("Gather,Id %d,Id %d,val" % (src, p))
    def select(self, pred): return self.emit("FoldSelect,val,Id %d,val,Id %d,val" % (self.pos(pred), pred))
    def shl(self, v, k): return self.bin("BitShift", v, self.bin("Subtract", self.const(0, v), self.const(k, v)))

    def join(self, fk, dim_pkey, carried):
        """the fact side looks an unfiltered dimension up through `fk`: (carried columns cleaned, positions into the dimension)"""
        sm = self.select(self.gather(self.const(1, dim_pkey), fk))
        return [self.gather(c, sm) for c in carried], self.gather(self.gather(self.pos(dim_pkey), fk), sm)

    def fold(self, kind, t): return self.emit("%s,val,Id %d,val,Id %d,val" % (kind, self.const(0, t), t))

    def grouped(self, key, domain, terms):
        part = self.emit("Partition,val,Id %d,val,Id %d,val" % (key, self.emit("RangeC,val,0,%d,1" % domain)))
        skey = self.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (key, self.pos(key), part))
        outs = []
        for kind, t in terms:
            st = self.emit("Scatter,Id %d,Id %d,val,Id %d,val" % (t, self.pos(t), part))
            outs.append(self.emit("%s,val,Id %d,val,Id %d,val" % (kind, skey, st)))
        return outs

    def done(self, outs):
        for o in outs:
            self.emit("MaterializeCompact,Id %d" % o)
        return prog(*self.lines)


# The affine target: u.x = 7 + 1000 e (int64).  (a) a range filter on the looked-up value whose bounds are no multiples of 1000, the
# upper one beyond anything an image holds; (b) a SUM factor with a multiplier of 2^61 + 5, so that the sums wrap.
# variant "global": two global scans; "grouped": the same terms grouped by a fact column (the grouped scan); "keyed": the looked-up
# value is also a component of the group key -- a raw use, for which an affine image may not stand in.
FILTER_LO, FILTER_HI, WRAP = 20500, 10 ** 7 + 3, 2 ** 61 + 5


def affine_program(variant="global"):
    b = Builder()
    a, fk, tp, d = b.load("t.a"), b.load("t.t_u"), b.load("t.t_pkey"), b.load("t.d")
    x, up = b.load("u.x"), b.load("u.u_pkey")
    (av, dv), gm = b.join(b.gather(fk, b.pos(tp)), up, [a, d])
    xv = b.gather(x, gm)
    s1 = b.select(b.bin("Greater", xv, b.const(FILTER_LO, xv)))
    av1, xv1, dv1 = b.gather(av, s1), b.gather(xv, s1), b.gather(dv, s1)
    s2 = b.select(b.bin("Greater", b.const(FILTER_HI, xv1), xv1))
    av2, xv2, dv2 = b.gather(av1, s2), b.gather(xv1, s2), b.gather(dv1, s2)
    if variant == "global":
        wrapped = b.bin("Multiply", av, b.bin("Multiply", xv, b.const(WRAP, xv)))
        return b.done([b.fold("FoldSum", av2), b.fold("FoldCount", av2), b.fold("FoldSum", wrapped)])
    wrapped = b.bin("Multiply", av2, b.bin("Multiply", xv2, b.const(WRAP, xv2)))
    key = dv2 if variant == "grouped" else b.bin("BitwiseOr", b.shl(dv2, 6), b.bin("BitShift", xv2, b.const(12, xv2)))
    return b.done(b.grouped(key, 16 if variant == "grouped" else 512, [("FoldSum", av2), ("FoldCount", av2), ("FoldSum", wrapped)]))


def affine_cols(nu=257, nt=20000, emax=200, seed=3):
    """fact t (nt rows) with a join index into u (nu rows); a few indices lie outside u on both sides (those rows are EPS)"""
    r = np.random.default_rng(seed)
    return {"t.a": r.integers(-50, 50, nt).astype(np.int64), "t.d": r.integers(0, 7, nt).astype(np.int16), "t.t_pkey": np.zeros(nt, np.int64),
            "t.t_u": r.integers(-1, nu + 2, nt).astype(np.int64), "u.x": (7 + 1000 * (np.arange(nu) * 37 % (emax + 1))).astype(np.int64),
            "u.u_pkey": np.zeros(nu, np.int64)}


# The lookup chain t.t_u -> u.u_w (40000 .. 40256: a 2-byte image of base 40000, scale 1) -> w.z (7 + 1000 e, e <= 100: a 1-byte
# image of scale 1000), grouped over a domain too large for the grouped scan: the plan gets a fused front, whose select side needs
# u.u_w per row (the source of a further lookup: decoded after the lookup) and whose take side hands w.z over decoded.
def chain_program():
    b = Builder()
    a, fk, bb = b.load("t.a"), b.load("t.t_u"), b.load("t.b")
    f2, up, z, wp = b.load("u.u_w"), b.load("u.u_pkey"), b.load("w.z"), b.load("w.w_pkey")
    s0 = b.select(b.bin("Greater", a, b.const(10, a)))
    (av, bv), gm = b.join(b.gather(fk, s0), up, [b.gather(a, s0), b.gather(bb, s0)])
    (av2, bv2), gm2 = b.join(b.gather(f2, gm), wp, [av, bv])
    zv = b.gather(z, gm2)
    key = b.bin("BitwiseOr", b.shl(b.bin("Add", av2, b.const(50, av2)), 8), bv2)
    return b.done(b.grouped(key, 32768, [("FoldSum", zv), ("FoldMax", zv), ("FoldCount", av2)]))


def chain_cols(nt=20000, nu=300, nw=40300, seed=5):
    r = np.random.default_rng(seed)
    return {"t.a": r.integers(-50, 50, nt).astype(np.int64), "t.b": r.integers(0, 30, nt).astype(np.int32), "t.t_pkey": np.zeros(nt, np.int64),
            "t.t_u": r.integers(-1, nu + 2, nt).astype(np.int64), "u.u_w": (40000 + np.arange(nu) % 257).astype(np.int64), "u.u_pkey": np.zeros(nu, np.int64),
            "w.z": (7 + 1000 * r.integers(0, 101, nw)).astype(np.int64), "w.w_pkey": np.zeros(nw, np.int64)}


def image_of(v):
    """(width, base, scale) the engine's ingest pass chooses for these values (vdl_column_image.h choose), or None"""
    stored = v.dtype.itemsize
    if stored <= 1 or len(v) == 0:
        return None
    v = v.astype(np.int64)
    mn, mx = int(v.min()), int(v.max())

    def narrowest(lo, hi):
        return next((w for w in (1, 2, 4) if -(1 << (8 * w - 1)) <= lo and hi <= (1 << (8 * w - 1)) - 1), 8)

    p, d = 0, np.unique(v - mn)
    while p < 18 and mx > mn and np.all(d % 10 ** (p + 1) == 0):
        p += 1
    pure, aff = narrowest(mn, mx), narrowest(0, (mx - mn) // 10 ** p)
    if min(pure, aff) >= stored:
        return None
    return (pure, 0, 1) if pure <= aff else (aff, mn, 10 ** p)


def declared_engine(cols):
    """no device: every column a pointer at its own width, with the image its values would get declared; {column: image}"""
    e = host_engine_with_declared(cols)
    images = {}
    for k, v in cols.items():
        im = None if k.endswith(".heap") else image_of(v)
        if im:
            e.declare_image(k, *im)
            images[k] = im
    return e, images


# ---- the rules ----------------------------------------------------------------------------------------------------------------
def _build(tmp_path, sanitize):
    exe = str(tmp_path / ("lookup_image" + ("_asan" if sanitize else "")))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    cmd = ["g++", "-std=c++17", "-Wall"] + flags + ["-I", CSRC, os.path.join(ROOT, "tools", "sanitize", "lookup_image_main.cpp"), "-o", exe]
    return exe if subprocess.call(cmd) == 0 else None


def test_lookup_rules_match_brute_force_under_sanitizers(tmp_path):
    """widths 1 / 2, bases -3 .. 3, scales 1, 10, 1000: map_range followed by a lookup of e admits exactly the rows whose decoded
    value lies in [lo, hi], compose gives the factor's value mod 2^64, and use_in_aggregate / use_in_vscan say what the comments do"""
    exe = _build(tmp_path, True) or _build(tmp_path, False)       # (a compiler without the sanitizer runtimes still checks the rules)
    assert exe, "the checker of the lookup rules does not build"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 1000000


def test_the_python_mirror_of_the_width_choice():
    assert image_of(affine_cols()["u.x"]) == (2, 7, 1000)          # e up to 200 does not fit a signed byte
    assert image_of(affine_cols(emax=127)["u.x"]) == (1, 7, 1000)
    assert image_of(chain_cols()["u.u_w"]) == (2, 40000, 1)
    assert image_of(chain_cols()["w.z"]) == (1, 7, 1000)
    assert image_of(np.arange(100, dtype=np.int32)) == (1, 0, 1)
    assert image_of(np.arange(100, dtype=np.int8)) is None


# ---- device-less builds ----------------------------------------------------------------------------------------------------------
def lookup_targets(p):
    got = {}
    for cols in p.lookup_columns().values():
        got.update(cols)
    return got


@pytest.mark.parametrize("name", list(TPCH))
def test_tpch_lookups_build_over_declared_images_without_a_gpu(name, tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    monkeypatch.delenv("VDL_LOOKUP_IMAGES", raising=False)
    text, cols = compiled(TPCH[name], 1e-4)
    e, images = declared_engine(cols)
    p = e.parse(text)
    off = p.jit_check()
    assert ",limg" not in off and "not specialised" not in off and p.lookup_columns() == {}, (off, p.lookup_columns())
    streamed = p.image_columns()
    e.set_lookup_images(True)
    on = p.jit_check()
    assert ",limg" in on and "not specialised" not in on, on
    assert code_bytes(on) and max(code_bytes(on)) < 64 << 10, on      # (the descriptor still folds)
    got = lookup_targets(p)
    assert got and all(images[c][0] == w for c, w in got.items()), (got, images)
    want = {"q14": {"part.p_type"}, "q12": {"orders.o_orderpriority"}, "q19": {"part.p_brand", "part.p_container", "part.p_size"},
            "q3": {"orders.o_orderdate", "orders.o_shippriority"}}[name]
    assert want <= set(got), (want, got)
    assert p.image_columns() == streamed                            # lookup targets are never listed among the streamed columns
    if name != "q3":
        # the forms the tuner can pick for a join scan: staged and queue (every filter counts as selective)
        monkeypatch.setenv("VDL_JIT_ASSUME_SELECTIVITY", "0.3")
        for late in ("1", "3"):
            monkeypatch.setenv("VDL_JIT_LATE", late)
            note = p.jit_check()
            built = [x for x in note.split("; ") if "k_mscan_specialised<" in x]
            assert all(",limg" in x for x in built), note
            assert not code_bytes(note) or max(code_bytes(note)) < 64 << 10, note
        monkeypatch.delenv("VDL_JIT_LATE")
    e.set_column_images(False)                                      # column images off: the switch is ignored
    assert ",limg" not in p.jit_check() and p.lookup_columns() == {} and p.image_columns() == {}
    e.set_column_images(True)
    e.set_lookup_images(False)
    assert p.jit_check() == off and p.lookup_columns() == {}
    e.close()


def test_every_compiled_plan_binds_its_lookups_without_a_gpu():
    """the 15 compiled plans over the synthetic catalog, every column's image declared: which plans look an image up (a plan that
    fuses as a whole binds its dimension and semi-join scans when it runs, so it names fewer roles here than on the device)"""
    looked = {}
    for n in PLANS:
        text, cols = compiled(n, 1e-3, seed=7)
        e, images = declared_engine(cols)
        e.set_lookup_images(True)
        p = e.parse(text)
        try:
            note = p.jit_check()
        except m.VdlError:
            assert n == 18                                          # neither fused nor a fused front
            continue
        assert "not specialised" not in note and max(code_bytes(note)) < 64 << 10, (n, note)
        looked[n] = lookup_targets(p)
        assert ("limg" in note) == bool(looked[n]), (n, note, looked[n])
        e.close()
    for n in MUST_LOOK_UP:
        assert looked[n], (n, looked)


@pytest.mark.parametrize("variant,emax", [("global", 200), ("global", 127), ("grouped", 200), ("keyed", 200)])
def test_affine_target_binds_encoded_unless_its_value_is_a_group_key(variant, emax):
    text, cols = affine_program(variant), affine_cols(emax=emax)
    e, images = declared_engine(cols)
    assert images["u.x"] == ((2 if emax > 127 else 1), 7, 1000)
    e.set_lookup_images(True)
    p = e.parse(text)
    assert p.is_fused, p.describe()
    note = p.jit_check()
    roles = p.lookup_columns()
    if variant == "keyed":
        assert roles == {} and ",limg" not in note, (roles, note)
    else:
        scans = 2 if variant == "global" else 1
        assert roles == {"scan%d" % s: {"u.x": images["u.x"][0]} for s in range(scans)}, roles
        assert note.count(",limg") == scans, note
    e.close()


def test_lookup_chain_decodes_the_source_of_a_further_lookup():
    text, cols = chain_program(), chain_cols()
    e, images = declared_engine(cols)
    assert images["u.u_w"] == (2, 40000, 1) and images["w.z"] == (1, 7, 1000)
    e.set_lookup_images(True)
    p = e.parse(text)
    d = p.describe()
    assert "\nfused front:" in d and "w.z[col3]" in d and "u.u_w[col1]" in d, d
    note = p.jit_check()
    assert "front: vdl_jit_project_front<" in note and ",limg" in note and max(code_bytes(note)) < 64 << 10, note
    want = {"u.u_w": 2, "w.z": 1}
    assert p.lookup_columns() == {"front.select": want, "front.take": want}, p.lookup_columns()
    # a per-row value takes an image of scale 1 only: with scale 10 the source of the further lookup stays on the catalog column
    e.declare_image("u.u_w", 2, 40000, 10)
    p.jit_check()
    assert p.lookup_columns() == {"front.select": {"w.z": 1}, "front.take": {"w.z": 1}}, p.lookup_columns()
    e.close()


def test_images_are_declared_only_without_a_device_and_on_known_columns():
    e = m.Engine(device=None)
    e.register_pointer("t.a", 0x10000, 8, 100)
    with pytest.raises(m.VdlError):
        e.declare_image("t.nope", 2)
    for bad in ((3, 0, 1), (8, 0, 1), (2, 0, 0)):
        with pytest.raises(m.VdlError):
            e.declare_image("t.a", *bad)
    e.declare_image("t.a", 2, -5, 100)
    assert e.image_info("t.a") == (2, -5, 100)
    e.close()


def test_the_environment_switches_lookup_images_on_when_the_context_opens(monkeypatch):
    text, cols = affine_program("global"), affine_cols()
    for env, want in (("1", True), ("0", False), (None, False)):
        if env is None:
            monkeypatch.delenv("VDL_LOOKUP_IMAGES", raising=False)
        else:
            monkeypatch.setenv("VDL_LOOKUP_IMAGES", env)
        e, _ = declared_engine(cols)
        p = e.parse(text)
        p.jit_check()
        assert bool(p.lookup_columns()) == want, (env, p.lookup_columns())
        e.close()
