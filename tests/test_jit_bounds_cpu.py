"""Filter bounds of the specialised scans at run time (vdl_plan_set_jit_bounds, Plan.set_jit(runtime_bounds=True),
VDL_JIT_BOUNDS=runtime), without a GPU: vdl_plan_jit_check builds every form of Q6, Q1, Q14, Q12, Q19 and Q3's front and
dimension scans for a text A and for a text B that is A with the constants of its filters changed -- dates, discount, quantity,
dictionary codes -- every range keeping its shape.

With the bounds at run time the translation units of A and B (VDL_JIT_DUMP) are byte for byte the same and hold none of A's
literals, B's builds are all found in the code-object cache ($VDL_JIT_CACHE from another process, memory in the same one) and add
no file to it; with the bounds as constants (the default) the same B compiles every form again; a change of a range's shape
-- a two-sided range that becomes a point or loses a side -- is another source.

Every set of builds runs in a process of its own: a process keeps what it built in memory, dumps a source only when it has to look
further than that, and the counters of vdl_jit_counters are the process's."""
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

I64MIN = -(1 << 63)
# (VDL_JIT_LATE, census build): eager; staged with one, two, all filter columns with the tile; the queue form; census builds of
# a staged and of the queue form.  Every filter counts as selective (VDL_JIT_ASSUME_SELECTIVITY pins the staging)
FORMS = [(0, 0), (1, 0), (1, 1), (2, 0), (4, 0), (3, 0), (3, 1)]
PACKED_FORMS = [(5, 0), (5, 1), (6, 0)]                         # filters packed and the price late, its census build, every column packed
# program -> {constant of A: constant of B}, applied to the RangeV constants of the program text
CHANGES = {
    "q6": {728294: 728659, 728659: 729024, 6: 5, 24: 25},       # 1994 -> 1995, discount 0.06 -> 0.05 (+- 0.01), quantity < 24 -> < 25
    "q6_packed": {728294: 728659, 728659: 729024, 6: 5, 24: 25},
    "q1": {729999: 729939},                                     # shipdate <= 1998-12-01 - 90 days -> - 150 days
    "q14": {728902: 728932, 728932: 728963},                    # 1995-09 -> 1995-10
    "q12": {728294: 728659, 728659: 729024, 40: 64, 160: 136},  # receipt year, the two ship modes' dictionary codes
    "q19": {464: 472, 432: 440, 80: 72, 536: 544, 888: 896, 720: 728, 136: 144, 160: 168, 1072: 1080, 560: 568, 384: 392, 48: 56,
            416: 424, 840: 848, 608: 616, 5: 6, 10: 11, 15: 14},             # the containers' dictionary codes, the size ranges' ends
    "q3": {728732: 728763, 16: 24},                             # the date on both sides of the join, the market segment's code
}
# Q6's shape changes: discount between 6 - 0 and 6 + 0 is a point; shipdate from INT64_MIN on has lost its lower bound
SHAPES = {"point": {1: 0}, "one_sided": {728294: I64MIN}}
TPCH = {"q1": 1, "q14": 14, "q12": 12, "q19": 19, "q3": 3}


def changed(text, mapping):
    """the program with the RangeV constants of `mapping` replaced (all at once); every one of them occurs"""
    seen = set()

    def sub(mo):
        k = int(mo.group(2))
        if k not in mapping:
            return mo.group(0)
        seen.add(k)
        return "%s%d%s" % (mo.group(1), mapping[k], mo.group(3))

    out = re.sub(r"^(\d+,RangeV,val,)(-?\d+)(,Id \d+,0)$", sub, text, flags=re.M)
    assert seen == set(mapping), sorted(set(mapping) - seen)
    return out


def program(name):
    """(text, engine without a device over the program's declared columns)"""
    import mplan2vdl_amd as m
    from mplan2vdl_amd import datagen
    if name in ("q6", "q6_packed"):
        import test_packed_images_cpu as P
        e = m.Engine(device=None)
        for k in datagen.Q6_COLUMNS:
            e.register_pointer(k, 0x10000, P.Q6_WIDTHS[k] if name == "q6_packed" else 8, 600000)
            if name == "q6_packed":
                e.declare_packed(k, *P.Q6_PACKED[k])
        return P.q6(), e
    import test_jit as J
    text, cols = J.compiled(TPCH[name], 1e-4)
    return text, J.host_engine_with_declared(cols)


def forms_of(name):
    return [(0, 0)] if name == "q3" else PACKED_FORMS if name == "q6_packed" else FORMS


def worker(spec_path):
    """builds, in this process and in order, every form of each variant of the spec; after each variant: the counters, the cache's
    files and the note of the last form, as one JSON line per variant"""
    import mplan2vdl_amd as m
    spec = json.load(open(spec_path))
    os.environ["VDL_JIT_CACHE"] = spec["cache"]
    os.environ["VDL_JIT_ASSUME_SELECTIVITY"] = "0.3"
    os.environ["VDL_JIT_U"] = os.environ["VDL_JIT_GROUP_U"] = "2"
    text, e = program(spec["program"])
    for v in spec["variants"]:
        os.makedirs(v["dump"], exist_ok=True)
        os.environ["VDL_JIT_DUMP"] = v["dump"]
        p = e.parse(changed(text, {int(a): b for a, b in v["mapping"].items()}))
        p.set_jit(True, runtime_bounds=spec["runtime_bounds"])
        notes = []
        for late, census in forms_of(spec["program"]):
            os.environ.pop("VDL_JIT_LATE", None)
            os.environ.pop("VDL_JIT_CENSUS", None)
            if late:
                os.environ["VDL_JIT_LATE"] = str(late)
            if census:
                os.environ["VDL_JIT_CENSUS"] = "1"
            notes.append(p.jit_check())
        print(json.dumps({"counters": m.jit_counters(), "files": sorted(f for f in os.listdir(spec["cache"]) if f.endswith(".vdlco")), "notes": notes}), flush=True)
    e.close()


def build(tmp_path, tag, name, runtime_bounds, cache, variants):
    """one process: variants = [(dump directory name, mapping)]; one record per variant"""
    spec = {"program": name, "runtime_bounds": runtime_bounds, "cache": str(cache),
            "variants": [{"dump": str(tmp_path / d), "mapping": {str(a): b for a, b in mp.items()}} for d, mp in variants]}
    path = tmp_path / (tag + ".json")
    path.write_text(json.dumps(spec))
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_jit_bounds_cpu as t; t.worker(sys.argv[1])" % (ROOT, os.path.join(ROOT, "tests"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("VDL_")}
    r = subprocess.run([sys.executable, "-c", code, str(path)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def sources(d):
    """{file name: text} of a dump directory (a name holds the hash and the length of its source)"""
    return {f: open(os.path.join(d, f)).read() for f in sorted(os.listdir(d))}


def generated(src):
    """what vdl_jit.cpp writes around the embedded device code: the stage lines, the descriptor, the kernel"""
    head = "\n".join(line for line in src.splitlines() if line.startswith(("#define VDL_STAGED", "#define VDL_QUEUE")))
    return head + src[src.index("constexpr MsArgs jit_args"):]


def bound_values(src):
    """the values the descriptor text gives the ranges of filters and formula tests"""
    g = generated(src)
    vals = re.findall(r"d\.f(?:lo|hi)\[\d+\] = (\(-9223372036854775807LL - 1\)|-?\d+)(?:LL)?;", g)
    vals += [x for step in re.findall(r"d\.form\[\d+\]\.op = 0;[^\n]*", g) for x in re.findall(r"\.(?:lo|hi) = (\(-9223372036854775807LL - 1\)|-?\d+)(?:LL)?;", step)]
    return [I64MIN if v.startswith("(") else int(v) for v in vals]


def built(rec):
    return rec["counters"]["compiled"] + rec["counters"]["from_disk"]


@pytest.mark.parametrize("name", sorted(CHANGES))
def test_plans_that_differ_in_bound_values_share_their_specialised_code(name, tmp_path):
    cache = tmp_path / "cache"
    nothing, b = {}, CHANGES[name]
    # bounds at run time.  Process 1: A.  Process 2, over the cache process 1 left: B, then A again
    (a1,) = build(tmp_path, "rt1", name, True, cache, [("rt_a", nothing)])
    b2, a2 = build(tmp_path, "rt2", name, True, cache, [("rt_b", b), ("rt_a_again", nothing)])
    n = a1["counters"]["compiled"]
    # (forms with the same text -- staged with one or with two filter columns ahead, when there is one -- are one build)
    assert 1 <= n <= len(a1["notes"]) * 3 and a1["counters"]["from_disk"] == 0 and len(a1["files"]) == n, a1
    assert all("not specialised" not in x and ",rtb>" in x for x in a1["notes"]), a1["notes"]
    assert b2["counters"]["compiled"] == 0 and b2["counters"]["from_disk"] == n, (a1, b2)      # B: every build from the cache
    assert b2["files"] == a1["files"] and b2["notes"] == a1["notes"]                          # ... to which it adds no file
    assert built(a2) == built(b2) and a2["counters"]["from_memory"] > b2["counters"]["from_memory"] and a2["files"] == a1["files"]
    src_a, src_b = sources(tmp_path / "rt_a"), sources(tmp_path / "rt_b")
    assert len(src_a) == n and src_a == src_b                                                # the same translation units, byte for byte
    assert sources(tmp_path / "rt_a_again") == {}                                            # (found in memory: nothing to dump)
    # the bounds as constants: the same B compiles every form again
    (c1,) = build(tmp_path, "c1", name, False, cache, [("const_a", nothing)])
    (c2,) = build(tmp_path, "c2", name, False, cache, [("const_b", b)])
    assert c1["counters"]["compiled"] == n and c1["counters"]["from_disk"] == 0, c1
    assert c2["counters"]["compiled"] == n and c2["counters"]["from_disk"] == 0 and len(c2["files"]) == 3 * n, c2
    const_a, const_b = sources(tmp_path / "const_a"), sources(tmp_path / "const_b")
    assert not set(const_a) & set(const_b) and not set(const_a) & set(src_a)
    # the text with run-time bounds holds shapes -- (open | 0, open | 0 | 1) -- and none of A's literals
    literals = {v for s in const_a.values() for v in bound_values(s) if abs(v) >= 1000 and v not in (I64MIN, -I64MIN - 1)}
    assert literals, name
    for s in src_a.values():
        assert "#define VDL_RT_BOUNDS 1" in s
        g = generated(s)
        assert not [v for v in literals if re.search(r"(?<![\d.])%d(LL|u)\b" % v, g)], name
        assert set(bound_values(s)) <= {I64MIN, -I64MIN - 1, 0, 1}, sorted(set(bound_values(s)))
    assert all("VDL_RT_BOUNDS 1" not in s for s in const_a.values())
    assert all(any(re.search(r"(?<![\d.])%d(LL|u)\b" % v, generated(s)) for s in const_a.values()) for v in literals)


@pytest.mark.parametrize("name", ["q6", "q6_packed"])
def test_a_change_of_shape_is_another_source(name, tmp_path):
    """Q6 with the discount range a point, and with the date range open below: each builds sources of its own (and builds them:
    correct, not shared); the point's text compares for equality"""
    cache = tmp_path / "cache"
    a, point, one = build(tmp_path, "shapes", name, True, cache, [("a", {}), ("point", SHAPES["point"]), ("one_sided", SHAPES["one_sided"])])
    n = a["counters"]["compiled"]
    assert point["counters"]["compiled"] == 2 * n and one["counters"]["compiled"] == 3 * n, (a, point, one)
    src = {k: sources(tmp_path / k) for k in ("a", "point", "one_sided")}
    assert len(src["a"]) == len(src["point"]) == len(src["one_sided"]) == n
    assert not set(src["a"]) & set(src["point"]) and not set(src["a"]) & set(src["one_sided"]) and not set(src["point"]) & set(src["one_sided"])
    for s in src["point"].values():
        assert (0, 0) in zip(bound_values(s)[::2], bound_values(s)[1::2])
    for s in src["a"].values():
        assert (0, 0) not in zip(bound_values(s)[::2], bound_values(s)[1::2])
    opens = lambda d: sum(v == I64MIN for s in d.values() for v in bound_values(s))
    assert opens(src["one_sided"]) > opens(src["a"])


def test_the_environment_switches_the_mode_on_for_plans_parsed_afterwards(tmp_path, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", str(tmp_path))
    text, e = program("q6")
    plain = e.parse(text)
    monkeypatch.setenv("VDL_JIT_BOUNDS", "runtime")
    shared = e.parse(text)
    monkeypatch.delenv("VDL_JIT_BOUNDS")
    assert ",rtb>" in shared.jit_check() and ",rtb>" not in plain.jit_check()
    shared.set_jit(True, runtime_bounds=False)
    plain.set_jit(True, runtime_bounds=True)
    assert ",rtb>" not in shared.jit_check() and ",rtb>" in plain.jit_check()
    e.close()
