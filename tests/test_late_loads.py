"""Late loads of the staged scan forms without branches (csrc/vdl_mscan_body.h buf_load_pair).

A staged form reads a column for the rows still in.  Written as `if (in) v = *p`, each such load sat in a branch of its own and
the compiler waited for it there, so a row slice's late loads were serial round trips.  The generated stage code now loads a
lane's row pair through a buffer resource over the tile, and a pair that is out passes an offset past the resource: the load
returns 0 and asks memory for nothing.  VDL_JIT_BRANCHY_LATE=1 builds the branchy form again, for profiles that compare the two
in one process.

CPU: the staged forms of Q6, Q12, Q14 and Q19 build without a GPU (census builds too) and their stage code has no per-row
conditional load in the pair path.  GPU: pinned staged forms give the oracle's answer bit for bit with the switch on and off,
the census counts the same lines either way, and a staged Q6 over raw SF100 columns (4.8 GB each, images off) keeps the
revenue of the SQL loop."""
import glob
import os
import re
import subprocess
import sys

import pytest

import test_scan_forms as F
from mplan2vdl_amd import datagen

QUERIES = ("q6", "q12", "q14", "q19")
# (u, late) staged forms tried per query; those a scan does not have are skipped (test_scan_forms.REFUSED says why)
STAGED = [(2, 1), (3, 1), (3, 2), (2, 4), (3, 4)]


@pytest.fixture(scope="module")
def jit_cache(tmp_path_factory):
    d = tmp_path_factory.mktemp("jit_cache")
    os.chmod(d, 0o700)
    return str(d)


def stage_macros(src):
    """the generated VDL_STAGED_PRE and VDL_STAGED_POST lines of a dumped translation unit"""
    return [ln for ln in src.splitlines() if ln.startswith("#define VDL_STAGED_PRE") or ln.startswith("#define VDL_STAGED_POST")]


def pair_paths(line):
    """the pair sections of a stage line: from each `if (RW % 2 == 0) {` to the scalar fallback's `} else {`"""
    return re.findall(r"if \(RW % 2 == 0\) \{(.*?)\} \} else \{", line)


def dump_forms(name, out, census, branchy):
    """(run in a child process: the engine compiles a source once per process and dumps it only then) every staged form of
    STAGED that the scan has, every filter selective, dumped under out/<name>_u<u>_l<late>/"""
    text, cols = F.tpch(name, scale=1e-4)
    e = F.declared_engine(cols)
    p = e.parse(text)
    os.environ["VDL_JIT_ASSUME_SELECTIVITY"] = "0.3"
    for k, on in (("VDL_JIT_CENSUS", census), ("VDL_JIT_BRANCHY_LATE", branchy)):
        if on:
            os.environ[k] = "1"
        else:
            os.environ.pop(k, None)
    for u, late in STAGED:
        if F.expected_refusal(name, u, late, True):
            continue
        d = os.path.join(out, "%s_u%d_l%d" % (name, u, late))
        os.mkdir(d)
        os.environ.update(VDL_JIT_DUMP=d, VDL_JIT_U=str(u), VDL_JIT_GROUP_U=str(u), VDL_JIT_LATE=str(late))
        note = p.jit_check()
        assert "not specialised" not in note and " (late)" in note, (name, u, late, note)
    p.close()
    e.close()


def build_forms(name, tmp_path, census, branchy=False):
    """{(u, late): [stage lines]} of the forms dump_forms builds"""
    env = dict(os.environ, VDL_JIT_CACHE=str(tmp_path / "cache"), PYTHONPATH=os.pathsep.join([F.ROOT, os.path.join(F.ROOT, "tests")]))
    subprocess.run([sys.executable, os.path.abspath(__file__), name, str(tmp_path), str(int(census)), str(int(branchy))], env=env,
                   cwd=os.path.join(F.ROOT, "tests"), check=True, timeout=600)
    out = {}
    for u, late in STAGED:
        srcs = glob.glob(str(tmp_path / ("%s_u%d_l%d" % (name, u, late)) / "*.hip"))
        if not srcs:                        # (refused, or the source of a form before -- Q12's lateall is its late form)
            continue
        assert len(srcs) == 1, (name, u, late, srcs)
        out[(u, late)] = stage_macros(open(srcs[0]).read())
    assert out, name
    return out


@pytest.mark.parametrize("census", (False, True), ids=("plain", "census"))
@pytest.mark.parametrize("name", QUERIES)
def test_staged_stage_code_has_no_conditional_load(name, census, tmp_path):
    for form, lines in build_forms(name, tmp_path, census).items():
        assert lines, (name, form)
        late_loads = 0
        for line in lines:
            for path in pair_paths(line):
                late_loads += 1
                assert "buf_load_pair<" in path and "buf_rsrc(" in path, (name, form, path)
                # the only load under a condition is the partial tile's unpaired last row (`two_` folds to true in full tiles)
                conditional = re.findall(r"if \(([^)]*)\) v\[\d+\]\[r1?\] = load_scalar", path)
                assert conditional and all(c.startswith("!two_ && ") for c in conditional), (name, form, path)
                assert "*(const " not in path, (name, form, path)
                assert ("__ballot" in path) == census, (name, form, census)
        assert late_loads > 0, (name, form, lines)


@pytest.mark.parametrize("name", QUERIES)
def test_branchy_switch_builds_the_earlier_form(name, tmp_path):
    for form, lines in build_forms(name, tmp_path, False, branchy=True).items():
        paths = [p for ln in lines for p in pair_paths(ln)]
        assert paths, (name, form)
        for path in paths:
            assert "buf_load_pair" not in path and re.search(r"if \(\w+\[r\] \| \w+\[r1\]\) \{", path), (name, form, path)


# ---- GPU ----------------------------------------------------------------------------------------------------------------
def pinned_forms(name):
    return [(u, late) for u, late in STAGED if not F.expected_refusal(name, u, late, F.SELECTIVE_ON_GPU[name])]


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUERIES)
def test_branch_free_and_branchy_late_loads_agree_with_the_oracle(name, jit_cache, monkeypatch):
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    full_text, full_cols = F.program(name)
    for u, late in pinned_forms(name):
        n = F.row_counts(u)[-1]                                     # (37 tiles and an odd tail)
        cols = F.sliced(full_cols, n, F.passing_row(name, full_text, full_cols))
        want = F.oracle_of(name, n, full_text, cols)
        monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % (u, late))
        for images in (True, False):
            e = F.gpu_engine(cols, images)
            for branchy in (False, True):
                if branchy:
                    monkeypatch.setenv("VDL_JIT_BRANCHY_LATE", "1")
                got, note, _ = F.run_pinned(e, full_text, u, late)
                monkeypatch.delenv("VDL_JIT_BRANCHY_LATE", raising=False)
                assert got == want, (name, u, late, images, branchy, note)
                F.check_form(name, u, late, note, images, None)
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("q6", "q14"))
def test_census_counts_the_same_lines_as_the_branchy_form(name, jit_cache, monkeypatch):
    """a masked lane asks for nothing: the census of the branch-free form equals that of the branchy one, column by column"""
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    text, cols = F.program(name)
    e = F.gpu_engine(cols, True)
    for u, late in pinned_forms(name):
        monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % (u, late))
        traffic = []
        for branchy in (False, True):
            if branchy:
                monkeypatch.setenv("VDL_JIT_BRANCHY_LATE", "1")
            p = e.parse(text)
            p.set_jit(True, tune=True)
            p.run()
            traffic.append(p.scan_traffic())
            p.close()
            monkeypatch.delenv("VDL_JIT_BRANCHY_LATE", raising=False)
        assert traffic[0] == traffic[1], (name, u, late, traffic)
        assert "late:" in str(traffic[0]), (name, u, late, traffic)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("u,late", [(3, 1), (3, 4)])
def test_staged_q6_over_raw_sf100_columns(u, late, q6_text, jit_cache, monkeypatch):
    """columns of 4.8 GB (int64, images off): a tile's resource starts at the tile, so its offsets stay 32 bits"""
    import oracle
    import torch

    free, _ = torch.cuda.mem_get_info(0)
    if free < 24 * 2**30:
        pytest.skip("needs 24 GiB of free HBM")
    n = datagen.LINEITEM_ROWS["sf100"]
    specs = [(datagen.SEED, datagen.col_id(c), datagen.LINEITEM[c].lo, datagen.LINEITEM[c].hi, datagen.LINEITEM[c].mul,
              datagen.LINEITEM[c].add) for c in datagen.Q6_COLUMNS]
    rev, _ = oracle.sql_q6_generated(specs, 0, n, threads=16)
    monkeypatch.setenv("VDL_JIT_CACHE", jit_cache)
    monkeypatch.setenv("VDL_JIT_PIN", "u=%d,late=%d" % (u, late))
    e = F.m.Engine(device=0)
    for name in datagen.Q6_COLUMNS:
        e.generate(datagen.LINEITEM[name], 0, n)
    e.set_column_images(False)
    p = e.parse(q6_text)
    p.set_jit(True, tune=True)
    res = p.run()
    note = p.jit_note()
    assert p.image_columns().get("scan0", {}) == {}, p.image_columns()
    assert re.search(r"-> k_mscan_specialised<\d+,%d,[^>]*%s>" % (u, F.SUFFIX[late]), note), note
    assert res["results"] == {"tmp42": {".revenue": [rev]}}, note
    p.close()
    e.close()


if __name__ == "__main__":
    dump_forms(sys.argv[1], sys.argv[2], sys.argv[3] == "1", sys.argv[4] == "1")
