#!/usr/bin/env python3
"""The translation units of every existing kind of specialised scan, for tools/jit_dump_diff.py:

    python3 tools/jit_dump_units.py TREE OUT

In TREE (a built checkout: this one or one of the parent commit), without a device and with no batch switch but vdl_set_batch_grouped
for the grouped kinds, calls vdl_plan_jit_check / vdl_batch_jit_check over declared columns so that VDL_JIT_DUMP = OUT/dump receives the
units of Q6, Q6 over packed images, Q1, Q14, Q12, Q19, Q3 and Q4 in every form (tests/test_jit_bounds_cpu.py forms_of) with the bounds
as constants and at run time, and of every _batch<K> kind that exists without vdl_set_batch_joins: Q6 at K = 2, 3, 4, 8, the packed
form at 3, edge_global at 4, group16 and Q1 grouped at 2, 3, 4.  OUT/notes.txt gets the notes.  Then:

    python3 tools/jit_dump_diff.py PARENT_OUT/dump THIS_OUT/dump --compile 88"""
import os, sys
tree, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, tree); sys.path.insert(0, os.path.join(tree, "tests"))
os.makedirs(out + "/dump", exist_ok=True); os.makedirs(out + "/cache", exist_ok=True)
os.chmod(out + "/cache", 0o700)
os.environ["VDL_JIT_DUMP"] = out + "/dump"
os.environ["VDL_JIT_CACHE"] = out + "/cache"
os.environ["VDL_JIT_ASSUME_SELECTIVITY"] = "0.3"
os.environ["VDL_JIT_U"] = os.environ["VDL_JIT_GROUP_U"] = "2"
import mplan2vdl_amd as m
assert os.path.realpath(m.__file__).startswith(os.path.realpath(tree)), m.__file__
import test_jit as J
import test_jit_bounds_cpu as B
import test_batch_cpu as BC
import test_batch_grouped_cpu as G
import test_scan_forms as F

notes = open(out + "/notes.txt", "w")
def forms(p, name):
    for late, census in B.forms_of(name):
        os.environ.pop("VDL_JIT_LATE", None); os.environ.pop("VDL_JIT_CENSUS", None)
        if late: os.environ["VDL_JIT_LATE"] = str(late)
        if census: os.environ["VDL_JIT_CENSUS"] = "1"
        try:
            notes.write("%s %s %s: %s\n" % (name, late, census, p.jit_check()))
        except m.VdlError as ex:
            notes.write("%s %s %s: ERROR %s\n" % (name, late, census, ex))
    os.environ.pop("VDL_JIT_LATE", None); os.environ.pop("VDL_JIT_CENSUS", None)

for name in ("q6", "q6_packed", "q1", "q14", "q12", "q19", "q3", "q4"):
    if name == "q4":
        text, cols = J.compiled(4, 1e-4); e = J.host_engine_with_declared(cols)
    else:
        text, e = B.program(name)
    for rt in (False, True):
        p = e.parse(text)
        p.set_jit(True, runtime_bounds=rt)
        forms(p, name if name != "q4" else "q14")
    e.close()

# the batch kinds
text, e = B.program("q6")
for k in (2, 3, 4, 8):
    notes.write("q6 batch %d: %s\n" % (k, e.batch_jit_check(BC.q6_plans(e, text, k))))
e.close()
os.environ["VDL_JIT_PIN"] = "u=2,late=6"
text, e = B.program("q6_packed")
plans = [e.parse(B.changed(text, BC.literal_set(k))) for k in range(3)]
for p in plans: p.set_jit(True, tune=True)
notes.write("q6 packed batch 3: %s\n" % e.batch_jit_check(plans))
e.close()
del os.environ["VDL_JIT_PIN"]
text, cols = F.program("edge_global", 5000)
e = F.declared_engine(cols)
plans = [e.parse(text) for _ in range(4)]
for p in plans: p.set_jit(True)
notes.write("edge_global batch 4: %s\n" % e.batch_jit_check(plans))
e.close()
e = F.declared_engine(G.columns(5000))
e.set_batch_grouped(True)
for k in (2, 3, 4):
    os.environ["VDL_BATCH_WIDTH"] = str(k)
    notes.write("group16 batch %d: %s\n" % (k, e.batch_jit_check(G.parsed(e, G.texts_of(G.SETS[:k])))))
e.close()
text, cols = J.compiled(1, 1e-4)
e = J.host_engine_with_declared(cols)
e.set_batch_grouped(True)
for k in (2, 3, 4):
    os.environ["VDL_BATCH_WIDTH"] = str(k)
    plans = [e.parse(B.changed(text, {729999: 729999 - 60 * i}) if i else text) for i in range(k)]
    for p in plans: p.set_jit(True)
    notes.write("q1 batch %d: %s\n" % (k, e.batch_jit_check(plans)))
e.close()
print(len(os.listdir(out + "/dump")), "units dumped")
