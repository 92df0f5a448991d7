"""The cases and references of tests/test_front_levels.py without a GPU (tests/front_cases.py): the two programs are accepted by the
oracle and keep their fused front when the engine plans them; the numpy reference equals the oracle for every survivor pattern at
sizes around 1, 2, 3 and 17 batches; the comparison the device tests use reports what an error of the front's look-back would leave
-- the survivors of one batch displaced by the count of one node, forwards and backwards --; and the constants the device tests'
sizes are derived from are still the kernels'."""
import os
import re

import numpy as np
import pytest

import front_cases as fc
import mplan2vdl_amd as m
from conftest import ROOT
from front_cases import B, T, FRONT_BATCH, FRONT_CARRY
from helpers import oracle_run

CSRC = os.path.join(ROOT, "mplan2vdl_amd", "csrc")


# ---- the programs -------------------------------------------------------------------------------------------------------------------
def _describe(text):
    e = m.Engine(device=None)
    try:
        p = e.parse(text)
        d = p.describe()
        p.close()
        return d
    finally:
        e.close()


def _front_line(description):
    (line,) = [ln for ln in description.splitlines() if "fused front" in ln]
    return line


def test_program_a_keeps_its_front_with_the_row_ids_and_both_fact_columns():
    d = _describe(fc.front_program(False)[0])
    line = _front_line(d)
    for vector in ("Id 16=rowid", "Id 17=col1", "Id 18=col2", "Id 22=rowid"):
        assert vector in line, (vector, d)
    assert fc.front_output_columns(d) == 2


def test_program_b_looks_the_dimension_up_in_the_front_and_hands_its_value_over():
    d = _describe(fc.front_program(True)[0])
    line = _front_line(d)
    for vector in ("Id 16=rowid", "Id 17=col1", "Id 18=col2", "Id 19="):
        assert vector in line, (vector, d)
    assert "d.g[col1] in [6,+inf]" in d, d
    assert fc.front_output_columns(d) == 3


SMALL = [(1, 0, 0), (0, 0, 1), (0, 0, T - 1), (0, 1, 0), (0, 1, 1), (0, 3, T - 1), (1, 0, 1), (1, 1, T - 1), (2, 0, 0), (1, 3, 1), (2, 2, 1), (3, 0, 0),
         (16, 1, 1), (17, 0, 0), (17, 2, T - 1), (17, 3, 1)]


def test_the_small_sizes_cover_every_shape_of_the_last_batch():
    sizes = [fc.rows_of(*s) for s in SMALL]
    assert {n % T for n in sizes} >= {0, 1, T - 1} and T == 2048
    assert {((n + T - 1) // T) % FRONT_BATCH for n in sizes} == {0, 1, 2, 3}
    assert {fc.batches_of(n) for n in sizes} >= {1, 2, 3, 17, 18}


@pytest.mark.parametrize("dimension_filter", [False, True], ids=["A", "B"])
@pytest.mark.parametrize("pattern", fc.PATTERNS)
def test_front_reference_is_what_the_oracle_computes(pattern, dimension_filter):
    """every pattern at 1 .. 18 batches, lengths with a partial last tile (n % T = 1, T - 1) and a last batch of 1, 2 and 3 tiles"""
    text, named = fc.front_program(dimension_filter)
    for size in SMALL:
        n = fc.rows_of(*size)
        mask = fc.pattern_mask(pattern, n)
        cols = fc.fact_columns(mask, dimension_filter, seed=n % 1000)
        assert np.array_equal(fc.selection(cols, dimension_filter), mask), (size, "the columns do not state the pattern")
        ref = fc.front_reference(cols, dimension_filter)
        assert np.array_equal(ref[fc.ROWS], np.flatnonzero(mask))
        got = fc.outputs(oracle_run(text, cols), named)
        assert not fc.front_mismatches(got, ref), (size, fc.front_mismatches(got, ref))


@pytest.mark.parametrize("extra_filters,extra_takes", [(5, 0), (9, 0), (3, 7)])
def test_the_kernel_variants_programs_are_what_the_oracle_computes(extra_filters, extra_takes):
    n = fc.rows_of(2, 1, 77)
    mask = fc.pattern_mask("signature", n)
    cols = dict(fc.fact_columns(mask, False), **fc.variant_columns(n, extra_filters, extra_takes))
    text, named = fc.front_program(False, extra_filters, extra_takes)
    ref = fc.front_reference(cols, False, extra_takes)
    got = fc.outputs(oracle_run(text, cols), named)
    assert sorted(got) == sorted(ref) and not fc.front_mismatches(got, ref)
    assert fc.front_column_counts(_describe(text)) == (1 + extra_filters, 3 + extra_filters + extra_takes)


def test_the_patterns_are_what_they_say():
    n = fc.rows_of(0x111, 2, 5)
    nb = fc.batches_of(n)
    assert nb == 0x112
    sig = fc.batch_counts(fc.pattern_mask("signature", n))
    assert np.array_equal(sig[:-1], fc.signature_count(np.arange(nb - 1))) and np.all(sig[1:-1] != sig[:-2])       # (every whole batch differs from its neighbour)
    assert set(sig[:-1].tolist()) == set(range(13))
    assert sig[:16 * (nb // 16)].reshape(-1, 16).sum(axis=1).min() > 0         # (no level-1 node is empty: dropping one shifts something)
    iso = fc.batch_counts(fc.pattern_mask("isolated", n))
    assert np.flatnonzero(iso).tolist() == [0, 14, 15, 16, 17, 254, 255, 256, 257, nb - 1]
    assert all(iso[b] == 1 << (b % 11) for b in (0, 14, 15, 16, 17, 254, 255, 256, 257))
    assert B > FRONT_CARRY > 12                                 # (`all`, `full head` and `full tail` overflow the carry area, `signature` never does)
    head = fc.batch_counts(fc.pattern_mask("full head", n))
    assert np.all(head[:256] == B) and not head[256:].any()
    tail = fc.batch_counts(fc.pattern_mask("full tail", n))
    assert not tail[:256].any() and np.all(tail[256:-1] == B) and tail[-1] == 2 * T + 5
    pos = fc.signature_positions()
    assert pos[:2] == [0, B - 1] and all(t * T - 1 in pos and t * T in pos for t in range(1, FRONT_BATCH))


# ---- what the comparison rejects ------------------------------------------------------------------------------------------------------
# (pattern, level of the node that is dropped or doubled).  The node is (16^level - 1, level): the count of the first 16^level batches.
# Batch 16^level reads that node alone; without it its survivors land `count` places early, on top of its predecessors'; with it twice
# they land `count` places late, on top of its successors'.
DISPLACED = [(pattern, level) for pattern in ("signature", "isolated") for level in (1, 2, 3)]


@pytest.fixture(scope="module")
def level_three_references():
    """the direct outputs of program A at 16^3 + 2 batches and 5 rows, once per pattern"""
    refs = {}
    n = fc.rows_of(FAN3 + 2, 0, 5)
    for pattern in ("signature", "isolated"):
        mask = fc.pattern_mask(pattern, n)
        cols = fc.fact_columns(mask, False)
        ref = fc.front_reference(cols, False)
        refs[pattern] = (ref, fc.batch_counts(mask))
    return refs


FAN3 = fc.FAN ** 3


@pytest.mark.parametrize("pattern,level", DISPLACED)
def test_the_comparison_reports_a_dropped_and_a_doubled_node(pattern, level, level_three_references):
    ref, counts = level_three_references[pattern]
    assert not fc.front_mismatches(dict(ref), ref)
    batch = fc.FAN ** level
    node = int(counts[:batch].sum())                            # the count of node (16^level - 1, level)
    assert node > 0 and counts[batch] > 0 and counts[batch + 1] > 0
    for by in (-node, node):
        got = fc.displaced(ref, counts, batch, by)
        bad = fc.front_mismatches(got, ref)
        assert fc.ROWS in bad, (pattern, level, by, bad)        # the row ids: strictly ascending, so no displaced value can equal what it covers
        assert set(bad) <= set(fc.DIRECT)
        assert np.any(np.diff(got[fc.ROWS]) <= 0)               # ... and the displaced vector is no longer ascending
    # a node of the batch's own level-0 neighbour (one batch's count) as well: the smallest shift there is
    for by in (-int(counts[batch - 1]), int(counts[batch + 1])):
        assert fc.ROWS in fc.front_mismatches(fc.displaced(ref, counts, batch, by), ref)


def test_a_lost_total_is_reported_by_the_lengths():
    n = fc.rows_of(17, 0, 0)
    mask = fc.pattern_mask("signature", n)
    ref = fc.front_reference(fc.fact_columns(mask, False), False)
    short = {name: (a[:-1] if name in fc.DIRECT else a) for name, a in ref.items()}
    assert sorted(fc.front_mismatches(short, ref)) == sorted(fc.DIRECT)
    assert fc.kept_note({"timeInMicrosecondsForFusedFront_f_5_statement_vectors_%d_of_%d_rows_kept_(dimension_side_included)" % (len(ref[fc.ROWS]), n): 1},
                        len(ref[fc.ROWS]), n)
    assert not fc.kept_note({"timeInMicrosecondsForFusedFront_f_5_statement_vectors_1%d_of_%d_rows_kept_(dimension_side_included)" % (len(ref[fc.ROWS]), n): 1},
                            len(ref[fc.ROWS]), n)


# ---- the constants the device tests' sizes rest on -------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text, flags=re.S)
    assert len(found) == 1, "%s: expected to find it once in the source, found %d times" % (what, len(found))
    return found[0]


def test_the_front_tests_sizes_still_sit_on_the_kernels_thresholds():
    body, index, engine, launch = _source("vdl_mscan_body.h"), _source("vdl_front_index.h"), _source("vdl_engine.cpp"), _source("vdl_mscan.hip")
    seen = {
        "kFrontFanBits": int(_one(r"constexpr int kFrontFanBits = (\d+),", index, "kFrontFanBits")),
        "kFrontLevels": int(_one(r"kFrontLevels = (\d+);", index, "kFrontLevels")),
        "kFrontWave": int(_one(r"constexpr int kFrontWave = (\d+);", index, "kFrontWave")),
        "VDL_FRONT_BATCH": int(_one(r"#ifndef VDL_FRONT_BATCH\n#define VDL_FRONT_BATCH (\d+)\n#endif", body, "VDL_FRONT_BATCH")),
        "VDL_PROJ_U": int(_one(r"#ifndef VDL_PROJ_U\n#define VDL_PROJ_U (\d+)", body, "VDL_PROJ_U")),
        "kMsBlock": int(_one(r"constexpr int kMsBlock = (\d+);", body, "kMsBlock")),
        "kFrontCarry": int(_one(r"constexpr int kFrontCarry = (\d+);", body, "kFrontCarry")),
        "first-run capacity: the whole table up to 2^k bytes": int(_one(r"\(n \* per_row <= \(\(int64_t\)1 << (\d+)\) \? n : 0\)", engine, "run_projection's first-run capacity")),
        "later capacity": _one(r"std::min<int64_t>\(n, (p->front_m_seen \+ p->front_m_seen / 8 \+ 4096)\)", engine, "run_projection's guess"),
        "the launcher's limit": _one(r"if \(project_tiles\(scols\.n\) >= \((\(int64_t\)1 << \(kFrontFanBits \* kFrontLevels\))\)\) return hipErrorInvalidValue;", launch,
                                     "launch_project_front's limit"),
        # the kernel takes its 15 siblings and its prefix walk from the header and spells the header's publish condition out
        "publish condition": (_one(r"for \(int j = 1; j < kFrontLevels && (\(\(batch \+ 1\) & [^;]*?) == 0; j\+\+\)", body, "the publisher's loop"),
                              _one(r"bool front_publishes\(int64_t u, int level\) \{ return (.*?) == 0; \}", index, "front_publishes").replace("u + 1", "batch + 1")
                              .replace("level", "j")),
        "siblings": len(re.findall(r"front_wait\(lk\.nodes \+ front_sibling\(nbatches, batch, j, lane\)\)", body)),
        "walk": len(re.findall(r"VDL_FRONT_PREFIX_WALK\(x, nbatches, batch, lane, VDL_FRONT_WAIT_AT\);", body)),
    }
    want = {"kFrontFanBits": 4, "kFrontLevels": 7, "kFrontWave": 64, "VDL_FRONT_BATCH": 4, "VDL_PROJ_U": 4, "kMsBlock": 256, "kFrontCarry": 512,
            "first-run capacity: the whole table up to 2^k bytes": 28, "later capacity": "p->front_m_seen + p->front_m_seen / 8 + 4096",
            "the launcher's limit": "(int64_t)1 << (kFrontFanBits * kFrontLevels)", "siblings": 1, "walk": 1}
    assert seen["publish condition"][0] == seen["publish condition"][1], ("project_front_body's publish condition is no longer the text of front_publishes "
                                                                          "(csrc/vdl_front_index.h), which the host program runs: %r" % (seen["publish condition"],))
    changed = {k: (seen[k], want[k]) for k in want if seen[k] != want[k]}
    assert not changed, ("constants the sizes of tests/test_front_levels.py and tests/front_cases.py are derived from have changed (found, expected): %r -- "
                         "move those tests' batch counts to the new thresholds (a batch = VDL_FRONT_BATCH tiles of kMsBlock x 2 x VDL_PROJ_U rows, a look-back "
                         "level per 2^kFrontFanBits batches, a first run that counts first from n x 8 x (outputs + 1) > 2^28 bytes on, kFrontCarry carried "
                         "values per batch), the batch counts of tools/sanitize/front_index_main.cpp and tests/test_front_index_cpu.py to the new levels, "
                         "the table of DESIGN.md section 5.16, then update this test" % changed)
    assert (T, FRONT_BATCH, FRONT_CARRY, fc.FAN) == (256 * 2 * 4, 4, 512, 1 << seen["kFrontFanBits"])
