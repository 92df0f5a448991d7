"""The look-back of the radix Partition without a GPU: the index functions of csrc/vdl_partition_index.h (which status row holds which
node of the fan-out-16 tree over the tiles, which rows make up a tile's prefix, which tile stores which level) played through on the
host, one count per tile, under ASan + UBSan (a stand-alone program, tools/sanitize/partition_index_main.cpp).  Tile counts around
every power of 16 up to 16^5 + 17 and the largest count launch_partition lets through: levels 3 to 5 of the tree, which a device test
would need 2^25 .. 2^37 rows to reach (tests/test_partition_levels.py runs levels 2 and 3 on the device).

And the guard of the sizes the two device test files are built on: tests/test_partition_levels.py and tests/test_scan_levels.py
place their cases at thresholds read from the kernels' constants; when one of those changes this test says which files to revisit."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "mplan2vdl_amd", "csrc")


def _build(tmp_path, sanitize):
    exe = str(tmp_path / ("partition_index" + ("_asan" if sanitize else "")))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    cmd = ["g++", "-std=c++17", "-Wall"] + flags + ["-I", CSRC, os.path.join(ROOT, "tools", "sanitize", "partition_index_main.cpp"), "-o", exe]
    return exe if subprocess.call(cmd) == 0 else None


def test_lookback_rows_give_every_tile_its_prefix_under_sanitizers(tmp_path):
    """1, 15, 16, 17, 255, 256, 257, 0x111, 0xFFF, 0x1000, 0x1001, 0xFFFF, 0x10000, 0x10001, 0xFFFFF, 0x100000 + 17 and 16^6 - 1 tiles:
    the rows built as part_pass_tile builds them sum to every tile's exclusive prefix; every row index lies inside partition_rows, no
    two nodes share a row, every row read is stored by an earlier tile; launch_partition's limit lies before the first count the
    rows cannot express."""
    exe = _build(tmp_path, True) or _build(tmp_path, False)       # (a compiler without the sanitizer runtimes still checks the arithmetic)
    assert exe, "the checker of the look-back's index arithmetic does not build"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 100000000


# ---- the constants the device tests' sizes rest on ---------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text, flags=re.S)
    assert len(found) == 1, "%s: expected to find it once in the source, found %d times" % (what, len(found))
    return found[0]


def test_the_level_tests_sizes_still_sit_on_the_kernels_thresholds():
    part, ops, index, folds = _source("vdl_partition.hip"), _source("vdl_ops.hip"), _source("vdl_partition_index.h"), _source("vdl_fold_body.h")
    scan = _one(r"void k_scan_counts\(.*?\n}\n", ops, "k_scan_counts")
    heads = _one(r"void k_sorted_heads_counted\(.*?\n}\n", part, "k_sorted_heads_counted")
    seen = {
        "VDL_PART_BLOCK": int(_one(r"#ifndef VDL_PART_BLOCK\n#define VDL_PART_BLOCK (\d+)\n#endif", part, "VDL_PART_BLOCK")),
        "VDL_PART_STEPS": int(_one(r"#ifndef VDL_PART_STEPS\n#define VDL_PART_STEPS (\d+)\n#endif", part, "VDL_PART_STEPS")),
        "kFanBits": int(_one(r"constexpr int kFanBits = (\d+),", index, "kFanBits")),
        "kFenLevels": int(_one(r"kFenLevels = (\d+);", index, "kFenLevels")),
        "kCompactWords": int(_one(r"constexpr int kCompactWords = (\d+);", folds, "kCompactWords")),
        "one-launch compaction up to kWave tiles": _one(r"if \(nb <= (\w+)\) \{[^\n]*\n\s*k_compact_count_scan<<<", ops, "launch_compact_offsets' threshold"),
        "K of k_scan_counts": int(_one(r"constexpr int K = (\d+);", scan, "K in k_scan_counts")),
        "block of k_scan_counts": int(_one(r"base \+= (\d+) \* K\)", scan, "the trip of k_scan_counts")),
        "launch of k_scan_counts": int(_one(r"k_scan_counts<<<1, (\d+), 0, s>>>", ops, "the launch of k_scan_counts")),
        "K of the last block's scan": int(_one(r"constexpr int K = (\d+);", heads, "K in k_sorted_heads_counted")),
        "trip of the last block's scan": int(_one(r"base < nb; base \+= (\d+) \* K\)", heads, "the trip of the last block's scan")),
        "kHeadMaxGrid": int(_one(r"constexpr int kHeadMaxGrid = (\d+);", part, "kHeadMaxGrid")),
        "kHeadArrivals": int(_one(r"constexpr int kHeadArrivals = (\d+);", part, "kHeadArrivals")),
        "kHeadTileGroups": int(_one(r"constexpr int kHeadTileGroups = (\d+);", part, "kHeadTileGroups")),
    }
    want = {"VDL_PART_BLOCK": 512, "VDL_PART_STEPS": 16, "kFanBits": 4, "kFenLevels": 6, "kCompactWords": 64,
            "one-launch compaction up to kWave tiles": "kWave", "K of k_scan_counts": 8, "block of k_scan_counts": 1024,
            "launch of k_scan_counts": 1024, "K of the last block's scan": 8, "trip of the last block's scan": 256,
            "kHeadMaxGrid": 2048, "kHeadArrivals": 64, "kHeadTileGroups": 16}
    changed = {k: (seen[k], want[k]) for k in want if seen[k] != want[k]}
    assert not changed, ("constants the sizes of tests/test_partition_levels.py and tests/test_scan_levels.py are derived from have changed "
                         "(found, expected): %r -- move those tests' sizes to the new thresholds (tile of a radix pass = VDL_PART_BLOCK x "
                         "VDL_PART_STEPS rows, a look-back level per 2^kFanBits tiles, compaction tile = 64 x kCompactWords rows, one-launch compaction up "
                         "to 64 tiles, 8 x 1024 counts per trip of k_scan_counts, kHeadMaxGrid blocks on kHeadArrivals counters), then update this test" % changed)
