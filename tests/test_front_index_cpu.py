"""The look-back of the one-pass fused front without a GPU: the index functions and the prefix walk of csrc/vdl_front_index.h (which
word holds which node of the fan-out-16 tree over the batches of tiles, which batch stores which level from which 15 nodes, and the walk
in which 64 lanes stride through the nodes of a prefix) played through on the host, one count per batch, by a stand-alone program
(tools/sanitize/front_index_main.cpp).  Batch counts around every power of 16 up to 16^5 + 17 under ASan + UBSan, and the largest count
launch_project_front lets through (2^26 batches) in a plain build -- EVERY prefix of every count is checked, and the 67 M prefixes of
the largest count do not fit a test's time under the sanitizers.  This is where levels 4 to 6 of the tree run, which a device test
would need 2^29 .. 2^39 rows to reach, and the walk's second trip (batch numbers whose hex digits sum to more than 64, from 0x5FFFF
on), which no device test can reach at all.  tests/test_front_levels.py runs levels 1 to 3 on the device."""
import os
import subprocess

from conftest import ROOT
from test_step_images import FRONT_BATCH                  # tiles per batch, read from csrc/vdl_mscan_body.h

CSRC = os.path.join(ROOT, "mplan2vdl_amd", "csrc")


def _build(tmp_path, sanitize):
    exe = str(tmp_path / ("front_index" + ("_asan" if sanitize else "")))
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    cmd = ["g++", "-std=c++17", "-Wall", "-DVDL_FRONT_BATCH=%d" % FRONT_BATCH] + flags + ["-I", CSRC, os.path.join(ROOT, "tools", "sanitize", "front_index_main.cpp"), "-o", exe]
    return exe if subprocess.call(cmd) == 0 else None


def _run(exe, arg):
    """-> (checks, prefixes with a second trip, batches of the largest run let through)"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, arg], capture_output=True, text=True, env=env, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("ok "), r.stdout + r.stderr
    words = lines[-1].split()
    return int(words[1]), int(words[3]), int(lines[-2].split()[2])


def test_front_lookback_gives_every_batch_its_prefix_under_sanitizers(tmp_path):
    """1, 15, 16, 17, 255, 256, 257, 0x111, 0xFFF, 0x1000, 0x1001, 0xFFFF, 0x10000, 0x10001, 0xFFFFF, 0x100000 + 17 batches: the nodes
    built as the kernel's publisher builds them sum, walked as the kernel's last wave walks them, to every batch's exclusive prefix;
    every word lies inside front_look_words, no two nodes share a word, every word read was stored by an earlier batch, none is read
    twice.  Batches from 0x5FFFF on make a lane take a second node: some prefixes did."""
    exe = _build(tmp_path, True) or _build(tmp_path, False)       # (a compiler without the sanitizer runtimes still checks the arithmetic)
    assert exe, "the checker of the front's look-back does not build"
    checks, second_trips, _ = _run(exe, "--no-largest")
    assert checks > 250000000
    assert second_trips > 0, "no prefix made a lane walk a second time"


def test_front_lookback_at_the_largest_count_the_launcher_lets_through(tmp_path):
    """ceil((16^7 - 1) / VDL_FRONT_BATCH) = 67 108 864 batches (about 1.4 GB of nodes, owners, stamps and counts), every prefix, in a
    plain build: the same checks as above, through level 6; 3.8 M of its prefixes make a lane take a second node."""
    exe = _build(tmp_path, False)
    assert exe, "the checker of the front's look-back does not build"
    checks, second_trips, largest = _run(exe, "--largest-only")
    assert largest == ((16 ** 7 - 1) + FRONT_BATCH - 1) // FRONT_BATCH
    assert checks > 9000000000
    assert second_trips > 3000000
