#!/usr/bin/env python3
"""Compares the specialised scans' translation units of two trees: two directories of VDL_JIT_DUMP output, e.g. of the CPU suite
run in a checkout of the parent commit and in this one.

    python3 tools/jit_dump_diff.py PARENT_DUMPS THIS_DUMPS [--compile N]

A translation unit is [generated stage lines] + the embedded device code (csrc/vdl_scan_desc.h + vdl_front_index.h + vdl_mscan_body.h as text) + [the
descriptor as constants + the kernel].  A file's name holds the hash of its whole text, so a change of the embedded code renames
every file; what a change of the host code may alter is the generated parts.  Printed: the number of distinct units per side, how many
generated parts occur on both sides / on one side only, the line diff of the embedded code, and -- with --compile N -- for N units
spread over the parent's list, whether hiprtc gives the same code object for the unit with the parent's and with this tree's
embedded code (no GPU needed)."""
import ctypes
import difflib
import os
import sys

MARK = "constexpr MsArgs jit_args"           # first words of the generated descriptor (after `namespace vdl {`)
FIRST = "typedef signed char int8_t;"        # early line of the embedded code (vdl_scan_desc.h)


def split(src):
    """(generated lines ahead of the embedded code, embedded code, generated tail)"""
    a = src.index("#if defined(__HIPCC_RTC__)") if "#if defined(__HIPCC_RTC__)" in src else src.index(FIRST)
    a = src.rfind("\n", 0, a) + 1
    b = src.rindex("namespace vdl {", 0, src.index(MARK))
    return src[:a], src[a:b], src[b:]


def load(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".hip"):
            head, body, tail = split(open(os.path.join(d, f)).read())
            out[(head, tail)] = body
    return out


def hiprtc_compile(src, arch="gfx950"):
    L = hiprtc_compile.lib
    prog = ctypes.c_void_p()
    assert L.hiprtcCreateProgram(ctypes.byref(prog), src.encode(), b"vdl_jit_scan.hip", 0, None, None) == 0
    opts = (ctypes.c_char_p * 3)(("--offload-arch=" + arch).encode(), b"-O3", b"-std=c++17")
    rc = L.hiprtcCompileProgram(prog, 3, opts)
    assert rc == 0, rc
    n = ctypes.c_size_t()
    L.hiprtcGetCodeSize(prog, ctypes.byref(n))
    buf = ctypes.create_string_buffer(n.value)
    L.hiprtcGetCode(prog, buf)
    L.hiprtcDestroyProgram(ctypes.byref(prog))
    return buf.raw


def sections(elf, names=(".text", ".rodata", ".note")):
    """the named sections of a code object (ELF64, little endian): the instructions, the kernel descriptors, the metadata.  (Whole
    files never compare equal across sources: the compiler adds a symbol named after a hash of the translation unit.)"""
    import struct
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    hdr = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    strtab = elf[hdr[shstrndx][4]:hdr[shstrndx][4] + hdr[shstrndx][5]]
    out = {}
    for h in hdr:
        name = strtab[h[0]:strtab.index(b"\0", h[0])].decode()
        if name in names:
            out[name] = elf[h[4]:h[4] + h[5]]
    return out


def main():
    parent, this = load(sys.argv[1]), load(sys.argv[2])
    both = set(parent) & set(this)
    print("distinct translation units: parent %d, this tree %d" % (len(parent), len(this)))
    print("generated parts (stage lines, descriptor, kernel) on both sides: %d; parent only: %d; this tree only: %d" %
          (len(both), len(set(parent) - both), len(set(this) - both)))
    bodies_p, bodies_t = set(parent.values()), set(this.values())
    print("embedded device code: %d text(s) in the parent, %d in this tree" % (len(bodies_p), len(bodies_t)))
    if bodies_p != bodies_t and len(bodies_p) == 1 and len(bodies_t) == 1:
        a, b = next(iter(bodies_p)).splitlines(), next(iter(bodies_t)).splitlines()
        d = [l for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        print("embedded device code: %d lines removed, %d lines added of %d" % (sum(l[0] == "-" for l in d), sum(l[0] == "+" for l in d), len(a)))
    if "--compile" in sys.argv:
        n = int(sys.argv[sys.argv.index("--compile") + 1])
        hiprtc_compile.lib = ctypes.CDLL(os.environ.get("VDL_HIPRTC_LIB", "libhiprtc.so"))
        keys = sorted(both)
        picked = [keys[i * len(keys) // n] for i in range(min(n, len(keys)))]
        same = 0
        for head, tail in picked:
            x = hiprtc_compile(head + parent[(head, tail)] + tail)
            y = hiprtc_compile(head + this[(head, tail)] + tail)
            same += sections(x) == sections(y) and len(sections(x)) == 3
        print("code objects (hiprtc, gfx950) of %d units with the parent's and with this tree's embedded code: .text, .rodata and .note identical in %d" % (len(picked), same))
    return 0 if set(parent) == set(this) else 1


if __name__ == "__main__":
    sys.exit(main())
