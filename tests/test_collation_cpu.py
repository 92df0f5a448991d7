"""Text keys of the order step, the device-free part: vdl_collate_host -- the definition of a heap's collation ranks -- against
Python's own order of `bytes` (unsigned, a prefix before its extensions); vdl_plan_set_order_text's argument handling on a
host-only context; vdlrun's --order-by FIELD[:asc|:desc][:text[=HEAP]] syntax.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib
from conftest import ROOT

VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")


def golden(name):
    return open(os.path.join(ROOT, "tests", "golden", name)).read()


def lay_out(pieces):
    """pieces: bytes objects laid down one after the other exactly as given (strings WITH the NULs and padding the test wants).
    Returns (heap bytes, [offset of every piece])."""
    buf, at = bytearray(), []
    for p in pieces:
        at.append(len(buf))
        buf += p
    return bytes(buf), at


def python_ranks(heap, codes):
    """The issue's definition, in Python: the strings that start in the heap (non-NUL byte after a NUL or at offset 0, cut at the
    next NUL or the heap's end), sorted(set(...)) of them as `bytes` -- which compares unsigned and puts a prefix first --, rank
    1 + index; a NUL byte is rank 0; anything else -1."""
    n = len(heap)
    starts = [i for i in range(n) if heap[i] != 0 and (i == 0 or heap[i - 1] == 0)]
    text = {i: heap[i:].split(b"\0", 1)[0] for i in starts}
    order = {s: k + 1 for k, s in enumerate(sorted(set(text.values())))}
    out = []
    for c in codes:
        if c < 0 or c >= n:
            out.append(-1)
        elif heap[c] == 0:
            out.append(0)
        else:
            out.append(order[text[c]] if c in text else -1)
    return out, text


A40 = b"the quick brown fox jumps over the lazy!"          # 40 bytes
assert len(A40) == 40


def edge_heap():
    """Every shape the issue lists, at whatever offsets the pieces fall on (nothing is aligned): lengths 1, 7, 8, 9, 15, 16, 17, 40;
    pairs that first differ at byte 8 and at byte 16 (the seams of the 8-byte order words); a string and its own prefix; first
    bytes 0x7f / 0x80 / 0xff; one string at two offsets; a last string without NUL."""
    strs = [b"a", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefghijklmno", b"abcdefghijklmnop", b"abcdefghijklmnopq", A40,
            b"abcdefghX", b"abcdefghY",                                   # first differ at byte 8
            b"abcdefghijklmnopX", b"abcdefghijklmnopY",                   # ... at byte 16
            b"abc", b"ab",                                                # a string and its prefix
            b"\x7fz", b"\x80a", b"\xffa", b"\x80", b"\xff\xff",
            b"abcdefgh",                                                  # again, at another offset: the same rank
            b"a",                                                         # and the one-byte string again
            b"zz\x80zz"]
    pieces = [b"\0\0\0"]                                                  # offset 0 is NUL; the first start is at 3
    for k, s in enumerate(strs):
        pieces.append(s + b"\0" * (1 + k % 3))                            # one to three NULs behind each: starts at every alignment
    pieces.append(b"tail-without-nul")
    heap, at = lay_out(pieces)
    return heap, at[1:], strs + [b"tail-without-nul"]


def test_collate_host_equals_sorted_set_of_bytes_on_every_edge():
    heap, at, strs = edge_heap()
    assert len({a % 8 for a in at}) >= 6 and heap[-1] != 0                # starts at (nearly) every alignment; no NUL at the end
    codes = list(range(len(heap)))                                        # every offset: starts, NULs and mid-string bytes
    got, bad, first = m.collate_host(heap, codes)
    want, text = python_ranks(heap, codes)
    assert got.tolist() == want
    assert sorted(text) == at and [text[a] for a in at] == strs
    rank = dict(zip(at, (got[a] for a in at)))
    dup = [a for a, s in zip(at, strs) if s == b"abcdefgh"]
    assert len(dup) == 2 and rank[dup[0]] == rank[dup[1]] > 0             # one string, two offsets, one rank
    by = {s: rank[a] for a, s in zip(at, strs)}
    assert by[b"ab"] < by[b"abc"] and by[b"abcdefgh"] < by[b"abcdefghX"] < by[b"abcdefghY"] < by[b"abcdefghi"]
    assert by[b"abcdefghijklmnop"] < by[b"abcdefghijklmnopX"] < by[b"abcdefghijklmnopY"] < by[b"abcdefghijklmnopq"]
    assert by[b"zz\x80zz"] < by[b"\x7fz"] < by[b"\x80"] < by[b"\x80a"] < by[b"\xffa"] < by[b"\xff\xff"]      # unsigned: 0x80 and 0xff come last
    assert max(by.values()) == len(set(strs)) and min(by.values()) == 1   # dense
    n_mid = sum(1 for c in codes if heap[c] != 0 and c not in text)
    assert bad == n_mid > 0 and first == at[1] + 1                        # the first mid-string byte: the second byte of "abcdefg"
    assert all(got[c] == 0 for c in codes if heap[c] == 0)


def test_collate_host_bad_codes_come_back_minus_one_with_count_and_first_row():
    heap, at, strs = edge_heap()
    n = len(heap)
    codes = [at[0], at[3], -1, n, at[3] + 2, at[5], 2 ** 40, -2 ** 62, 0]
    got, bad, first = m.collate_host(heap, codes)
    want, _ = python_ranks(heap, codes)
    assert got.tolist() == want and [k for k, r in enumerate(want) if r < 0] == [2, 3, 4, 6, 7]
    assert (bad, first) == (5, 2)
    got, bad, first = m.collate_host(heap, [at[2], at[1]])
    assert (bad, first) == (0, -1) and got[0] > got[1] > 0
    got, bad, first = m.collate_host(heap, [])
    assert len(got) == 0 and (bad, first) == (0, -1)


def test_collate_host_all_nul_empty_and_single_byte_heaps():
    got, bad, first = m.collate_host(b"\0" * 13, list(range(-1, 14)))
    assert got.tolist() == [-1] + [0] * 13 + [-1] and (bad, first) == (2, 0)
    got, bad, first = m.collate_host(b"", [0, -1, 5])
    assert got.tolist() == [-1, -1, -1] and (bad, first) == (3, 0)
    got, bad, first = m.collate_host(b"x", [0, 1])
    assert got.tolist() == [1, -1] and (bad, first) == (1, 1)
    got, _, _ = m.collate_host(np.frombuffer(b"b\0a\0\0b", dtype=np.int8), [0, 2, 5, 1, 3, 4])
    assert got.tolist() == [2, 1, 2, 0, 0, 0]


@pytest.mark.parametrize("seed", range(6))
def test_collate_host_random_heaps_with_prefixes_and_duplicates(seed):
    rng = np.random.default_rng(seed)
    alphabet = np.array([ord("a"), ord("b"), ord("c"), 0x80, 0xff], dtype=np.uint8)
    pieces = [b"\0" * int(rng.integers(0, 4))]
    for _ in range(400):
        s = bytes(rng.choice(alphabet, size=int(rng.integers(0, 41))))
        pieces.append(s + b"\0" * int(rng.integers(1, 10)))
    if seed % 2:
        pieces.append(b"cab")                                             # no NUL at the end
    heap, _ = lay_out(pieces)
    codes = list(range(-2, len(heap) + 2))
    got, bad, first = m.collate_host(heap, codes)
    want, text = python_ranks(heap, codes)
    assert got.tolist() == want and len(set(text.values())) < len(text)  # duplicates did occur
    assert bad == sum(1 for r in want if r < 0) and first == 0


def test_collate_host_rejects_bad_arguments():
    L = _lib.load()
    assert L.vdl_collate_host(None, 4, None, 0, None, None, None) == _lib.VDL_ERR_ARG
    assert L.vdl_collate_host(None, -1, None, 0, None, None, None) == _lib.VDL_ERR_ARG
    assert L.vdl_collate_host(None, 0, None, 3, None, None, None) == _lib.VDL_ERR_ARG
    assert L.vdl_collate_host(None, 0, None, 0, None, None, None) == _lib.VDL_OK


# ---- vdl_plan_set_order_text: no device, no run ----------------------------------------------------------------------------------

DATE, REV = "o_orderdate__orders__o_orderdate", "revenue"


def test_set_order_text_needs_a_key_of_the_current_order():
    e = m.Engine(device=None)
    p = e.parse(golden("q3.vdl"))
    with pytest.raises(m.VdlError) as ei:                                 # before any order
        p.set_order_text(DATE, "orders.o_orderdate.heap")
    assert ei.value.code == _lib.VDL_ERR_ARG and DATE in str(ei.value) and "no order" in str(ei.value)
    p.set_order([(REV, True)], limit=10)
    with pytest.raises(m.VdlError) as ei:                                 # an output, but no key
        p.set_order_text(DATE, "orders.o_orderdate.heap")
    assert ei.value.code == _lib.VDL_ERR_ARG and DATE in str(ei.value) and "not a key" in str(ei.value)
    with pytest.raises(m.VdlError) as ei:                                 # no output at all
        p.set_order_text("nosuchfield", "x.heap")
    assert ei.value.code == _lib.VDL_ERR_ARG and "nosuchfield" in str(ei.value)
    with pytest.raises(m.VdlError) as ei:
        p.set_order_text(REV, "")
    assert ei.value.code == _lib.VDL_ERR_ARG
    p.set_order_text(REV, "t.revenue.heap")                               # a key: by its field name ...
    p.set_order_text("tmp110", "t.revenue.heap")                          # ... or its tmpN key; twice is the same mark
    p.set_order_text(REV, None)                                           # cleared
    p.set_order_text(REV, None)
    e.close()


def test_set_order_with_heaps_is_set_order_plus_marks_and_a_new_order_replaces_the_keys():
    """A host-only context cannot run, but it says what it would have needed: with a mark the sharded refusal and the device
    error come first as ever; the marks themselves are observable through the third tuple element of set_order, which is
    set_order + set_order_text, and through a set_order_text that fails once set_order has replaced the keys."""
    e = m.Engine(device=None)
    p = e.parse(golden("q3.vdl"))
    p.set_order([(DATE, False, "orders.o_orderdate.heap"), (REV, True)], limit=5)
    p.set_order_text(DATE, "orders.other.heap")                           # still a key
    p.set_order([(REV, True)])                                            # a new order: DATE is no key any more, and REV carries no mark
    with pytest.raises(m.VdlError) as ei:
        p.set_order_text(DATE, None)
    assert ei.value.code == _lib.VDL_ERR_ARG
    with pytest.raises(m.VdlError) as ei:
        p.set_order([(REV, True, "t.r.heap"), ("nosuchfield", False, "t.x.heap")])
    assert ei.value.code == _lib.VDL_ERR_ARG and "nosuchfield" in str(ei.value)
    with pytest.raises(m.VdlError) as ei:
        p.run()
    assert ei.value.code == _lib.VDL_ERR_DEVICE
    p.set_order([])
    assert p.order_note() == ""
    e.close()


def test_collation_entry_points_without_a_device():
    e = m.Engine(device=None)
    with pytest.raises(m.VdlError) as ei:
        e.build_collation("part.p_brand.heap")
    assert ei.value.code == _lib.VDL_ERR_DEVICE
    with pytest.raises(m.VdlError) as ei:
        e.collation_info("part.p_brand.heap")
    assert ei.value.code == _lib.VDL_ERR_COLUMN
    e.register_pointer("part.p_brand.heap", 0x1000, 1, 64)
    assert e.collation_info("part.p_brand.heap") == (False, 0, 0, 0)
    e.close()


# ---- vdlrun ----------------------------------------------------------------------------------------------------------------------

def q16_text():
    from mplan2vdl_amd import frontend
    meta = os.path.join(ROOT, "tests", "golden", "tpch10noorder")
    return frontend.compile_plan(open(os.path.join(meta, "16.sql.mplan")).read(), frontend.load_metadata(meta))


def describe(order_by, text):
    return subprocess.run([VDLRUN, "--describe", "--order-by", order_by], input=text, capture_output=True, text=True, timeout=60)


def test_vdlrun_accepts_text_keys_in_describe_without_a_device():
    text = q16_text()
    assert "p_brand__part__p_brand" in text
    for spec in ("p_brand__part__p_brand:text", "p_brand__part__p_brand:text=part.p_brand.heap:desc", "p_brand__part__p_brand:desc:text",
                 "p_brand__part__p_brand:asc:text=part.p_brand.heap,p_type__part__p_type:text,p_size__part__p_size"):
        r = describe(spec, text)
        assert r.returncode == 0 and r.stdout, (spec, r.stderr)
    r = describe("nosuchfield__t__c:text", text)                          # the syntax is fine, the field is no output
    assert r.returncode != 0 and "nosuchfield__t__c" in r.stderr and "usage" not in r.stderr


@pytest.mark.parametrize("spec,says", [("revenue:text", "no heap can be derived"), ("x:text=", None), ("x:text:text", None), ("x:text=a.heap:text", None),
                                       ("x:desc:asc", None), ("x:texts", None), (":text", None), ("a__b:text", "no heap can be derived"),
                                       ("a__b__c__d:text", "no heap can be derived")])
def test_vdlrun_rejects_malformed_text_keys_with_usage(spec, says):
    r = subprocess.run([VDLRUN, "--order-by", spec], input=golden("q3.vdl"), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    assert "usage: vdlrun" in r.stderr and ":text[=HEAP]" in r.stderr
    if says:
        assert says in r.stderr and spec.split(":")[0] in r.stderr


def test_collation_kernels_are_built_for_gfx950():
    mk = open(os.path.join(ROOT, "mplan2vdl_amd", "csrc", "Makefile")).read()
    assert "vdl_collate.hip" in mk
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in ("k_col_mark", "k_col_lengths", "k_col_words", "k_col_heads", "k_col_table_init", "k_col_table_ranks", "k_ord_textkey"):
        assert k.encode() in blob, k
