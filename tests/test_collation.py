"""ORDER BY on string keys: the collation index of a heap column (vdl_collate.hip) and the order step's text keys.

The reference of every check is Python: the strings of the heap as `bytes`, `sorted(set(..))` of them for the ranks (bytes compare
unsigned and put a prefix before its extensions), and for ordered runs np.lexsort over those ranks with the position last -- the
order of `sorted` on (bytes.., position).  vdl_collate_host, which tests/test_collation_cpu.py pins to the same definition, is the
second reference of the index.  Every comparison is exact.

A case of the issue that this catalog cannot build: a heap with a validity mask that cuts a string short.  A catalog column is
{pointer, width, rows} (vdl_register_column / vdl_upload_column); validity bitmaps exist only on vectors inside a run, so a heap
column never carries one and the case is left out."""
import csv
import io
import json
import os
import subprocess

import numpy as np
import pytest

import mplan2vdl_amd as m
from mplan2vdl_amd import _lib, catalog, frontend, resolve
from conftest import ROOT
from helpers import engine_with, prog
from test_random_programs import Gen
from test_tpch_plans import META

pytestmark = pytest.mark.gpu

VDLRUN = os.path.join(ROOT, "mplan2vdl_amd", "bin", "vdlrun")
ALPHABET = np.array([ord("a"), ord("b"), ord("c"), 0x80, 0xff], dtype=np.uint8)


def host(v):
    if type(v).__name__ == "DeviceValues":
        import torch
        return torch.as_tensor(v, device="cuda:0").cpu().numpy().astype(np.int64)
    return np.asarray(v, dtype=np.int64)


def random_heap(rng, d, aligned, max_len=40):
    """A heap in which exactly d strings start: lengths drawn from 0..max_len over three letters plus 0x80 / 0xff (a draw of 0 leaves
    one more NUL: the empty string), starts at multiples of 8 (`aligned`) or wherever they fall; every third heap ends without a NUL;
    heap_n is no multiple of 8."""
    buf, starts = bytearray(int(rng.integers(0, 3)) if not aligned else 8), []
    lens = rng.integers(0, max_len + 1, size=2 * d + 8)
    body = rng.choice(ALPHABET, size=int(lens.sum()) + 1).tobytes()
    at = 0
    for ln in lens:
        if len(starts) == d:
            break
        ln = int(ln)
        if aligned:
            buf += b"\0" * (-len(buf) % 8)
        if ln:
            starts.append(len(buf))
        buf += body[at:at + ln] + b"\0" * (1 if aligned else int(1 + (at % 3)))
        at += ln
    assert len(starts) == d
    open_end = d % 3 == 0 and d > 0 and not aligned
    if open_end:
        while buf[-1] == 0:
            buf.pop()                                                      # the last string runs to the heap's end
    if len(buf) % 8 == 0:
        buf += b"c" if open_end else b"\0"
    return bytes(buf), starts


def strings_of(heap, starts):
    ends = [heap.find(b"\0", s) for s in starts]
    return [heap[s:e if e >= 0 else len(heap)] for s, e in zip(starts, ends)]


def python_ranks(heap, starts):
    text = strings_of(heap, starts)
    order = {s: k + 1 for k, s in enumerate(sorted(set(text)))}
    return np.array([order[t] for t in text], dtype=np.int64), text


def as_column(heap):
    return np.frombuffer(heap, dtype=np.int8).copy()


# ---- 5. the index equals the host ranks ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("d", [0, 1, 3, 65, 4097, 70001])
def test_index_equals_host_ranks(d, aligned):
    rng = np.random.default_rng(7 * d + aligned)
    heap, starts = random_heap(rng, d, aligned)
    n = len(heap)
    assert n % 8 != 0 and (not aligned or all(s % 8 == 0 for s in starts)) and (aligned or d < 60 or len({s % 8 for s in starts}) == 8)
    e = engine_with({"t.s.heap": as_column(heap)})
    assert e.collation_info("t.s.heap") == (False, 0, 0, 0)
    e.build_collation("t.s.heap")
    want_ranks, text = python_ranks(heap, starts)
    longest = max((len(t) for t in text), default=0)
    assert e.collation_info("t.s.heap") == (True, d, len(set(text)), longest)
    # every start, every offset of a small heap, and a sample of NULs, mid-string bytes and codes outside the heap of a large one
    others = np.arange(-3, n + 3) if n < 5000 else np.concatenate([rng.integers(-5, n + 5, size=20000), [-1, n, n - 1, 0]])
    codes = np.concatenate([np.array(starts, dtype=np.int64), others.astype(np.int64)])
    got, bad, first = e.collate("t.s.heap", codes)
    ref, rbad, rfirst = m.collate_host(heap, codes)
    assert np.array_equal(got, ref) and (bad, first) == (rbad, rfirst)
    assert np.array_equal(got[:d], want_ranks)                              # ... and Python's sorted(set(bytes)) directly
    if d >= 4097:
        assert len(set(text)) < d and bad > 0 and (got[d:] == 0).any()      # duplicates, bad codes and empty strings all occurred
    e.close()


def test_boundary_string_lengths_and_the_refusal_of_257_bytes():
    def heap_with(longest):
        parts = [b"\0", b"b" * 255 + b"\0", b"b" * longest + b"\0\0\0", b"b" * 254 + b"c\0", b"a\0", b"b" * 248 + b"\0"]
        heap = b"".join(parts)
        starts = np.cumsum([0] + [len(p) for p in parts])[1:-1]
        return heap, [int(s) for s in starts]

    heap, starts = heap_with(256)                                           # 256 bytes: 32 whole words, the terminator in none of them
    e = engine_with({"t.s.heap": as_column(heap)})
    got, bad, _ = e.collate("t.s.heap", starts)
    want, _ = python_ranks(heap, starts)
    assert bad == 0 and np.array_equal(got, want) and e.collation_info("t.s.heap") == (True, 5, 5, 256)
    heap, starts = heap_with(257)
    e.upload("t.s.heap", as_column(heap))
    with pytest.raises(m.VdlError) as ei:
        e.build_collation("t.s.heap")
    assert ei.value.code == _lib.VDL_ERR_UNSUPPORTED and "t.s.heap" in str(ei.value) and "257" in str(ei.value) and "256" in str(ei.value)
    assert e.collation_info("t.s.heap") == (False, 0, 0, 0)
    e.upload("t.w", np.arange(10, dtype=np.int64))
    with pytest.raises(m.VdlError) as ei:
        e.build_collation("t.w")                                            # no heap: eight bytes per slot
    assert ei.value.code == _lib.VDL_ERR_ARG and "t.w" in str(ei.value)
    e.close()


# ---- 6. ordered runs of a single-table program -----------------------------------------------------------------------------------------

def filter_program():
    """Load a, b, c, f; keep the rows where f != 0; outputs ka, kb, kc (the shape of LINEITEM_FILTER in tests/test_order.py: a
    FoldSelect and a MaterializeCompact per column)."""
    g = Gen.__new__(Gen)
    g.lines, g.nid = [], 0
    v = {c: g.project(g.emit("Load,t.%s" % c), c) for c in "abcf"}
    sel = g.emit("FoldSelect,val,Id %d,val,Id %d,val" % (g.rangev(0, v["f"], 1), v["f"]))
    for c in "abc":
        g.emit("MaterializeCompact,Id %d" % g.emit("Project,k%s,Id %d,val" % (c, g.gather(v[c], sel))))
    return prog(*g.lines)


class TextTable:
    """Two heaps -- t.a.heap with arbitrary starts, ~300 strings of which many occur at two offsets; t.b.heap 8-aligned, 40 strings -- and
    for each the Python rank of every code a column may hold (starts and a few NUL offsets: the empty string)."""

    def __init__(self):
        rng = np.random.default_rng(2024)
        self.heap_a, sa = random_heap(rng, 300, aligned=False, max_len=12)
        self.heap_b, sb = random_heap(rng, 40, aligned=True, max_len=20)
        self.codes, self.rank = {}, {}
        for name, heap, starts in (("a", self.heap_a, sa), ("b", self.heap_b, sb)):
            ranks, text = python_ranks(heap, starts)
            nuls = [i for i in range(len(heap)) if heap[i] == 0][:2]
            self.codes[name] = np.array(starts + nuls, dtype=np.int64)
            self.rank[name] = np.full(len(heap), -1, dtype=np.int64)        # offset -> Python's rank
            self.rank[name][starts] = ranks
            self.rank[name][nuls] = 0
            if name == "a":
                assert len(set(text)) < len(text) - 20                      # the same string at two offsets, often

    def columns(self, rng, n):
        cols = {"t.a": rng.choice(self.codes["a"], size=n), "t.b": rng.choice(self.codes["b"], size=n), "t.c": rng.integers(-2, 3, size=n, dtype=np.int64),
                "t.f": (rng.integers(0, 8, size=n) > 0).astype(np.int64) if n > 1 else np.ones(n, np.int64),
                "t.a.heap": as_column(self.heap_a), "t.b.heap": as_column(self.heap_b)}
        return cols

    def expected(self, unordered, keys, limit):
        """np.lexsort over (position, last key, .., first key): a text key by its Python rank, a descending key complemented"""
        cols = {next(iter(v))[1:]: host(next(iter(v.values()))) for v in unordered.values()}
        rows = len(cols["ka"])
        ks = []
        for field, desc, heap in keys:
            k = cols[field]
            if heap:
                k = self.rank[heap.split(".")[1]][k]
                assert (k >= 0).all()
            ks.append(~k if desc else k)
        order = np.lexsort(tuple([np.arange(rows, dtype=np.int64)] + ks[::-1]))
        if limit > 0:
            order = order[:limit]
        return {f: v[order] for f, v in cols.items()}, rows


TABLE = None


def table():
    global TABLE
    if TABLE is None:
        TABLE = TextTable()
    return TABLE


HA, HB = "t.a.heap", "t.b.heap"
ORDERS = [[("ka", False, HA)], [("ka", True, HA)], [("kc", False, None), ("ka", False, HA)], [("ka", False, HA), ("kc", True, None)],
          [("kb", True, HB), ("ka", False, HA)]]


@pytest.mark.parametrize("n", [1, 64, 4097, 200003])
def test_ordered_runs_with_text_keys(n):
    t = table()
    rng = np.random.default_rng(n)
    cols = t.columns(rng, n)
    text = filter_program()
    e = engine_with(cols)
    p = e.parse(text)
    plain = p.run(as_numpy=True)["results"]
    first = True
    for device_outputs in (False, True):
        p.set_device_outputs(device_outputs)
        for limit, path in ((10, "topn"), (4096, "topn"), (0, "sort"), (5000, "sort")):
            for keys in ORDERS:
                p.set_order(keys, limit=limit)
                res = p.run(as_numpy=True)
                want, rows = t.expected(plain, keys, limit)
                note = p.order_note()
                got = {next(iter(v))[1:]: host(next(iter(v.values()))) for v in res["results"].values()}
                for f in want:
                    assert np.array_equal(got[f], want[f]), (f, keys, limit, note)
                n_text = sum(1 for k in keys if k[2])
                assert note.endswith(" text_keys=%d" % n_text) and (rows < 2 or note.startswith(path)), note
                assert ("timeInMicrosecondsForCollation_" + HA in res["timings"]) == first, (note, sorted(res["timings"]))
                assert "timeInMicrosecondsForOrder" in res["timings"]
                first = False
    # by the code instead of the text the same rows come out in another order: the duplicates' offsets do not interleave
    if n >= 4097:
        p.set_device_outputs(False)
        p.set_order([("ka", False), ("kc", False)])
        by_code = host(p.run(as_numpy=True)["results"][list(plain)[2]][".kc"])
        want, _ = t.expected(plain, [("ka", False, HA), ("kc", False, None)], 0)
        assert not np.array_equal(by_code, want["kc"])
        assert p.order_note().startswith("sort") and "text_keys" not in p.order_note()
    e.close()


# ---- 7. / 8. TPC-H plans over the synthetic catalog ----------------------------------------------------------------------------------

def decode_column(cols, path, codes):
    heap = cols[path + ".heap"].tobytes()
    out = []
    for c in codes:
        c = int(c)
        end = heap.find(b"\0", c)
        out.append(heap[c:end if end >= 0 else len(heap)])
    return out


def rank_of(strings):
    order = {s: k for k, s in enumerate(sorted(set(strings)))}
    return np.array([order[s] for s in strings], dtype=np.int64)


def test_q12_orders_its_host_assembled_groups_by_the_text_of_l_shipmode():
    cfg = frontend.load_metadata(META)
    text = frontend.compile_plan(open(os.path.join(META, "12.sql.mplan")).read(), cfg)
    cols = catalog.synth_columns(META, cfg, text, scale=1e-3, seed=7, extra=("lineitem.l_shipmode.heap",))
    e = engine_with(cols)
    p = e.parse(text)
    assert p.is_fused
    plain = p.run(as_numpy=True)["results"]
    names = {next(iter(v))[1:]: t for t, v in plain.items()}
    mode = [f for f in names if f.startswith("l_shipmode")][0]
    codes = host(plain[names[mode]]["." + mode])
    assert len(codes) >= 2
    strings = decode_column(cols, "lineitem.l_shipmode", codes)
    for desc in (False, True):
        p.set_order([(mode, desc, "lineitem.l_shipmode.heap")])
        res = p.run(as_numpy=True)
        note = p.order_note()
        assert note.startswith("host") and note.endswith(" text_keys=1"), note
        r = rank_of(strings)
        order = np.lexsort((np.arange(len(r)), ~r if desc else r))
        for tmp, v in plain.items():
            (k, vals), = v.items()
            assert np.array_equal(host(res["results"][tmp][k]), host(vals)[order]), (tmp, note)
        got = decode_column(cols, "lineitem.l_shipmode", host(res["results"][names[mode]]["." + mode]))
        assert got == sorted(strings, reverse=desc)
    e.close()


@pytest.mark.parametrize("limit", [0, 100])
def test_q16_with_its_own_order_by(limit):
    """order by supplier_cnt desc, p_brand, p_type, p_size -- the expected order from the unordered run of the same plan (pinned by
    the parity tests), its codes decoded through the heaps"""
    cfg = frontend.load_metadata(META)
    text = frontend.compile_plan(open(os.path.join(META, "16.sql.mplan")).read(), cfg)
    cols = catalog.synth_columns(META, cfg, text, scale=5e-3, seed=3, extra=("part.p_brand.heap", "part.p_type.heap"))
    e = engine_with(cols)
    p = e.parse(text)
    plain = p.run(as_numpy=True)["results"]
    names = {next(iter(v))[1:]: t for t, v in plain.items()}
    col = {f: host(plain[t]["." + f]) for f, t in names.items()}
    cnt = [f for f in names if "supplier_cnt" in f][0]
    brand, ptype, size = "p_brand__part__p_brand", "p_type__part__p_type", "p_size__part__p_size"
    rows = len(col[cnt])
    assert rows > 100
    rb, rt = rank_of(decode_column(cols, "part.p_brand", col[brand])), rank_of(decode_column(cols, "part.p_type", col[ptype]))
    order = np.lexsort((np.arange(rows), col[size], rt, rb, ~col[cnt]))
    if limit:
        order = order[:limit]
    p.set_order([(cnt, True), (brand, False, "part.p_brand.heap"), (ptype, False, "part.p_type.heap"), size], limit=limit)
    res = p.run(as_numpy=True)
    note = p.order_note()
    assert note.endswith(" text_keys=2") and note.split()[0] == ("topn" if limit else "sort"), note
    for f, t in names.items():
        assert np.array_equal(host(res["results"][t]["." + f]), col[f][order]), (f, note)
    # the text order is not the code order here: the run by codes differs
    p.set_order([(cnt, True), brand, ptype, size], limit=limit)
    other = p.run(as_numpy=True)["results"]
    assert any(not np.array_equal(host(other[t]["." + f]), col[f][order]) for f, t in names.items())
    e.close()


# ---- 9. refusal ------------------------------------------------------------------------------------------------------------------

def test_a_code_inside_a_string_is_refused_and_the_plan_runs_again_once_restored():
    t = table()
    rng = np.random.default_rng(99)
    n = 10000
    cols = t.columns(rng, n)
    cols["t.f"] = np.ones(n, np.int64)
    e = engine_with(cols)
    p = e.parse(filter_program())
    keys = [("kc", False, None), ("ka", True, HA)]
    p.set_order(keys, limit=50)
    good = p.run(as_numpy=True)["results"]
    row = 7777
    inside = [int(c) for c in t.codes["a"] if t.rank["a"][c] > 0 and c + 1 < len(t.heap_a) and t.heap_a[int(c) + 1] != 0][0] + 1
    broken = cols["t.a"].copy()
    broken[row] = inside
    e.upload("t.a", broken)
    for limit in (50, 0):
        p.set_order(keys, limit=limit)
        with pytest.raises(m.VdlError) as ei:
            p.run()
        msg = str(ei.value)
        assert ei.value.code == _lib.VDL_ERR_SHAPE and "'ka'" in msg and HA in msg and "but 1 of" in msg and "row %d" % row in msg, msg
    e.upload("t.a", cols["t.a"])
    p.set_order(keys, limit=50)
    again = p.run(as_numpy=True)["results"]
    for tmp in good:
        (k, v), = good[tmp].items()
        assert np.array_equal(host(again[tmp][k]), host(v))
    p.set_order([("ka", False, "t.nosuch.heap")])
    with pytest.raises(m.VdlError) as ei:
        p.run()
    assert ei.value.code == _lib.VDL_ERR_ARG and "t.nosuch.heap" in str(ei.value)
    e.close()


# ---- 10. the index is cached with its column ------------------------------------------------------------------------------------------

def test_the_index_is_built_once_and_goes_with_its_column():
    heap = b"\0\0\0\0\0\0\0\0pear\0\0\0\0apple\0\0\0fig\0\0\0\0\0kiwi\0\0\0\0"
    starts = [8, 16, 24, 32]
    assert [heap[s:heap.find(b"\0", s)] for s in starts] == [b"pear", b"apple", b"fig", b"kiwi"]
    n = 1000
    rng = np.random.default_rng(3)
    cols = {"t.a": rng.choice(np.array(starts, dtype=np.int64), size=n), "t.b": np.zeros(n, np.int64), "t.c": np.arange(n, dtype=np.int64),
            "t.f": np.ones(n, np.int64), "t.a.heap": as_column(heap)}
    e = engine_with(cols)
    p = e.parse(filter_program())
    p.set_order([("ka", False, HA)], limit=0)
    label = "timeInMicrosecondsForCollation_" + HA
    assert e.collation_info(HA) == (False, 0, 0, 0)
    one = p.run(as_numpy=True)
    assert label in one["timings"] and e.collation_info(HA) == (True, 4, 4, 5)
    two = p.run(as_numpy=True)
    assert label not in two["timings"] and not [k for k in two["timings"] if "Collation" in k]
    for tmp in one["results"]:
        (k, v), = one["results"][tmp].items()
        assert host(v).tobytes() == host(two["results"][tmp][k]).tobytes()
    first_code = lambda r: int(host(next(iter(r["results"].values()))[".ka"])[0])          # noqa: E731
    assert first_code(two) == 16                                            # apple
    changed = heap.replace(b"pear", b"aaaa")
    e.upload(HA, as_column(changed))
    assert e.collation_info(HA) == (False, 0, 0, 0)
    three = p.run(as_numpy=True)
    assert label in three["timings"] and e.collation_info(HA) == (True, 4, 4, 5)
    assert first_code(three) == 8                                           # what was pear now sorts first
    e.drop(HA)
    with pytest.raises(m.VdlError) as ei:
        p.run()
    assert ei.value.code == _lib.VDL_ERR_ARG and HA in str(ei.value)
    e.close()


# ---- 11. batched runs -----------------------------------------------------------------------------------------------------------

def test_run_batch_applies_a_text_order_as_run_does():
    cfg = frontend.load_metadata(META)
    text = frontend.compile_plan(open(os.path.join(META, "12.sql.mplan")).read(), cfg)
    cols = catalog.synth_columns(META, cfg, text, scale=1e-3, seed=7, extra=("lineitem.l_shipmode.heap",))
    t = table()
    cols.update(t.columns(np.random.default_rng(5), 5000))
    e = engine_with(cols)
    q12 = [e.parse(text) for _ in range(2)]
    mode = [next(iter(v))[1:] for v in q12[0].run()["results"].values() if next(iter(v)).startswith(".l_shipmode")][0]
    for p in q12:
        p.set_order([(mode, True, "lineitem.l_shipmode.heap")])
    flt = e.parse(filter_program())
    flt.set_order([("ka", False, HA), ("kc", True, None)], limit=20)
    plans = q12 + [flt]
    alone = [p.run(as_numpy=True)["results"] for p in plans]
    notes = [p.order_note() for p in plans]
    together = e.run_batch(plans, as_numpy=True)
    assert all(n.endswith("text_keys=1") for n in notes) and [p.order_note() for p in plans] == notes
    for a, b in zip(alone, together):
        assert list(a) == list(b["results"])
        for tmp in a:
            (k, v), = a[tmp].items()
            assert np.array_equal(host(v), host(b["results"][tmp][k]))
    e.close()


# ---- 12. the CLI ----------------------------------------------------------------------------------------------------------------

NAME_PROGRAM = prog(
    "1,Load,t.f", "2,Project,val,Id 1,f", "3,RangeV,val,0,Id 2,1", "4,FoldSelect,val,Id 3,val,Id 2,val",
    "5,Load,t.name", "6,Project,val,Id 5,name", "7,Gather,Id 6,Id 4,val", "8,Project,name__t__name,Id 7,val", "9,MaterializeCompact,Id 8",
    "10,Load,t.v", "11,Project,val,Id 10,v", "12,Gather,Id 11,Id 4,val", "13,Project,v,Id 12,val", "14,MaterializeCompact,Id 13")


def test_vdlrun_orders_by_text_and_resolve_decodes_alphabetical_names(tmp_path):
    rng = np.random.default_rng(12)
    names = ["Customer#%09d" % k for k in rng.permutation(3000)[:500]]
    heap, where = bytearray(16), {}
    for s in names:                                                         # 8-aligned, in shuffled order: code order is not text order
        heap += b"\0" * (-len(heap) % 8)
        where[s] = len(heap)
        heap += s.encode() + b"\0"
    n = 20000
    code = np.array([where[s] for s in names], dtype=np.int64)
    cols = {"t.name": rng.choice(code, size=n), "t.v": rng.integers(0, 1000, size=n, dtype=np.int64), "t.f": (rng.integers(0, 4, size=n) > 0).astype(np.int64),
            "t.name.heap": as_column(bytes(heap))}
    d = str(tmp_path / "cols")
    catalog.export_columns(cols, d)
    with open(os.path.join(d, "dictionary.csv"), "w", newline="") as fh:
        csv.writer(fh).writerows(("t", "name", s, where[s]) for s in names)
    kept = cols["t.f"] != 0
    by_code = {c: s for s, c in where.items()}
    rows = sorted(((by_code[int(c)], -int(v), i) for i, (c, v) in enumerate(zip(cols["t.name"][kept], cols["t.v"][kept]))))[:5]
    r = subprocess.run([VDLRUN, "--data", d, "--order-by", "name__t__name:text,v:desc", "--limit", "5"], input=NAME_PROGRAM.encode(), capture_output=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    reply = json.load(io.BytesIO(r.stdout))
    assert "timeInMicrosecondsForCollation_t.name.heap" in reply["timings"] and "timeInMicrosecondsForOrder" in reply["timings"]
    cols_out, decoded = resolve.decode(reply, resolve.load_dictionary(os.path.join(d, "dictionary.csv")))
    assert [c.lstrip(".") for c in cols_out] == ["name", "v"] and decoded == [[s, -v] for s, v, _ in rows]
    assert [row[0] for row in decoded] == sorted(row[0] for row in decoded)
    # a heap that is not among the exported columns: the usual error
    r = subprocess.run([VDLRUN, "--data", d, "--order-by", "name__t__name:text=t.other.heap", "--limit", "5"], input=NAME_PROGRAM.encode(),
                       capture_output=True, timeout=300)
    assert r.returncode != 0 and b"t.other.heap" in r.stderr and b"columns.csv" in r.stderr
