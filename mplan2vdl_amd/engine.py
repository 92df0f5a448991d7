"""Host-side mirror of the reference's executor interface.

In the reference the executor is reached as text over a pipe: VDL in, JSON out
(/root/reference/eval_query.sh:18-26; reply shape /root/reference/resolve.py:8-32).
``Engine.run_vdl(text)`` is that request/response pair as a function call; everything it
does goes through the C ABI of libvdl.so (include/vdl.h) into hand-written HIP kernels.
"""
import ctypes
import weakref

import numpy as np

from . import _lib
from . import datagen


class VdlError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("[vdl error %d] %s" % (code, message))
        self.code = code


def prelude_counters():
    """Prelude tables built in this process so far (vdl.h: vdl_prelude_counters): {"items": LIKE tables, dimension bitmaps and semi-join
    sets, one count per table and run}."""
    L = _lib.load()
    a = ctypes.c_int64()
    L.vdl_prelude_counters(ctypes.byref(a))
    return {"items": a.value}


def jit_counters():
    """Builds of specialised scan code in this process so far (vdl.h: vdl_jit_counters): {"compiled": by hiprtc, "from_disk": read
    from $VDL_JIT_CACHE, "from_memory": built earlier in this process}."""
    L = _lib.load()
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    L.vdl_jit_counters(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return {"compiled": a.value, "from_disk": b.value, "from_memory": c.value}


class DeviceValues:
    """An output left in device memory (Plan.set_device_outputs): int64 values at `ptr`, valid until the plan runs again."""

    def __init__(self, ptr, n, owner):
        self.ptr, self.n, self._owner = int(ptr), int(n), owner

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.n,), "typestr": "<i8", "data": (self.ptr, False), "version": 3, "strides": None}

    def __len__(self):
        return self.n


class Plan:
    def __init__(self, engine, handle, text):
        self._e = engine
        self._h = handle
        self.text = text

    def close(self):
        if self._h:
            self._e._L.vdl_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def describe(self):
        return self._e._L.vdl_plan_describe(self._h).decode()

    @property
    def is_fused(self):
        return bool(self._e._L.vdl_plan_is_fused(self._h))

    def set_fusion(self, enabled):
        self._e._check(self._e._L.vdl_plan_set_fusion(self._h, int(bool(enabled))))

    def set_profiling(self, enabled):
        self._e._check(self._e._L.vdl_plan_set_profiling(self._h, int(bool(enabled))))

    def set_jit(self, enabled, tune=False, runtime_bounds=None):
        """Scan kernels specialised for this plan by hiprtc at the next run; tune: rows per lane chosen by timing at that
        run (vdl.h: vdl_plan_set_jit).  runtime_bounds: the specialised code reads the values of the filter bounds from the plan's
        descriptor, so that plans which differ in their literals alone share it (vdl.h: vdl_plan_set_jit_bounds); None leaves
        the plan's setting (off, unless VDL_JIT_BOUNDS=runtime was set when it was parsed) as it is."""
        self._e._check(self._e._L.vdl_plan_set_jit(self._h, (2 if tune else 1) if enabled else 0))
        if runtime_bounds is not None:
            self._e._check(self._e._L.vdl_plan_set_jit_bounds(self._h, int(bool(runtime_bounds))))

    def jit_note(self):
        return self._e._L.vdl_plan_jit_note(self._h).decode()

    def jit_check(self):
        """Build (not load, not run: no GPU needed) the specialised kernels against the registered columns; the note."""
        self._e._check(self._e._L.vdl_plan_jit_check(self._e._c, self._h))
        return self.jit_note()

    def image_columns(self):
        """{role: {catalog column: image width}} of the scans as bound at the last run or jit_check (vdl.h:
        vdl_plan_image_columns): roles "scan<k>", "front.select", "front.take", "dim<k>", "semi<k>"; roles that read no image are left out."""
        text = ctypes.c_char_p()
        self._e._check(self._e._L.vdl_plan_image_columns(self._h, ctypes.byref(text)))
        return _lib.parse_image_columns((text.value or b"").decode())

    def step_columns(self):
        """{role: [catalog column, ...]} of the scans that read a column from its step image, as bound at the last run or jit_check
        (vdl.h: vdl_plan_step_columns); such a column is not in image_columns() under that role.  {} when none does."""
        text = ctypes.c_char_p()
        self._e._check(self._e._L.vdl_plan_step_columns(self._h, ctypes.byref(text)))
        return _lib.parse_step_columns((text.value or b"").decode())

    def lookup_columns(self):
        """{role: {target column: image width}} of the lookups that read the image of their target column (Engine.set_lookup_images),
        as bound at the last run or jit_check (vdl.h: vdl_plan_lookup_columns); the roles are image_columns()'s, and a lookup target
        is never listed there.  {} when no lookup reads an image."""
        text = ctypes.c_char_p()
        self._e._check(self._e._L.vdl_plan_lookup_columns(self._h, ctypes.byref(text)))
        return _lib.parse_image_columns((text.value or b"").decode())

    def set_trace(self, enabled):
        """Keep a host copy of every statement's vector (statement-by-statement runs only): see `traced()`."""
        self._e._check(self._e._L.vdl_plan_set_trace(self._h, int(bool(enabled))))

    def traced(self):
        """[(statement id, form, n, values or None, holds_value or None)] of the last traced run, in execution order."""
        L, out = self._e._L, []
        for k in range(L.vdl_n_traced(self._h)):
            node, form, n = ctypes.c_int(), ctypes.c_char_p(), ctypes.c_int64()
            vals, ok = ctypes.POINTER(ctypes.c_int64)(), ctypes.POINTER(ctypes.c_uint8)()
            L.vdl_traced(self._h, k, ctypes.byref(node), ctypes.byref(form), ctypes.byref(n), ctypes.byref(vals), ctypes.byref(ok))
            if ok or n.value == 0:      # null pointers = not evaluated at that point (an empty vector has nothing to point at either)
                v = np.ctypeslib.as_array(vals, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int64)
                o = np.ctypeslib.as_array(ok, shape=(n.value,)).astype(bool) if n.value else np.zeros(0, bool)
            else:
                v = o = None
            out.append((node.value, form.value.decode(), n.value, v, o))
        return out

    def set_device_outputs(self, enabled):
        """Large outputs (>= 65536 values) stay in HBM: `collect()` returns them as `DeviceValues` (device pointer +
        length, `__cuda_array_interface__`: `torch.as_tensor(v, device=...)` wraps them without a copy).  They belong
        to the plan until its next run."""
        self._e._check(self._e._L.vdl_plan_set_device_outputs(self._h, int(bool(enabled))))

    def set_wide_sums(self, mode, sharded=False, tail=False):
        """Exact 128-bit SUM results (vdl.h: vdl_plan_set_wide_sums).  0: off -- sums wrap around in int64 and results have the
        types they always had.  1: wide -- `run()` / `collect()` return every output as a list of exact Python ints of any size
        (as_numpy=True: an object-dtype array of them); `collect_words()` hands out the (lo, hi) int64 pairs instead.  2: checked
        -- as 1, and a run in which a value does not fit int64 raises VdlError with code VDL_ERR_OVERFLOW naming output, group and
        value.  Only plans that fuse as a whole are served; every other route raises VDL_ERR_UNSUPPORTED with its reason.
        `sharded=True` (with mode 1 or 2) switches the wide merge of sharded runs on (vdl_plan_set_wide_sums_sharded):
        `run_sharded` and the `run_sharded_begin` / `_end` pair then accept the plan on the fold route, every rank ends with the
        exact answer of the whole table, and mode 2 is checked on the merged values.  Every call passes it down, so a later plain
        set_wide_sums(..) switches it off again.
        `tail=True` (with mode 1 or 2) lets `run()` also serve the plans whose sums run through the per-operator folds
        (vdl_plan_set_wide_sums_tail): a GROUP BY tail behind a fused front, fusion off, the rerun of a fused plan that found keys
        outside the pivots.  A wide sum that reaches an output through Project / Shuffle / MaterializeCompact is delivered exact; one
        that any other statement reads must fit int64, or the run raises VDL_ERR_OVERFLOW naming that statement.  Passed down by
        every call like `sharded`; the sharded entry points refuse such a plan either way."""
        self._e._check(self._e._L.vdl_plan_set_wide_sums(self._h, int(mode)))
        self._e._check(self._e._L.vdl_plan_set_wide_sums_sharded(self._h, int(bool(sharded) and int(mode) != 0)))
        self._e._check(self._e._L.vdl_plan_set_wide_sums_tail(self._h, int(bool(tail) and int(mode) != 0)))

    @property
    def wide_sums(self):
        return int(self._e._L.vdl_plan_wide_sums(self._h))

    @property
    def wide_sums_sharded(self):
        return bool(self._e._L.vdl_plan_wide_sums_sharded(self._h))

    @property
    def wide_sums_tail(self):
        return bool(self._e._L.vdl_plan_wide_sums_tail(self._h))

    def high_device(self):
        """{tmpN: DeviceValues or None} of the last run: the high words of the outputs that stayed in device memory
        (set_device_outputs with wide sums in the tail; vdl.h: vdl_output_high_device), None for every other output."""
        L, out = self._e._L, {}
        for k in range(L.vdl_n_outputs(self._h)):
            tmp, dev, n = ctypes.c_char_p(), ctypes.POINTER(ctypes.c_int64)(), ctypes.c_size_t()
            L.vdl_output(self._h, k, None, ctypes.byref(tmp), None, None)
            self._e._check(L.vdl_output_high_device(self._h, k, ctypes.byref(dev), ctypes.byref(n)))
            out[tmp.value.decode()] = DeviceValues(ctypes.cast(dev, ctypes.c_void_p).value, n.value, self) if dev else None
        return out

    def wide_note(self):
        """What served the plan's scans in the last wide run ("wide: k_mscan<...> grouped, 7 sums"), or "refused: <reason>"."""
        return (self._e._L.vdl_plan_wide_note(self._h) or b"").decode()

    def collect_words(self):
        """{tmpN: (lo, hi)} of the last run as int64 arrays: what vdl_output and vdl_output_high hand out; hi is None after a
        run with wide sums off."""
        L, out = self._e._L, {}
        for k in range(L.vdl_n_outputs(self._h)):
            tmp = ctypes.c_char_p()
            vals, high, n = ctypes.POINTER(ctypes.c_int64)(), ctypes.POINTER(ctypes.c_int64)(), ctypes.c_size_t()
            L.vdl_output(self._h, k, None, ctypes.byref(tmp), ctypes.byref(vals), ctypes.byref(n))
            L.vdl_output_high(self._h, k, ctypes.byref(high), None)
            grab = lambda p: np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value and p else np.zeros(0, np.int64)      # noqa: E731
            # (an output of no values has no high vector to point at: it is the empty one while the switch is on)
            has_high = bool(high) or (n.value == 0 and self.wide_sums != 0)
            out[tmp.value.decode()] = (grab(vals), grab(high) if has_high else None)
        return out

    def set_order(self, keys, limit=0, sharded=False):
        """ORDER BY / LIMIT on the device: `keys` is a list of (field, descending) pairs (a bare string = ascending), a field
        being an output's full name or its "tmpN" key; `limit` 0 = all rows.  Every output of `run()` then comes back permuted
        by that one order (signed int64 keys, ties in the order of the unordered result) and cut to the limit.  No keys and
        limit 0 clears it.  A string field is its dictionary code: ordered as a number it groups equal strings but is not
        alphabetical.  A third element, (field, descending, heap), declares the key as text over that heap column
        ("part.p_brand.heap"): it is then ordered by the strings themselves -- unsigned bytes, a prefix before its extensions,
        equal strings at different offsets tie -- through the heap's collation index (`Engine.build_collation`; built by the
        first run that needs it otherwise).  The heap must be in the catalog when the plan runs.
        `sharded=True` switches the merged order of sharded runs on (vdl_plan_set_order_sharded): `run_sharded` and the
        `run_sharded_begin` / `_end` pair then accept the plan and every rank ends with the same ordered answer; on the exchange
        route the limit must be 1..4096.  Every call passes it down, so a later plain set_order(..) switches it off again."""
        triples = []
        for k in keys:
            if isinstance(k, (str, bytes)):
                triples.append((k, False, None))
            else:
                triples.append((k[0], bool(k[1]), k[2] if len(k) > 2 else None))
        n = len(triples)
        enc = lambda t: t.encode() if isinstance(t, str) else t       # noqa: E731
        fields = (ctypes.c_char_p * max(n, 1))(*[enc(f) for f, _, _ in triples])
        desc = (ctypes.c_int * max(n, 1))(*[int(d) for _, d, _ in triples])
        self._e._check(self._e._L.vdl_plan_set_order(self._h, n, fields, desc, int(limit)))
        self._e._check(self._e._L.vdl_plan_set_order_sharded(self._h, int(bool(sharded))))
        for f, _, heap in triples:
            if heap is not None:
                self.set_order_text(f, heap)

    def set_order_text(self, field, heap):
        """Mark one key of the order set now as text over the heap column `heap` (vdl_plan_set_order_text); None clears the mark."""
        enc = lambda t: t.encode() if isinstance(t, str) else t       # noqa: E731
        self._e._check(self._e._L.vdl_plan_set_order_text(self._h, enc(field), None if heap is None else enc(heap)))

    def order_note(self):
        """What the order step of the last run did ("host ...", "topn ...", "sort ..."); "" when no order is set."""
        return (self._e._L.vdl_plan_order_note(self._h) or b"").decode()

    def _collect(self, as_numpy=False):
        L = self._e._L
        results = {}
        for k in range(L.vdl_n_outputs(self._h)):
            name, tmp = ctypes.c_char_p(), ctypes.c_char_p()
            vals, n = ctypes.POINTER(ctypes.c_int64)(), ctypes.c_size_t()
            L.vdl_output(self._h, k, ctypes.byref(name), ctypes.byref(tmp), ctypes.byref(vals), ctypes.byref(n))
            high = ctypes.POINTER(ctypes.c_int64)()
            L.vdl_output_high(self._h, k, ctypes.byref(high), None)
            if high and vals and n.value:
                # wide sums: the exact values as Python ints, (hi << 64) | lo with lo taken unsigned; as_numpy: an object array of them
                lo = np.ctypeslib.as_array(vals, shape=(n.value,)).tolist()
                hi = np.ctypeslib.as_array(high, shape=(n.value,)).tolist()
                arr = [(h << 64) | (x & 0xFFFFFFFFFFFFFFFF) for x, h in zip(lo, hi)]
                if as_numpy:
                    arr = np.array(arr, dtype=object)
            elif n.value and not vals:
                dev = ctypes.POINTER(ctypes.c_int64)()
                L.vdl_output_device(self._h, k, ctypes.byref(dev), ctypes.byref(n))
                arr = DeviceValues(ctypes.cast(dev, ctypes.c_void_p).value, n.value, self)
            elif as_numpy:
                arr = np.ctypeslib.as_array(vals, shape=(n.value,)).copy() if n.value else np.zeros(0, np.int64)
            else:
                arr = np.ctypeslib.as_array(vals, shape=(n.value,)).tolist() if n.value else []
            results[tmp.value.decode()] = {"." + name.value.decode(): arr}
        timings = {}
        for k in range(L.vdl_n_timings(self._h)):
            label, us = ctypes.c_char_p(), ctypes.c_double()
            L.vdl_timing(self._h, k, ctypes.byref(label), ctypes.byref(us))
            timings[label.value.decode()] = int(round(us.value))
        return {"results": results, "timings": timings}

    def batch_note(self):
        """What the last Engine.run_batch / Engine.batch_jit_check did with this plan: "batch <b>: slot <q> of <K>, <kernel>" or
        "alone: <reason>"; "" after a plain run() (vdl.h: vdl_plan_batch_note)."""
        return (self._e._L.vdl_plan_batch_note(self._h) or b"").decode()

    def batch_sharded_note(self):
        """What the last Engine.run_batch_sharded / batch_sharded_layout did with this plan: "collective <c>: words [<off>,<off+h>) of
        <B>" or "own: <route> route" (vdl.h: vdl_plan_batch_sharded_note)."""
        return (self._e._L.vdl_plan_batch_sharded_note(self._h) or b"").decode()

    def batch_code_bytes(self):
        """The code size of the batch kernel that served this plan in the last Engine.run_batch / batch_jit_check; 0 when it ran alone."""
        return int(self._e._L.vdl_plan_batch_code_bytes(self._h))

    def execute(self):
        """vdl_run only: the outputs stay in the plan (borrowed until the next run); `collect()` converts them."""
        self._e._check(self._e._L.vdl_run(self._e._c, self._h))

    def collect(self, as_numpy=False):
        return self._collect(as_numpy)

    def run(self, as_numpy=False):
        """Execute on the GPU; returns {"results": {tmpN: {".name": [ints]}}, "timings": {...}} (the reply shape of
        /root/reference/resolve.py:8-32).  as_numpy=True keeps the value lists as int64 arrays: converting millions
        of result rows to Python ints costs far more than computing them."""
        self._e._check(self._e._L.vdl_run(self._e._c, self._h))
        return self._collect(as_numpy)

    # ---- sharded execution (one process per GPU) ----
    def partial_spec(self):
        n, ops = ctypes.c_int64(), ctypes.POINTER(ctypes.c_int32)()
        self._e._check(self._e._L.vdl_plan_partial_spec(self._h, ctypes.byref(n), ctypes.byref(ops)))
        return n.value, [int(ops[i]) for i in range(n.value)]

    def run_local(self, dev_ptr):
        self._e._check(self._e._L.vdl_run_local(self._e._c, self._h, ctypes.c_void_p(dev_ptr)))

    def finalize(self, dev_ptr):
        self._e._check(self._e._L.vdl_finalize(self._e._c, self._h, ctypes.c_void_p(dev_ptr)))
        return self._collect()

    def set_sharded_table(self, table):
        """Placement for plans that do not fuse: `table` is split by rows over the ranks, the others are replicated
        (then partial_spec / run_local / finalize also serve general plans whose outputs hang off global folds)."""
        self._e._check(self._e._L.vdl_plan_set_sharded_table(self._h, table.encode() if table else None))

    def set_row_offset(self, row0):
        self._e._check(self._e._L.vdl_plan_set_row_offset(self._h, int(row0)))

    def resolve_first(self, dev_ptr):
        self._e._check(self._e._L.vdl_resolve_first(self._e._c, self._h, ctypes.c_void_p(dev_ptr)))

    # ---- sharded Partition exchange (joins / sparse GROUP BY) ----
    def exchange_columns(self, sharded_table=None):
        n = ctypes.c_int()
        tbl = sharded_table.encode() if sharded_table else None
        self._e._check(self._e._L.vdl_exchange_spec(self._h, tbl, ctypes.byref(n)))
        return n.value

    def exchange_begin(self, world):
        counts = (ctypes.c_int64 * world)()
        self._e._check(self._e._L.vdl_exchange_begin(self._e._c, self._h, world, counts))
        return list(counts)

    def exchange_pack(self, dev_ptr):
        self._e._check(self._e._L.vdl_exchange_pack(self._e._c, self._h, ctypes.c_void_p(dev_ptr)))

    def exchange_finish(self, dev_ptr, n_recv, as_numpy=False):
        self._e._check(self._e._L.vdl_exchange_finish(self._e._c, self._h, ctypes.c_void_p(dev_ptr or 0), int(n_recv)))
        return self._collect(as_numpy)

    # ---- multi-GPU behind the C ABI (Engine.comm_init_*): the collectives happen inside libvdl ----
    def run_sharded(self, as_numpy=False):
        """Local phase over this rank's rows, collectives, finalisation (vdl_run_sharded).  Fold plans: every rank gets the
        full result; plans with a Partition: this rank's slice (the ranks' slices concatenate in rank order) -- or, with
        set_order(.., sharded=True), the same ordered and cut rows on every rank."""
        self._e._check(self._e._L.vdl_run_sharded(self._e._c, self._h))
        return self._collect(as_numpy)

    def sharded_route(self):
        """("fold" | "set" | "exchange", every rank ends with the whole answer?) -- vdl_plan_sharded_route; raises when the plan
        has no sharded route under the placement named with set_sharded_table."""
        name, whole = ctypes.c_char_p(), ctypes.c_int()
        self._e._check(self._e._L.vdl_plan_sharded_route(self._e._c, self._h, ctypes.byref(name), ctypes.byref(whole)))
        return name.value.decode(), bool(whole.value)

    def execute_sharded(self):
        """vdl_run_sharded only: the outputs stay in the plan (`collect()` converts them)."""
        self._e._check(self._e._L.vdl_run_sharded(self._e._c, self._h))

    def run_sharded_begin(self, slot):
        self._e._check(self._e._L.vdl_run_sharded_begin(self._e._c, self._h, int(slot)))

    def run_sharded_end(self, slot):
        self._e._check(self._e._L.vdl_run_sharded_end(self._e._c, self._h, int(slot)))
        return self._collect()

    def finalize_begin(self, dev_ptr, slot):
        self._e._check(self._e._L.vdl_finalize_begin(self._e._c, self._h, ctypes.c_void_p(dev_ptr), int(slot)))

    def finalize_end(self, slot):
        self._e._check(self._e._L.vdl_finalize_end(self._e._c, self._h, int(slot)))
        return self._collect()

    def scan_stats(self):
        rows, nbytes, us = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        self._e._check(self._e._L.vdl_plan_scan_stats(self._h, ctypes.byref(rows), ctypes.byref(nbytes), ctypes.byref(us)))
        return rows.value, nbytes.value, us.value

    def scan_traffic(self):
        """(HBM bytes one launch of the dominant fused scan moves, per-column detail): vdl_plan_scan_traffic -- measurement,
        call after a run and outside timed regions (a staged scan's late columns are counted by a census launch)."""
        b, detail = ctypes.c_int64(), ctypes.c_char_p()
        self._e._check(self._e._L.vdl_plan_scan_traffic(self._e._c, self._h, ctypes.byref(b), ctypes.byref(detail)))
        return b.value, (detail.value or b"").decode()


def order_host(keys, descending, limit=0):
    """vdl_order_host: the positions of the first `limit` (0 = all) rows under the engine's order -- `keys` a list of equally
    long int64 arrays compared key by key, `descending` one flag each, ties by position -- as an int64 array.  Needs no GPU."""
    L = _lib.load()
    cols = [np.ascontiguousarray(k, dtype=np.int64) for k in keys]
    if len(cols) != len(list(descending)):
        raise ValueError("one direction per key")
    m = len(cols[0]) if cols else 0
    if any(len(c) != m for c in cols):
        raise ValueError("keys of different lengths")
    if not cols and limit > 0:
        raise ValueError("no keys: the number of rows is unknown")
    n = len(cols)
    ptrs = (ctypes.POINTER(ctypes.c_int64) * max(n, 1))(*[c.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) for c in cols])
    desc = (ctypes.c_int * max(n, 1))(*[int(bool(d)) for d in descending])
    out = np.empty(min(limit, m) if limit > 0 else m, np.int64)
    rc = L.vdl_order_host(n, ptrs, desc, m, int(limit), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    if rc != _lib.VDL_OK:
        raise VdlError(rc, "vdl_order_host: bad argument")
    return out


def order_merge_host(counts, words, limit=0):
    """vdl_order_merge_host: the merge of a sharded run's ordered candidates, device-free.  `counts[r]` candidates of rank r, one
    run after the other; `words` a list of K uint64 arrays over all N = sum(counts) candidates (order words u = key ^ flip), each
    run ascending under them with ties in its own order.  Returns (run, index) int64 arrays of the first min(limit or N, N) rows
    of the order (u_1, .., u_K, run, index)."""
    L = _lib.load()
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    n = int(cnt.sum())
    cols = [np.ascontiguousarray(w, dtype=np.uint64) for w in words]
    if any(len(c) != n for c in cols):
        raise ValueError("every word column holds sum(counts) values")
    w = np.ascontiguousarray(np.concatenate(cols)) if cols else np.zeros(0, np.uint64)
    keep = min(limit, n) if limit > 0 else n
    run, idx, got = np.empty(keep, np.int64), np.empty(keep, np.int64), ctypes.c_int64()
    p64 = ctypes.POINTER(ctypes.c_int64)
    rc = L.vdl_order_merge_host(len(cnt), len(cols), cnt.ctypes.data_as(p64), w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(limit),
                                run.ctypes.data_as(p64), idx.ctypes.data_as(p64), ctypes.byref(got))
    if rc != _lib.VDL_OK or got.value != keep:
        raise VdlError(rc, "vdl_order_merge_host: bad argument")
    return run, idx


def comm_merge_host_wide(world, ops, gathered, stride_words=0):
    """vdl_comm_merge_host_wide: the merge of a sharded wide run's gathered blocks, device-free.  `gathered` holds `world` blocks
    of `stride_words` int64 (0 = 3 * len(ops) + 1): the raw words, the words with FIRST entries resolved, the rank's status, the
    high words of the raw words.  Returns (lo, hi, (status, rank)) -- int64 arrays of len(ops) values each; rank -1 = no rank
    failed."""
    L = _lib.load()
    n = len(ops)
    g = np.ascontiguousarray(gathered, dtype=np.int64)
    stride = int(stride_words) or 3 * n + 1
    if len(g) < world * stride:
        raise ValueError("gathered holds fewer than world * stride_words values")
    c_ops = (ctypes.c_int32 * max(n, 1))(*[int(o) for o in ops])
    lo, hi, status = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(2, np.int64)
    p64 = ctypes.POINTER(ctypes.c_int64)
    rc = L.vdl_comm_merge_host_wide(int(world), n, c_ops, g.ctypes.data_as(p64), int(stride_words), lo.ctypes.data_as(p64), hi.ctypes.data_as(p64),
                                    status.ctypes.data_as(p64))
    if rc != _lib.VDL_OK:
        raise VdlError(rc, "vdl_comm_merge_host_wide: bad argument")
    return lo, hi, (int(status[0]), int(status[1]))


def comm_merge_host_batch(world, n_words, offsets, ops, gathered, block_words):
    """vdl_comm_merge_host_batch: the merge of a sharded batch's gathered blocks, device-free.  Plan q has n_words[q] words, its
    operators ops[q] (a list per plan) and its segment at offsets[q] of every rank's block of `block_words` int64: the raw words, the
    words with FIRST entries resolved (only where the plan has a FIRST word), the rank's status.  Returns ([merged words per plan],
    [(status, rank) per plan]) -- rank -1 = no rank failed."""
    L = _lib.load()
    n = len(n_words)
    if len(offsets) != n or len(ops) != n or any(len(o) != w for o, w in zip(ops, n_words)):
        raise ValueError("one offset and one operator list of n_words[q] entries per plan")
    g = np.ascontiguousarray(gathered, dtype=np.int64)
    if len(g) < world * int(block_words):
        raise ValueError("gathered holds fewer than world * block_words values")
    flat = [int(o) for per in ops for o in per]
    c_ops = (ctypes.c_int32 * max(len(flat), 1))(*flat)
    nw = np.ascontiguousarray(n_words, dtype=np.int64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    out, status = np.zeros(max(len(flat), 1), np.int64), np.zeros(2 * max(n, 1), np.int64)
    p64 = ctypes.POINTER(ctypes.c_int64)
    rc = L.vdl_comm_merge_host_batch(int(world), n, nw.ctypes.data_as(p64), off.ctypes.data_as(p64), c_ops, g.ctypes.data_as(p64), int(block_words),
                                     out.ctypes.data_as(p64), status.ctypes.data_as(p64))
    if rc != _lib.VDL_OK:
        raise VdlError(rc, "vdl_comm_merge_host_batch: bad argument")
    cuts = np.cumsum([0] + [int(w) for w in n_words])
    return [out[cuts[q]:cuts[q + 1]].copy() for q in range(n)], [(int(status[2 * q]), int(status[2 * q + 1])) for q in range(n)]


def collate_host(heap, codes):
    """vdl_collate_host: (ranks, n_bad, first_bad) -- for every code the dense rank of the string that starts at that offset of
    `heap` (bytes or an int8 / uint8 array) in text order: unsigned bytes, a prefix before its extensions, equal strings share a
    rank, 0 = the empty string (a NUL byte), -1 = the code names no string of the heap (first_bad = the first such row, -1 =
    none).  The definition the device's collation index is checked against.  Needs no GPU."""
    L = _lib.load()
    h = np.frombuffer(bytes(heap), dtype=np.int8) if isinstance(heap, (bytes, bytearray)) else np.ascontiguousarray(heap).view(np.int8)
    c = np.ascontiguousarray(codes, dtype=np.int64)
    out = np.empty(len(c), np.int64)
    bad, first = ctypes.c_int64(), ctypes.c_int64()
    p64 = ctypes.POINTER(ctypes.c_int64)
    rc = L.vdl_collate_host(h.ctypes.data_as(ctypes.c_void_p) if len(h) else None, len(h), c.ctypes.data_as(p64), len(c), out.ctypes.data_as(p64),
                            ctypes.byref(bad), ctypes.byref(first))
    if rc != _lib.VDL_OK:
        raise VdlError(rc, "vdl_collate_host: bad argument")
    return out, bad.value, first.value


class Engine:
    """One context = one GPU (``device=None``: host-only, can parse/describe but not run)."""

    def __init__(self, device=0):
        self._L = _lib.load()
        c = ctypes.c_void_p()
        rc = self._L.vdl_open(ctypes.byref(c), -1 if device is None else int(device))
        self._c = c
        self._keep = {}
        self._plans = weakref.WeakSet()
        if rc:
            msg = self._L.vdl_last_error(c).decode()
            self._L.vdl_close(c)
            self._c = None
            raise VdlError(rc, msg)

    def close(self):
        if self._c:
            for p in list(self._plans):     # plans hold device events / pinned buffers of this context
                p.close()
            self._L.vdl_close(self._c)
            self._c = None
            self._keep.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise VdlError(rc, self._L.vdl_last_error(self._c).decode())

    def version(self):
        return self._L.vdl_version().decode()

    def set_stream(self, hip_stream_handle):
        """Launch on this HIP stream handle (0 = the legacy default stream torch uses by default)."""
        self._check(self._L.vdl_set_stream(self._c, ctypes.c_void_p(hip_stream_handle or 0)))

    def use_torch_stream(self):
        """Launch on torch's current stream, so torch ops / collectives order against the engine."""
        import torch

        self.set_stream(torch.cuda.current_stream().cuda_stream)

    def use_own_stream(self):
        self._check(self._L.vdl_use_own_stream(self._c))

    # ---- communicator (one process per GPU; see include/vdl.h "multi-GPU behind this boundary") ----
    def comm_unique_id(self):
        """128 bytes made by ONE rank (ncclGetUniqueId); hand them to the other ranks over any channel."""
        buf = ctypes.create_string_buffer(_lib.COMM_ID_BYTES)
        self._check(self._L.vdl_comm_unique_id(buf))
        return buf.raw

    def comm_init_rccl(self, rank, world, unique_id):
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise VdlError(_lib.VDL_ERR_ARG, "the communicator id is %d bytes" % _lib.COMM_ID_BYTES)
        self._check(self._L.vdl_comm_init(self._c, int(rank), int(world), ctypes.c_char_p(unique_id)))

    def comm_init_host(self, rank, world, all_gather, all_to_all):
        """Collectives supplied by the caller over host memory:
        all_gather(send: bytes) -> list of `world` bytes objects (rank order);
        all_to_all(pieces: list of `world` bytes objects, one per destination) -> list of `world` bytes objects, one per source."""
        def c_all_gather(_user, send, recv, nbytes):
            try:
                parts = all_gather(ctypes.string_at(send, nbytes))
                for r, part in enumerate(parts):
                    if len(part) != nbytes:
                        return 1
                    ctypes.memmove(recv + r * nbytes, part, nbytes)
                return 0
            except Exception:              # noqa: BLE001 -- must not propagate through the C frame
                import traceback
                traceback.print_exc()
                return 1

        def c_all_to_all(_user, send, send_bytes, recv, recv_bytes):
            try:
                pieces, at = [], 0
                for r in range(world):
                    pieces.append(ctypes.string_at(send + at, send_bytes[r]) if send_bytes[r] else b"")
                    at += send_bytes[r]
                got = all_to_all(pieces)
                at = 0
                for r in range(world):
                    if len(got[r]) != recv_bytes[r]:
                        return 1
                    if recv_bytes[r]:
                        ctypes.memmove(recv + at, got[r], recv_bytes[r])
                    at += recv_bytes[r]
                return 0
            except Exception:              # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        self._comm_host = _lib.CommHost(None, _lib.ALL_GATHER_FN(c_all_gather), _lib.ALL_TO_ALL_FN(c_all_to_all))     # kept alive with the engine
        self._check(self._L.vdl_comm_init_host(self._c, int(rank), int(world), ctypes.byref(self._comm_host)))

    def comm_info(self):
        rank, world, name = ctypes.c_int(), ctypes.c_int(), ctypes.c_char_p()
        self._check(self._L.vdl_comm_info(self._c, ctypes.byref(rank), ctypes.byref(world), ctypes.byref(name)))
        return rank.value, world.value, name.value.decode()

    # ---- catalog ----
    def register_tensor(self, name, tensor):
        """Borrow a 1-D integer torch tensor that already lives in HBM."""
        if not tensor.is_cuda or tensor.dim() != 1 or not tensor.is_contiguous():
            raise VdlError(_lib.VDL_ERR_ARG, "register_tensor needs a contiguous 1-D device tensor")
        self._keep[name] = tensor
        self._check(self._L.vdl_register_column(self._c, name.encode(), ctypes.c_void_p(tensor.data_ptr()),
                                                tensor.element_size(), tensor.numel()))

    def register_pointer(self, name, dev_ptr, elem_bytes, nrows):
        """Borrow nrows integers of elem_bytes each at a device address the caller keeps alive (vdl_register_column)."""
        self._check(self._L.vdl_register_column(self._c, name.encode(), ctypes.c_void_p(dev_ptr), elem_bytes, nrows))

    def upload(self, name, array):
        a = np.ascontiguousarray(array)
        if a.dtype.kind != "i":
            raise VdlError(_lib.VDL_ERR_ARG, "columns are signed integers")
        self._check(self._L.vdl_upload_column(self._c, name.encode(), a.ctypes.data_as(ctypes.c_void_p),
                                              a.dtype.itemsize, a.shape[0]))

    def generate(self, spec, row0, nrows, seed=datagen.SEED):
        """Materialise rows [row0, row0+nrows) of a synthetic column directly in HBM."""
        self._check(self._L.vdl_generate_column(self._c, spec.name.encode(), np.dtype(spec.dtype).itemsize, row0, nrows,
                                                seed, spec.lo, spec.hi, spec.mul, spec.add))

    def download(self, name):
        w, n = ctypes.c_int(), ctypes.c_int64()
        self._check(self._L.vdl_column_info(self._c, name.encode(), ctypes.byref(w), ctypes.byref(n), None))
        out = np.empty(n.value, dtype={1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[w.value])
        self._check(self._L.vdl_download_column(self._c, name.encode(), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return out

    def column_device(self, name):
        """A registered / generated column as it lies in HBM: `DeviceValues`-like object with `__cuda_array_interface__`
        (`torch.as_tensor(x, device=...)` wraps it without a copy; checkers use it to read the very bytes the engine scans)."""
        w, n, ptr = ctypes.c_int(), ctypes.c_int64(), ctypes.c_void_p()
        self._check(self._L.vdl_column_info(self._c, name.encode(), ctypes.byref(w), ctypes.byref(n), ctypes.byref(ptr)))

        class _Column:
            __cuda_array_interface__ = {"shape": (n.value,), "typestr": "<i%d" % w.value, "data": (ptr.value or 0, False), "version": 3, "strides": None}
            owner = self
        return _Column()

    def encode(self, name):
        """Build the frame-of-reference image of a catalog column (vdl_encode_column; generated columns have one already).
        For a borrowed column the caller promises not to write it afterwards."""
        self._check(self._L.vdl_encode_column(self._c, name.encode()))

    def image_info(self, name):
        """(width, base, scale) of a column's image: v = base + scale * e; width 0 = no image"""
        w, b, s = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.vdl_column_image_info(self._c, name.encode(), ctypes.byref(w), ctypes.byref(b), ctypes.byref(s)))
        return w.value, b.value, s.value

    def packed_info(self, name):
        """(bits, base, scale) of a column's bit-packed image: v = base + scale * e'; bits 0 = none"""
        b, base, s = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.vdl_column_packed_info(self._c, name.encode(), ctypes.byref(b), ctypes.byref(base), ctypes.byref(s)))
        return b.value, base.value, s.value

    def download_packed(self, name):
        """the packed image's dwords (vdl_download_packed_image) as a uint32 array"""
        bits = self.packed_info(name)[0]
        n = ctypes.c_int64()
        self._check(self._L.vdl_column_info(self._c, name.encode(), None, ctypes.byref(n), None))
        out = np.empty((n.value + 2047) // 2048 * bits * 64, dtype=np.uint32)
        self._check(self._L.vdl_download_packed_image(self._c, name.encode(), out.ctypes.data_as(ctypes.c_void_p), out.nbytes))
        return out

    def declare_packed(self, name, bits, base=0, scale=1):
        """a context without a device: the column has a packed image of `bits` bits (jit_check builds the packed form over it)"""
        self._check(self._L.vdl_declare_packed_image(self._c, name.encode(), int(bits), int(base), int(scale)))

    def declare_image(self, name, width, base=0, scale=1):
        """a context without a device: the column has a byte image of `width` bytes, v = base + scale * e (jit_check builds the scans
        and lookups that read it)"""
        self._check(self._L.vdl_declare_column_image(self._c, name.encode(), int(width), int(base), int(scale)))

    def set_lookup_images(self, enabled):
        """True: lookups through a join index read the byte image of their target column where its use allows (vdl.h:
        vdl_set_lookup_images; off by default, VDL_LOOKUP_IMAGES=1 switches it on when the context opens; ignored while
        set_column_images(False)).  Bound plans re-bind at their next run."""
        self._check(self._L.vdl_set_lookup_images(self._c, 1 if enabled else 0))

    def set_column_images(self, enabled):
        """False: scans read the catalog columns and ignore their images (tests, A/B runs in one process)"""
        self._check(self._L.vdl_set_column_images(self._c, 1 if enabled else 0))

    def encode_steps(self, name):
        """Try to build the step image of a catalog column (vdl_encode_steps): a column that never decreases and steps by at most
        1 gets one, any other column none.  For a borrowed column the caller promises not to write it afterwards."""
        self._check(self._L.vdl_encode_steps(self._c, name.encode()))

    def steps_info(self, name):
        """(present, base, groups) of a column's step image; (False, 0, 0) = none"""
        p, b, g = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.vdl_column_steps_info(self._c, name.encode(), ctypes.byref(p), ctypes.byref(b), ctypes.byref(g)))
        return bool(p.value), b.value, g.value

    def download_steps(self, name):
        """the step image (vdl_download_steps_image): (heads as uint64, anchors as uint32), one entry per 64 rows"""
        groups = self.steps_info(name)[2]
        heads, anchors = np.empty(groups, dtype=np.uint64), np.empty(groups, dtype=np.uint32)
        self._check(self._L.vdl_download_steps_image(self._c, name.encode(), heads.ctypes.data_as(ctypes.c_void_p),
                                                     anchors.ctypes.data_as(ctypes.c_void_p), groups))
        return heads, anchors

    def declare_steps(self, name, base=0):
        """a context without a device: the column has a step image (jit_check builds the scans that decode it)"""
        self._check(self._L.vdl_declare_steps_image(self._c, name.encode(), int(base)))

    def set_step_images(self, enabled):
        """False: scans leave the step images unbound (A/B runs in one process)"""
        self._check(self._L.vdl_set_step_images(self._c, 1 if enabled else 0))

    def build_collation(self, heap):
        """Build the collation index of a heap column now (vdl_build_collation) instead of at the first run that orders by its
        text; nothing happens when the column has one."""
        self._check(self._L.vdl_build_collation(self._c, heap.encode()))

    def collate(self, heap, codes):
        """(ranks, n_bad, first_bad) like `collate_host`, through the device's collation index of the heap column `heap`
        (vdl_collate_device; the index is built if the column has none)."""
        c = np.ascontiguousarray(codes, dtype=np.int64)
        out = np.empty(len(c), np.int64)
        bad, first = ctypes.c_int64(), ctypes.c_int64()
        p64 = ctypes.POINTER(ctypes.c_int64)
        self._check(self._L.vdl_collate_device(self._c, heap.encode(), c.ctypes.data_as(p64), len(c), out.ctypes.data_as(p64), ctypes.byref(bad),
                                               ctypes.byref(first)))
        return out, bad.value, first.value

    def collation_info(self, heap):
        """(present, strings, distinct, max_bytes) of a heap column's collation index; (False, 0, 0, 0) = none"""
        p, n, d, b = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        self._check(self._L.vdl_collation_info(self._c, heap.encode(), ctypes.byref(p), ctypes.byref(n), ctypes.byref(d), ctypes.byref(b)))
        return bool(p.value), n.value, d.value, b.value

    def drop(self, name):
        self._keep.pop(name, None)
        self._check(self._L.vdl_drop_column(self._c, name.encode()))

    # ---- programs ----
    def parse(self, vdl_text):
        data = vdl_text.encode() if isinstance(vdl_text, str) else vdl_text
        h = ctypes.c_void_p()
        rc = self._L.vdl_parse(self._c, data, len(data), ctypes.byref(h))
        self._check(rc)
        plan = Plan(self, h, vdl_text)
        self._plans.add(plan)
        return plan

    def _handles(self, plans):
        plans = list(plans)
        return plans, (ctypes.c_void_p * max(len(plans), 1))(*[p._h if p is not None else None for p in plans])

    def run_batch(self, plans, as_numpy=False):
        """Run the plans in one call (vdl.h: vdl_run_batch): those that differ in their literals alone share one pass over the
        columns, the others run alone; the list of the dicts `Plan.run()` returns, in the plans' order.  `Plan.batch_note()` says
        what became of each."""
        plans, arr = self._handles(plans)
        self._check(self._L.vdl_run_batch(self._c, arr, len(plans)))
        return [p._collect(as_numpy) for p in plans]

    def run_batch_sharded(self, plans, as_numpy=False):
        """Run the plans in ONE sharded call (vdl.h: vdl_run_batch_sharded): the plans that fuse as a whole on the fold route share
        one all-gather and one merge, the others run through run_sharded afterwards; the list of the dicts `Plan.run_sharded()`
        returns, in the plans' order.  `Plan.batch_sharded_note()` and `Plan.batch_note()` say what became of each."""
        plans, arr = self._handles(plans)
        self._check(self._L.vdl_run_batch_sharded(self._c, arr, len(plans)))
        return [p._collect(as_numpy) for p in plans]

    def batch_sharded_layout(self, plans):
        """([offset per plan, -1 = an own plan], [height per plan], block words) of the rank block run_batch_sharded would gather
        (vdl_batch_sharded_layout; needs neither a device nor a communicator)."""
        plans, arr = self._handles(plans)
        n = len(plans)
        off, h, b = (ctypes.c_int64 * max(n, 1))(), (ctypes.c_int64 * max(n, 1))(), ctypes.c_int64()
        self._check(self._L.vdl_batch_sharded_layout(self._c, arr, n, off, h, ctypes.byref(b)))
        return list(off)[:n], list(h)[:n], b.value

    def set_batch_grouped(self, on):
        """True: run_batch also batches plans whose one scan is a GROUP BY over table columns (vdl.h: vdl_set_batch_grouped; off by
        default, VDL_BATCH_GROUPED=1 switches it on when the context opens)."""
        self._check(self._L.vdl_set_batch_grouped(self._c, 1 if on else 0))

    def set_batch_joins(self, on):
        """True: run_batch also batches plans whose one scan has derived columns and a prelude -- join scans such as TPC-H Q14, Q12, Q19
        and Q4 -- when they build the same lookup tables and hold the same literals in their conditions (vdl.h: vdl_set_batch_joins; off
        by default, VDL_BATCH_JOINS=1 switches it on when the context opens)."""
        self._check(self._L.vdl_set_batch_joins(self._c, 1 if on else 0))

    def batch_jit_check(self, plans):
        """Group the plans and build the batch kernels against the registered columns without a device (vdl_batch_jit_check); the notes."""
        plans, arr = self._handles(plans)
        self._check(self._L.vdl_batch_jit_check(self._c, arr, len(plans)))
        return [p.batch_note() for p in plans]

    def run_vdl(self, vdl_text, fuse=True):
        plan = self.parse(vdl_text)
        try:
            plan.set_fusion(fuse)
            return plan.run()
        finally:
            plan.close()
