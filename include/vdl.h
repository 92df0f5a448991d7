/*
 * vdl.h -- C ABI of libvdl, the MI355X-native execution engine for the textual VDL
 * (Voodoo vector-operator dataflow) printed by orm011/mplan2vdl.
 *
 * What this boundary replaces.  The reference has no in-process executor: its VDL text
 * leaves the process on stdout (/root/reference/src/MainFuns.hs:157) and is POSTed to
 * an external Voodoo server, whose JSON reply is decoded by resolve.py
 * (/root/reference/eval_query.sh:18-26, /root/reference/resolve.py:8-32).  libvdl is
 * that server's `/voodoo/.../run` hop as a library:
 *
 *     request  body  = VDL text (grammar: /root/reference/src/Vdl.hs:410-477;
 *                      " ;; metadata" suffixes as stripped by eval_query.sh:20 are ignored)
 *     response body  = {"results": {"tmpN": {".<name>": [ints]}}, "timings": {label: usec}}
 *                      -> vdl_output() / vdl_timing() below, one entry per MaterializeCompact.
 *
 * A Haskell host binds these with `foreign import ccall` (stub in INTEGRATION.md); the
 * CLI `vdlrun` and the Python package `mplan2vdl_amd` are the callers exercised here.
 *
 * Conventions: plain C types only, no callbacks (except the optional host transport of vdl_comm_init_host); every call returns VDL_OK (0) or a
 * VDL_ERR_* code and leaves a message for vdl_last_error(); pointers returned by
 * vdl_output()/vdl_timing()/vdl_plan_describe() are borrowed and stay valid until the
 * plan is run again or freed.  One context per process and GPU; calls on one context
 * are not re-entrant (the reference's model is one query per request, no shared state).
 * There is NO CPU fallback: every run call needs a HIP device and fails with
 * VDL_ERR_DEVICE without one.
 */
#ifndef VDL_H
#define VDL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vdl_ctx  vdl_ctx;   /* device, stream, column catalog, memory pool   */
typedef struct vdl_plan vdl_plan;  /* parsed program + fused execution plan + results */

enum {
    VDL_OK              = 0,
    VDL_ERR_PARSE       = 1,  /* malformed VDL text (line number in vdl_last_error)          */
    VDL_ERR_COLUMN      = 2,  /* Load of a column that is not in the catalog                  */
    VDL_ERR_UNSUPPORTED = 3,  /* operator / pattern outside the implemented set               */
    VDL_ERR_DEVICE      = 4,  /* no HIP device, or a HIP call failed                          */
    VDL_ERR_ARG         = 5,  /* bad argument                                                 */
    VDL_ERR_SHAPE       = 6,  /* operand lengths / field names do not fit                     */
    VDL_ERR_NOMEM       = 7,
    VDL_ERR_OVERFLOW    = 8   /* checked sums (vdl_plan_set_wide_sums 2): a result does not fit int64 */
};

/* partial-state merge operators for sharded execution */
enum {
    VDL_REDUCE_NONE = 0, VDL_REDUCE_SUM = 1, VDL_REDUCE_MIN = 2, VDL_REDUCE_MAX = 3,
    /* FoldChoose of a grouped plan: the word holds the group's smallest GLOBAL row id after the local
     * phase.  Merge = all-reduce MIN, then vdl_resolve_first() (the rank owning that row substitutes the
     * column value, every other rank 0), then all-reduce SUM of the same words. */
    VDL_REDUCE_FIRST = 4
};

/* ---- context ------------------------------------------------------------------ */

/* device >= 0 binds that HIP device and creates the engine stream; device < 0 makes a
 * host-only context that can parse, plan and describe but not run (used by CPU tests). */
int  vdl_open(vdl_ctx **out, int device);
void vdl_close(vdl_ctx *ctx);
const char *vdl_last_error(const vdl_ctx *ctx);
const char *vdl_version(void);

/* Run on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream).  The handle is
 * used as given: 0 / NULL means the legacy default stream (what torch uses unless told otherwise),
 * so that collectives and tensor ops issued by the caller order against the engine's kernels.
 * vdl_use_own_stream() goes back to the engine's private non-blocking stream.  Both drain the stream being left
 * first (the engine's buffers are protected by stream order), so switch streams between queries, not inside one. */
int  vdl_set_stream(vdl_ctx *ctx, void *hip_stream);
int  vdl_use_own_stream(vdl_ctx *ctx);

/* ---- column catalog ("Load table.col", /root/reference/src/Vdl.hs:161-168,419-420) --
 * Columns are contiguous little-endian signed integers of elem_bytes in {1,2,4,8}
 * (storage widths /root/reference/tests/tpch10noorder/storage.csv:188-208), resident in
 * HBM.  `name` is the key path as printed after Load, e.g. "lineitem.l_shipdate". */
int  vdl_register_column(vdl_ctx *ctx, const char *name, const void *dev_ptr,
                         int elem_bytes, int64_t nrows);               /* borrowed device memory */
int  vdl_upload_column(vdl_ctx *ctx, const char *name, const void *host_ptr,
                       int elem_bytes, int64_t nrows);                 /* engine-owned copy, H2D   */
/* Synthetic column generated in place in HBM by the counter-based generator of
 * v(row) = add + mul*(lo + splitmix64(seed ^ fnv1a(name)*PHI ^ row) % (hi-lo+1)),
 * rows [row0, row0+nrows). */
int  vdl_generate_column(vdl_ctx *ctx, const char *name, int elem_bytes, int64_t row0,
                         int64_t nrows, uint64_t seed, int64_t lo, int64_t hi,
                         int64_t mul, int64_t add);
int  vdl_drop_column(vdl_ctx *ctx, const char *name);
int  vdl_column_info(const vdl_ctx *ctx, const char *name, int *elem_bytes, int64_t *nrows,
                     const void **dev_ptr);
/* Copy a catalog column back to the host (tests, debugging). */
int  vdl_download_column(vdl_ctx *ctx, const char *name, void *host_ptr, size_t bytes);

/* ---- column images ----------------------------------------------------------------
 * A column whose values span few significant digits is kept a second time, narrow: its frame-of-reference image,
 * v = base + scale * e with e in 1, 2 or 4 bytes (scale a power of ten all differences share).  Fused aggregate scans
 * read the image instead of the column where every use of the column in that scan allows it (range filters, formula
 * tests and aggregate factors are rewritten into the encoded domain; a pure narrowing, base 0 and scale 1, may stand
 * in for any use), with the same results.  The catalog column itself stays as it is: vdl_column_info and
 * vdl_download_column see it, never the image.  vdl_generate_column builds the image; uploaded and registered
 * columns have none until vdl_encode_column is called (for a registered column the caller promises not to write
 * it afterwards: the image would go stale).  The image goes with its column (drop, re-registration).
 * No image is built when it would not be narrower than the column. */
int  vdl_encode_column(vdl_ctx *ctx, const char *name);
/* width 0: the column has no image; otherwise its width in bytes and v = base + scale * e */
int  vdl_column_image_info(const vdl_ctx *ctx, const char *name, int *width, int64_t *base, int64_t *scale);
/* The bit-packed image built beside a byte image: v = base + scale * e' with e' in `bits` bits (1..32) per row, in lane-transposed
 * stripes of 2048 rows (row 2048 s + 64 j + l is value j of lane l; lane l's values are a bit stream of `bits` dwords, dword k at
 * dword index (s * bits + k) * 64 + l; zero-padded to whole stripes).  bits 0: the column has none. */
int  vdl_column_packed_info(const vdl_ctx *ctx, const char *name, int *bits, int64_t *base, int64_t *scale);
/* its bytes: ceil(nrows / 2048) * bits * 256 */
int  vdl_download_packed_image(vdl_ctx *ctx, const char *name, void *host_ptr, size_t bytes);
/* contexts without a device (vdl_plan_jit_check): declare a registered column's packed image (no bytes behind it) */
int  vdl_declare_packed_image(vdl_ctx *ctx, const char *name, int bits, int64_t base, int64_t scale);
/* contexts without a device (vdl_plan_jit_check): declare a registered column's byte image (no bytes behind it): width 1, 2 or 4 and
 * narrower than the column, scale >= 1.  Scans and lookups bound on that context treat it like an image a device built. */
int  vdl_declare_column_image(vdl_ctx *ctx, const char *name, int width, int64_t base, int64_t scale);
/* on = 0: scans bind the catalog columns and ignore the images (tests, A/B comparisons in one process); default 1 */
int  vdl_set_column_images(vdl_ctx *ctx, int on);
/* Lookup images.  A dimension column looked up through a join index -- p_type at lineitem_part[row], o_orderdate at
 * lineitem_orders[row] -- is by default read from the catalog column at its stored width.  on = 1: where the target column has a byte
 * image and the use of the looked-up value allows it, every scan role reads the image at v[index] instead -- a quarter or an eighth of
 * the table for the caches to hold --, by the rules of the streamed columns: a value used only in a range filter, a formula test or
 * an aggregate factor stays encoded (bounds and factors rewritten); a value an aggregate scan needs as stored (the source of another
 * lookup, a group-key load, a FIRST column) takes a pure narrowing only; in fronts, dimension and semi-join scans a value needed per
 * row (the source of a further lookup or of a difference, a semi-join position) takes an image of scale 1 and is decoded after the
 * lookup; the take side of a front decodes whatever it looks up, at any scale.  An index outside the target's rows makes the row EPS
 * as before.  Results are bit-identical.  Off by default (VDL_LOOKUP_IMAGES=1 in the environment when the context opens switches it
 * on); ignored while vdl_set_column_images(ctx, 0).  Flipping it re-binds bound plans at their next run.  Kernels that read a
 * lookup image carry ",limg" in the names vdl_plan_jit_note and the timings list.  Bit-packed and step images are not read by lookups. */
int  vdl_set_lookup_images(vdl_ctx *ctx, int on);

/* ---- step images ------------------------------------------------------------------
 * A column that never decreases and whose consecutive rows differ by 0 or 1 -- the join index of a table clustered by its
 * parent, lineitem.lineitem_orders -- can be kept as its first value, one bit per row and one anchor per 64 rows.  With
 * G = ceil(nrows / 64) groups:
 *   heads[g]   uint64: bit i is 1 iff row r = 64 g + i has r >= 1 and v[r] != v[r - 1]
 *   anchors[g] uint32: v[64 g - 1] - base for g >= 1, anchors[0] = 0                  (base = v[0])
 *   v[r] = base + anchors[r >> 6] + popcount(heads[r >> 6] & (~0 >> (63 - (r & 63))))
 * 12 bytes per 64 rows.  The scans that look things up through such a column -- fused fronts, dimension scans, semi-join
 * scans -- read the step image in place of the column or its byte image and decode it as the tile comes in, always to the
 * column's own values: results are the same.  Fused aggregate scans do not read it.
 * Strictly opt-in: vdl_encode_steps builds the step image of a generated, uploaded or registered column (for a registered
 * column the caller promises not to write it afterwards), 1 <= nrows < 2^32 at any element width.  A column that does not
 * qualify gets none, and the call still returns VDL_OK.  The image goes with its column (drop, re-registration) and is
 * ignored while vdl_set_column_images(ctx, 0).  VDL_STEP_IMAGES=1 in the environment makes vdl_encode_column try a step
 * image as well. */
int  vdl_encode_steps(vdl_ctx *ctx, const char *name);
/* present 0: the column has no step image (base and groups are then 0); otherwise its base and G */
int  vdl_column_steps_info(const vdl_ctx *ctx, const char *name, int *present, int64_t *base, int64_t *groups);
/* the image's `groups` (= G) head words and anchors */
int  vdl_download_steps_image(vdl_ctx *ctx, const char *name, uint64_t *heads, uint32_t *anchors, int64_t groups);
/* contexts without a device (vdl_plan_jit_check): declare a registered column's step image (no bytes behind it) */
int  vdl_declare_steps_image(vdl_ctx *ctx, const char *name, int64_t base);
/* on = 0: scans leave the step images unbound and read what they read without them (A/B runs in one process); default 1 */
int  vdl_set_step_images(vdl_ctx *ctx, int on);

/* ---- plans --------------------------------------------------------------------- */

/* Parse the VDL text, check it, and build the execution plan (operator fusion included).
 * Needs no device.  Both output formats of the compiler are accepted: the default VDL lines
 * (/root/reference/src/Vdl.hs:410-453) and the --vliteformat lines (Vdl.hs:370-408,455-475; recognised by
 * their Output statements).
 * One point where a program's meaning is narrower than its text: Scatter(src, fold, pos) with the SAME position twice
 * leaves one of the two values there, which one is unspecified (the oracle keeps the later slot's, the kernels whichever
 * store lands last).  Every Scatter the compiler emits has unique positions -- Partition ranks, filtered row ids
 * (/root/reference/src/Vlite.hs:508,1058-1059,1267-1275) -- and the parity tests only build such programs. */
int  vdl_parse(vdl_ctx *ctx, const char *vdl_text, size_t len, vdl_plan **out);
void vdl_plan_free(vdl_plan *plan);

/* Human-readable plan: one line per execution step ("scan ...", "op 17 Greater ..."). */
const char *vdl_plan_describe(const vdl_plan *plan);
/* 1 if every output of the plan comes from fused scan kernels (no per-operator steps). */
int  vdl_plan_is_fused(const vdl_plan *plan);
/* Force per-operator execution (no fusion) for this plan: used by parity tests to check
 * every operator kernel against the oracle on programs that would otherwise fuse. */
int  vdl_plan_set_fusion(vdl_plan *plan, int enabled);

/* Run-time specialisation of a fused plan's multi-aggregate scans: the scan kernels' own device code compiled by hiprtc with
 * this plan's descriptor (column kinds, filters, group key, aggregate terms, conditions) as compile-time constants, at the
 * next run after it is switched on -- seconds, once per distinct scan per process (kept under $VDL_JIT_CACHE when that
 * names a directory).  Off by default (VDL_JIT=1 in the environment switches it on for every plan parsed afterwards).
 * enabled = 2 (VDL_JIT=2) also tunes: at the first run each specialised scan is built with 2, 3, 4 and 6 row pairs per
 * lane and the quickest of a few timed launches over the real columns stays (a few seconds more, once).  A scan
 * whose specialisation does not build runs on the precompiled kernels; vdl_plan_jit_note says which did and which did not.
 * vdl_plan_jit_check builds the specialised kernels against the columns registered now without loading or running them
 * (no GPU needed): VDL_OK, or VDL_ERR_UNSUPPORTED with the compiler's message in vdl_last_error.
 * (The reference hands its text to an engine that generates code per program: /root/reference/README.md:57.) */
int  vdl_plan_set_jit(vdl_plan *plan, int enabled);
/* Filter bounds of the specialised code at run time.  By default the specialised code holds every literal of the query, so Q6
 * for another year is another translation unit for every form the tuner tries and no cache ever hits.  at_run_time = 1: the
 * generated code holds the SHAPE of each range filter and formula test only -- no lower bound, no upper bound, both, or a point
 * (lo = hi: one equality compare); a bound at or beyond the end of the domain its column is read in counts as absent -- and
 * reads the values from the plan's descriptor in device memory by scalar loads.  Plans that differ in bound values alone then
 * share source, cache key and code object: the second one compiles nothing.  A change of shape or of structure (which columns
 * are read late, a filter that vanishes) compiles anew.  Everything else stays a constant of the code.  Off by default
 * (VDL_JIT_BOUNDS=runtime in the environment switches it on for every plan parsed afterwards); kernels built this way carry
 * ",rtb" in the names vdl_plan_jit_note lists.  Takes effect at the plan's next run or vdl_plan_jit_check. */
int  vdl_plan_set_jit_bounds(vdl_plan *plan, int at_run_time);
/* Builds of specialised code in this process so far: compiled by hiprtc, read from $VDL_JIT_CACHE, found in memory.  Any pointer
 * may be null.  (vdl_plan_jit_note also says, per scan of a plan that ran, how many of its builds came from a cache:
 * "from cache: 2 of 3 builds of scan 0; ".) */
void vdl_jit_counters(int64_t *compiled, int64_t *from_disk, int64_t *from_memory);
/* Prelude tables built in this process so far: LIKE tables, dimension bitmaps (by a scan or by their witness statements) and semi-join
 * sets, one count per table and run.  A join batch (vdl_set_batch_joins) builds its tables once, K plans run alone K times. */
void vdl_prelude_counters(int64_t *items);
const char *vdl_plan_jit_note(const vdl_plan *plan);
int  vdl_plan_jit_check(vdl_ctx *ctx, vdl_plan *plan);
/* Which catalog columns the plan's scans read from their images, as bound at its last run or vdl_plan_jit_check: one entry
 * per scan role that reads any -- "scan<k>" (fused aggregate scans), "front.select" / "front.take" (the two sides of a fused
 * front), "dim<k>" (dimension scans), "semi<k>" (semi-join scans) -- each listing "table.column:width", e.g.
 * "front.select: lineitem.l_shipdate:2 lineitem.lineitem_orders:4; dim3: orders.o_orderdate:2".  "" when none does.
 * The text stays valid until the next call for this plan. */
int  vdl_plan_image_columns(const vdl_plan *plan, const char **list);
/* Likewise the columns read from their step images, "table.column:s" per scan role, e.g.
 * "front.select: lineitem.lineitem_orders:s; front.take: lineitem.lineitem_orders:s".  A column listed here under a role is
 * not listed under that role by vdl_plan_image_columns.  Kernels that read a step image carry ",stp" in the names
 * vdl_plan_jit_note lists. */
int  vdl_plan_step_columns(const vdl_plan *plan, const char **list);
/* Likewise the TARGET columns the plan's lookups read from their images (vdl_set_lookup_images), "table.column:width" per scan role,
 * e.g. "front.take: orders.o_orderdate:2 orders.o_shippriority:1" or "scan0: part.p_type:2".  Lookup targets are never listed by
 * vdl_plan_image_columns, which speaks of the columns a scan streams.  "" when no lookup reads an image. */
int  vdl_plan_lookup_columns(const vdl_plan *plan, const char **list);

/* Execute: binds Loads to the catalog, runs all kernels, copies the MaterializeCompact
 * outputs to the host and synchronises. */
int  vdl_run(vdl_ctx *ctx, vdl_plan *plan);

/* ---- batched runs: plans that differ in their literals alone share one pass over the columns -----------------------------
 * The same query for eight years, a dashboard's slices of one table: each vdl_run re-reads the same columns.  vdl_run_batch runs
 * n plans in one call and ALWAYS produces every answer: after VDL_OK every plan holds what vdl_run of it alone would have left
 * -- the same outputs bit for bit through vdl_output, an order set on the plan applied as vdl_run applies it.  Plans that can share
 * a scan are grouped and each group is cut into batches of at most 8 plans -- fewer for scans of many aggregates: a lane keeps
 * slots x (1 + aggregates) <= 32 accumulators in registers --; one kernel reads every tile once and tests it against each plan's
 * bounds, with a count and accumulators per plan.  Every other plan runs alone through the vdl_run path inside the same call.
 * Two plans share a scan when both are fused with specialisation on (vdl_plan_set_jit >= 1), each is exactly one global aggregate scan
 * over table columns (no grouped scan, no derived columns, no lookup tables or semi-join sets) that is not known to be empty, they
 * bind the same columns (same images, row count, row offset), and their generated code under run-time bounds is the same (the shapes
 * of vdl_plan_set_jit_bounds; the batch always generates with the bounds at run time, whatever the plans' own setting).  The batch
 * kernel is a code object of its own per width (",batch<K>,rtb>" in its name), cached like any other and kept loaded with the context:
 * a second batch of the same width and shape with new literals compiles nothing.  Untuned plans get the eager form; when every plan
 * of a batch tunes (vdl_plan_set_jit 2) the eager form at 2, 3, 4 row pairs per lane and the every-column packed form at 2, 4 are
 * timed once per shape and width (VDL_JIT_PIN / VDL_JIT_U pin as they do for one plan); the forms that read late are not batched.
 * n < 1, a null entry or the same plan twice: VDL_ERR_ARG.  A plan's failure is reported as vdl_run would report it, the message
 * naming the plan's index; the plans after it may not have run.
 * vdl_plan_batch_note: what the last vdl_run_batch / vdl_batch_jit_check did with the plan -- "batch <b>: slot <q> of <K>, <kernel name>"
 * or "alone: <reason>" ("specialisation is off", "grouped scans are not batched", "its filter shapes differ from every other
 * plan's", ...); "" after a plain vdl_run.
 * vdl_batch_jit_check: like vdl_plan_jit_check, groups the plans and builds the batch kernels against the columns registered now
 * without a device, and fills the notes.
 * With vdl_plan_set_profiling every plan of a batch carries ONE timing, "timeInMicrosecondsForBatchedScan_<kernel>": the whole batch
 * kernel's time, under a label of its own so that it is never read as a per-query figure.
 *
 * Grouped batches (opt-in: vdl_set_batch_grouped(ctx, 1), or VDL_BATCH_GROUPED=1 in the environment when the context opens; off, every
 * grouped plan runs alone as above).  A plan whose ONE scan is a grouped scan over table columns (no second scan, no derived columns, no
 * prelude, not known to be empty) shares a batch with plans of the same columns and the same generated code under run-time bounds --
 * pivots, key and aggregates are part of that code; grouped and global plans never mix.  A row's group and aggregate terms do not depend
 * on anybody's bounds, only the SET of plans it passes does: the kernel keeps one table per non-empty set (2^K - 1 pass-class tables per
 * replica) in LDS, issues per row the 1 + aggregates atomics the unbatched scan issues, and folds the classes into the plans' tables once
 * per block.  With words = pivots x (1 + aggregates), a batch of K plans needs R x (((2^K - 1) x words) | 1) + 256 + aggregates + 1 words
 * within 8192 (64 KiB), R the largest power of two <= 8 that fits; the widest K of 4, 3, 2 is taken whose R is at least min(the
 * replicas the scan has alone, 2).  TPC-H Q1 (32 pivots, 8 words each): K = 4 at R = 2.  A scan whose table leaves no room for three
 * tables runs alone ("its group table leaves no room in LDS for a second plan's classes").  Only the eager tile form is batched (tuned:
 * at 2, 3, 4 row pairs per lane); the name carries ",grouped" and ",batch<K>,rtb>".  When the rows ONE plan keeps carry group keys
 * outside the pivots, that plan alone is rerun inside the call, on the general path at once -- its note becomes "alone: rerun after batch <b>:
 * <reason>" -- and the other slots keep their answers.  VDL_BATCH_WIDTH=k (k >= 2) caps the width of every batch, grouped or global.
 * vdl_plan_batch_code_bytes: the code size of the batch kernel that served the plan in the last vdl_run_batch / vdl_batch_jit_check,
 * 0 when none did.
 *
 * Join batches (opt-in: vdl_set_batch_joins(ctx, 1), or VDL_BATCH_JOINS=1 in the environment when the context opens; off, every plan
 * whose scan has derived columns or a prelude runs alone as above, with the same notes).  With the switch on the ONE scan of a plan may
 * have derived columns -- lookups through a join index, bits of a dimension bitmap or a semi-join set, LIKE tables, differences, row
 * ids, conditions -- and a prelude; it is global, or grouped with vdl_set_batch_grouped on as well.  Wide sums stay excluded.  Such plans
 * share a batch when, beside the same columns (the lookup targets' addresses and widths included) and the same generated code under
 * run-time bounds, (a) their preludes build the same tables -- the same LIKE heap and pattern, the same dimension or semi-join scan with
 * all its bounds, the same witness statements -- and (b) their conditions (IN lists, disjunctions, CASE WHEN tests) hold the same
 * literals.  What differs between the plans of a join batch are the range bounds of table columns and of filtered derived columns that
 * are no conditions.  The prelude runs ONCE per batch, through the first plan, by the code a plan alone runs; the kernel reads the fact
 * columns once, looks a row up once while any plan still wants it, computes every condition once per row, and keeps per row the set of
 * plans whose filters have held so far.  One prelude item is left out of (a): a dimension bitmap that a semi-join scan tests for the
 * very row whose bit it sets, made of range filters on the scanned table that the plan's scan applies itself with the same bounds
 * (TPC-H Q4's quarter): the batch leaves it open -- every row selected --, so plans for different quarters build one set and each
 * plan's own filter drops the rest.  A plan with no partner says "no other plan of the call builds the same lookup tables" or "its
 * conditions' literals differ from every other plan's".  A batch whose semi-join set cannot stand for the emitted `mod` (the indexed
 * table has more rows than the modulus) sends EVERY member back alone on the general path: "alone: rerun after batch <b>: <reason>".
 * A join batch is at most 8 plans wide within slots x (1 + aggregates) <= 32 (global) or the grouped rule above; only the eager tile form
 * is batched, the name carries ",derived" and ",batch<K>,rtb>".  Under vdl_plan_set_profiling the first plan of a join batch that
 * finalises also carries "timeInMicrosecondsForBatchedPrelude": the time of the batch's one prelude.  vdl_run_batch_sharded does not
 * read the switch. */
int  vdl_run_batch(vdl_ctx *ctx, vdl_plan *const *plans, int n);
const char *vdl_plan_batch_note(const vdl_plan *plan);
int  vdl_batch_jit_check(vdl_ctx *ctx, vdl_plan *const *plans, int n);
int  vdl_set_batch_grouped(vdl_ctx *ctx, int on);
int  vdl_set_batch_joins(vdl_ctx *ctx, int on);
int64_t vdl_plan_batch_code_bytes(const vdl_plan *plan);

int  vdl_n_outputs(const vdl_plan *plan);
/* k-th output in program order: `name` is the output field (resolve.py:64-78 splits it on
 * "__"), `tmp` the "tmpN" result key (N = id of the MaterializeCompact line). */
int  vdl_output(const vdl_plan *plan, int k, const char **name, const char **tmp,
                const int64_t **vals, size_t *n);
/* Results that stay in HBM.  With device outputs enabled, an output of 65536 values or more is not copied to the
 * host: vdl_output reports its length with *vals == NULL and vdl_output_device hands out the device pointer (int64
 * values, owned by the plan until it is run again or freed; the run has completed on the context's stream when
 * vdl_run returns).  Smaller outputs stay host-side (*dev_vals == NULL).  Q3 at SF100 returns 4 x 13.9M values:
 * 445 MB over PCIe is a quarter of the run (vdl_plan_set_order with the query's own LIMIT is the way not to make that copy). */
int  vdl_plan_set_device_outputs(vdl_plan *plan, int enabled);
int  vdl_output_device(const vdl_plan *plan, int k, const int64_t **dev_vals, size_t *n);

/* ---- wide sums: exact 128-bit SUM results from the fused aggregate scans ---------------------------------------------
 * Every FoldSum adds in int64 and wraps around, and so does the CPU oracle: a sum that leaves int64 comes back as a wrong
 * number, silently (Q1's sum_charge over the generated lineitem is 0.547 of INT64_MAX at SF100 and wraps from about SF183: measured).  The switch widens the ACCUMULATION.
 *   mode 0  off: everything as it is without the switch (the default; VDL_WIDE_SUMS=1|2 in the environment sets the mode at vdl_parse).
 *   mode 1  wide: every output carries a second vector of the same length, bits 64..127 of its exact value (vdl_output_high);
 *           vdl_output's vector is what it is with the switch off -- bits 0..63.
 *   mode 2  checked: as wide, and a run in which some output's high word is not the sign extension of its low word fails with
 *           VDL_ERR_OVERFLOW; the message names the output field, the group (its position in the result) and the exact value
 *           in decimal, and the outputs are not delivered (vdl_n_outputs is 0).
 * "Exact" is the SUM of the per-row terms in two's-complement 128-bit arithmetic.  The per-row TERM stays the int64 the program
 * computes, wrap-around included: overflow of a per-row product is out of scope, only the accumulation widens.  A sum that leaves
 * int64 on the way and comes back ends with a clean high word: excursions are no overflow.  COUNT, MIN, MAX and FIRST have the
 * sign extension as their high word.  An output that is a scalar expression over aggregates (avg = Divide(sum, count)) is
 * evaluated over the exact 128-bit aggregate values with 128-bit wrap-around, the int64 rules widened (x / 0 = x % 0 = 0,
 * MIN128 / -1 wraps, a shift count of 127 or more shifts everything out).
 * Served: plans that fuse as a whole (vdl_plan_is_fused) -- global and dense-domain grouped aggregate scans, with or without
 * derived columns -- on the precompiled kernels (a single-sum scan runs on k_mscan, not k_scan) and, with vdl_plan_set_jit, on
 * the specialised ones in every form the scan has (eager, staged, queue; packed, which only global scans over table columns
 * have): their names carry ",wide".  Refused with
 * VDL_ERR_UNSUPPORTED before any kernel runs, the message naming the route: a plan that does not fuse as a whole or whose
 * fusion is off (its sums would run through the GROUP BY tail or the per-operator folds); a fused plan whose rows carry group
 * keys outside the pivots (it would be rerun statement by statement); every sharded entry point (vdl_run_local, vdl_finalize*,
 * vdl_resolve_first, vdl_exchange_begin, vdl_run_sharded*) unless vdl_plan_set_wide_sums_sharded (below, with the sharded entry
 * points) has switched the merge of (lo, hi) pairs on.  vdl_run_batch runs such a plan alone inside the call ("alone: wide
 * sums are not batched").  With an order set the high vectors are permuted and cut with the low ones; keys are compared as the
 * int64 they are, and a key output whose value does not fit int64 fails the run with VDL_ERR_OVERFLOW naming it, in either mode.
 * vdl_plan_set_wide_sums: mode outside 0..2 is VDL_ERR_ARG.  vdl_output_high: *hi is NULL before a run and after a mode-0 run,
 * else n values (on the host also under vdl_plan_set_device_outputs: a fused plan assembles a handful of rows there).
 * vdl_plan_wide_note: what served the plan's scans in the last run ("wide: k_mscan grouped, 7 sums"), or the reason of a refusal.
 * vdl_plan_jit_check builds the wide units without a device when the switch is on.
 * vdl_wide_eval_bin: the 128-bit operator of the scalar expressions on its own, (alo, ahi) op (blo, bhi), `op` numbered as
 * the engine numbers the VDL binary operators (0 LogicalAnd, 1 LogicalOr, 2 BitwiseAnd, 3 BitwiseOr, 4 BitShift, 5 Equals, 6 Add,
 * 7 Subtract, 8 Greater, 9 Multiply, 10 Divide, 11 Modulo; anything else VDL_ERR_ARG); host only, no device needed. */
int  vdl_plan_set_wide_sums(vdl_plan *plan, int mode);
int  vdl_plan_wide_sums(const vdl_plan *plan);
int  vdl_output_high(const vdl_plan *plan, int k, const int64_t **hi, size_t *n);
const char *vdl_plan_wide_note(const vdl_plan *plan);
int  vdl_wide_eval_bin(int op, int64_t alo, int64_t ahi, int64_t blo, int64_t bhi, int64_t *lo, int64_t *hi);
/* ---- wide sums in the GROUP BY tail and the per-operator folds ----
 * vdl_plan_set_wide_sums_tail(plan, on): with on != 0 and vdl_plan_set_wide_sums at 1 or 2, vdl_run also serves the plans the switch
 * above refuses on ONE GPU: a plan that does not fuse as a whole (a fused front or a semi-join set, then the GROUP BY tail), a plan
 * whose fusion is off, and the statement-by-statement rerun of a fused plan whose rows carry keys outside the pivots.  Off by default
 * (VDL_WIDE_TAIL=1 sets it at vdl_parse; vdl_plan_set_wide_sums(plan, 0) clears it, and on a plan in mode 0 the call leaves it off);
 * with it off every refusal is what it was.  The
 * sharded entry points refuse such a plan whatever this switch says.
 *   - A FoldSum result is the exact two's-complement sum of its int64 per-entry terms (the term itself still wraps); bits 0..63 are
 *     bit for bit the switch-off result.  A fold over more than 2^31 entries is refused with VDL_ERR_UNSUPPORTED naming the count.
 *   - Wide where delivered: a wide sum that reaches an output through Project / Shuffle / MaterializeCompact carries its high words
 *     to vdl_output_high; every other output's high words are the sign extension.  Mode 2 checks the delivered values as above.
 *   - Checked where consumed: a wide sum read by any other statement (an element-wise operator, another fold, Gather, Scatter,
 *     Partition; a RangeV only takes its shape and does not count) must fit int64 in EITHER mode: if not, the run fails with
 *     VDL_ERR_OVERFLOW naming the consuming statement's id and operator, the first offending position and the exact value, and
 *     delivers nothing.  The checks' flags are read once, when the run ends.
 *   - With an order set the device order step permutes and cuts the high vectors with the low ones; a key output whose value does
 *     not fit int64 fails the run with VDL_ERR_OVERFLOW naming the key.
 *   - vdl_output_high_device: under vdl_plan_set_device_outputs, the high words of an output that stayed in HBM (beside
 *     vdl_output_device's pointer; vdl_output_high then hands out NULL for it); *dev_hi is NULL, with VDL_OK, for an output that is
 *     on the host or of a run without wide sums.
 *   - vdl_plan_wide_note names the route ("tail: k_group_fold ...").
 * vdl_wide_join_halves: the join of the two half sums the folds accumulate -- sl = the sum of the terms' low 32 bits (0 <= sl < 2^63),
 * sh = the sum of their arithmetic high halves (|sh| < 2^62) -- into bits 0..63 and 64..127 of sh * 2^32 + sl; host only. */
int  vdl_plan_set_wide_sums_tail(vdl_plan *plan, int on);
int  vdl_plan_wide_sums_tail(const vdl_plan *plan);
int  vdl_output_high_device(const vdl_plan *plan, int k, const int64_t **dev_hi, size_t *n);
int  vdl_wide_join_halves(int64_t sl, int64_t sh, int64_t *lo, int64_t *hi);
int  vdl_n_timings(const vdl_plan *plan);
int  vdl_timing(const vdl_plan *plan, int k, const char **label, double *usec);

/* ---- ordered and top-N results: ORDER BY / LIMIT -------------------------------------------------------------------
 * The plans this engine runs were compiled with the ORDER BY and LIMIT of their SQL cut off (the reference compiler stops
 * at an ORDER BY list and never lowers `top N`), so a run hands back every result row in program order.  An order set on
 * the plan makes vdl_run deliver the same outputs, all of them permuted by ONE permutation and cut to the limit, computed
 * where the rows are: on the device for everything a MaterializeCompact produces there (Q3's 4 x 13.9M values at SF100 never
 * leave HBM: 4 x 10 do), on the host for the handful of rows a fused plan assembles there.
 *   - keys are compared as signed int64, key by key in the order given, each ascending (descending[k] = 0) or descending;
 *   - rows equal on every key stay in the order of the unordered result (ties are broken by the row's position, ascending):
 *     the order is total and equals numpy's lexsort with the position as the last key;
 *   - a key is ordered by the int64 the engine holds for it.  For decimals and dates that is the SQL order.  A string field
 *     is its dictionary code (a heap offset, dictionary.csv): ordered as an int64 it groups equal strings but is NOT alphabetical.
 *     vdl_plan_set_order_text declares such a key as text over its heap column, and the key is then ordered by the strings
 *     themselves, on the device, through the heap's collation index (below);
 *   - limit 0 = all rows; limit L > 0 = the first min(L, m) rows of that order.  No keys and L > 0 = the first L rows in program
 *     order.  No keys and limit 0 clears the order: the plan runs as if none had ever been set.
 * A key names an output by its full field name (the `name` of vdl_output, e.g. "o_orderdate__orders__o_orderdate") or by its
 * "tmpN" key.  An unknown name, a name given twice, more than 8 keys or a negative limit: VDL_ERR_ARG (no device, no run needed:
 * the outputs are known from the program text).  At run time all outputs must have one length m (they are the columns of one
 * result), VDL_ERR_SHAPE names outputs and lengths otherwise; m = 0 is fine.  With vdl_plan_set_device_outputs the 65536 rule
 * applies to the ordered, cut outputs.  Sharded runs (vdl_run_sharded*, vdl_run_local, vdl_exchange_begin) refuse a plan with an
 * order set, VDL_ERR_UNSUPPORTED, unless vdl_plan_set_order_sharded (below, with the sharded entry points) has switched the merged
 * order on.  vdl_plan_set_order replaces the whole order and so switches it off again.
 * With an order set the timings carry one more entry, "timeInMicrosecondsForOrder": device events around the order step (the
 * host's own time where the step ran on the host). */
int  vdl_plan_set_order(vdl_plan *plan, int n_keys, const char *const *fields, const int *descending, int64_t limit);
/* After a run, what the order step did: "host m=.. rows=..", "topn m=.. rows=.. rounds=.. candidates=.. digits_used_up=0|1"
 * (selection rounds run, candidate rows the final step ordered) or "sort m=.. rows=.. partitions=..".  "" when no order is set. */
const char *vdl_plan_order_note(const vdl_plan *plan);
/* The host formulation of exactly that order, device-free: index_out[r] = position of the row of rank r, for r < min(limit or m, m).
 * keys[k] points to m int64.  What the engine itself uses for results that lie on the host. */
int  vdl_order_host(int n_keys, const int64_t *const *keys, const int *descending, int64_t m, int64_t limit, int64_t *index_out);

/* ---- text keys: alphabetical order from a collation index ------------------------------------------------------------
 * A string heap is an ordinary catalog column of one byte per slot ("part.p_brand.heap"): NUL-terminated strings at the offsets
 * dictionary.csv names, no alignment promised.  Its collation index maps every offset at which a string starts to that string's
 * dense rank in text order:
 *   - text order is strcmp order on UNSIGNED bytes (0x80 sorts after 0x7f), a string before its extensions; the heap's end
 *     terminates a last string without NUL;
 *   - an offset whose byte is NUL is the empty string, rank 0;
 *   - an offset whose byte is not NUL and whose predecessor is NUL (or offset 0) starts a string: rank = 1 + the number of DISTINCT
 *     non-empty strings of the heap that sort strictly before it.  Equal strings stored at different offsets share a rank: they tie,
 *     and the next key, then the position, decides, as SQL requires;
 *   - every other code -- negative, at or past the heap's end, inside a string -- names no string of the heap.
 * The index is one int32 per g heap bytes, g the largest power of two <= 8 that divides every start (4 * heap_n / 8 bytes for the
 * 8-aligned heaps MonetDB writes, never more than 4 bytes per heap byte).  It belongs to the context and goes with its column (drop,
 * re-registration, a new upload).  It is built by vdl_build_collation, or by the first run whose order needs it; that run then
 * carries a timing "timeInMicrosecondsForCollation_<heap>" of its own (the build is not part of timeInMicrosecondsForOrder; with
 * vdl_plan_set_profiling also "timeInMicrosecondsForCollation{Mark,Starts,Words,Sort,Ranks,Table}_<heap>", the build's steps).
 * Heaps of 2^31 bytes or more, and heaps with a string longer than 256 bytes: VDL_ERR_UNSUPPORTED, the message naming heap and
 * length.  A column that is not one byte wide: VDL_ERR_ARG.
 * vdl_collation_info: present = 0 (and zeros) when the column has no index; otherwise the strings that start in the heap, how many
 * of them are distinct, and the longest one's bytes.  Any out pointer may be null.
 *
 * vdl_plan_set_order_text marks ONE key of the order currently set (named as in vdl_plan_set_order) as text over heap_column;
 * heap_column NULL clears the mark.  VDL_ERR_ARG if `field` is no key of the current order; no device and no run needed.  (An
 * output is a key at most once -- vdl_plan_set_order refuses a field given twice, under either of its names -- so one mark per field
 * is all there is to set.)
 * vdl_plan_set_order clears all marks.  At run time the order word of a text key is rank ^ flip like any key's: the codes are
 * translated by one kernel per text key inside the order step, the selection / sort / gather run on the ranks as on any int64
 * key, and results a fused plan assembles on the host get their ranks from the same device index.  The heap must be registered
 * when the plan runs (VDL_ERR_ARG naming it otherwise).  A run that meets a code that names no string of the heap fails with
 * VDL_ERR_SHAPE, the message naming key, heap, how many such rows there were and the first of them: nothing is ordered by garbage.
 * With vdl_plan_set_profiling the translate launches are also timed alone, "timeInMicrosecondsForOrderTextKeys" (they lie inside
 * timeInMicrosecondsForOrder).  vdl_plan_order_note ends in " text_keys=<n>" when n > 0 keys were text.  vdl_run_batch applies such an order as vdl_run does;
 * sharded entry points treat the plan like any ordered plan (on the exchange route the heap must be replicated: vdl_plan_set_order_sharded). */
int  vdl_build_collation(vdl_ctx *ctx, const char *heap_column);
int  vdl_collation_info(const vdl_ctx *ctx, const char *heap_column, int *present, int64_t *strings, int64_t *distinct, int *max_bytes);
int  vdl_plan_set_order_text(vdl_plan *plan, const char *field, const char *heap_column);
/* The host formulation of exactly those ranks, device-free (a sort under strcmp-on-unsigned): ranks_out[i] for codes[i], i < m;
 * a code that names no string gets -1, *n_bad counts them and *first_bad is the first such i (-1: none).  n_bad / first_bad may be
 * null. */
int  vdl_collate_host(const int8_t *heap, int64_t heap_n, const int64_t *codes, int64_t m, int64_t *ranks_out, int64_t *n_bad,
                      int64_t *first_bad);
/* A TEST AID, not a query path: the same through the device index of a registered heap column (built now if the column has none),
 * codes and ranks in HOST memory, one translate launch in between.  Bad codes are reported as by vdl_collate_host, not refused.
 * It exists so that the index can be compared with vdl_collate_host code by code; an ordered run never calls it. */
int  vdl_collate_device(vdl_ctx *ctx, const char *heap_column, const int64_t *codes, int64_t m, int64_t *ranks_out, int64_t *n_bad,
                        int64_t *first_bad);


/* Debugging aid for parity work.  With tracing on, a vdl_run that goes statement by statement (plan not fused, or
 * vdl_plan_set_fusion(plan, 0)) keeps a host copy of every statement's vector as it stood right after the statement:
 * n slots, vals[i] and ok[i] (1 = the slot holds a value, 0 = EPS; vals is 0 there).  `form` names the engine's
 * internal representation ("dense", "sparse", "range", "onehot", ...).  vals / ok are NULL for statements whose
 * evaluation was deferred at that point (fused expression trees, lazy gathers) and for vectors of more than 2^22
 * slots.  Entries are in execution order and stay valid until the plan runs again or is freed. */
int  vdl_plan_set_trace(vdl_plan *plan, int enabled);
int  vdl_n_traced(const vdl_plan *plan);
int  vdl_traced(const vdl_plan *plan, int k, int *node_id, const char **form, int64_t *n,
                const int64_t **vals, const uint8_t **ok);

/* Per-kernel device time of the last vdl_run()/vdl_run_local(), measured with HIP events
 * on the stream the kernels were launched on; enabled with vdl_plan_set_profiling(). */
int  vdl_plan_set_profiling(vdl_plan *plan, int enabled);
/* Rows scanned and algorithmic bytes read by the dominant (fused scan) kernel of the last
 * run, and its device time in microseconds (0 if profiling was off). */
int  vdl_plan_scan_stats(const vdl_plan *plan, int64_t *rows, int64_t *algo_bytes, double *usec);
/* HBM bytes ONE launch of that kernel moves over the columns registered now (measurement; call after a run, outside any
 * timed region).  A scan that reads every column with the tile moves its algorithmic bytes.  A scan specialised to read
 * late (vdl_plan_set_jit: staged reads) moves the eager columns in full plus 128 bytes for every cache line of a late
 * column in which some row was still in when the column was read -- the memory side fetches whole 128-byte lines
 * (tools/ubench/fetch_calib.hip) -- and that number is COUNTED: a census build of the same kernel form runs once.
 * `detail` (may be null): "column=bytes ..." text, valid until the next call.
 * Only the lines of the scanned (fact) table are counted: what the scan's lookups fetch on the dimension side -- catalog columns or,
 * under vdl_set_lookup_images, their images -- is not part of this number. */
int  vdl_plan_scan_traffic(vdl_ctx *ctx, vdl_plan *plan, int64_t *bytes_moved, const char **detail);

/* ---- sharded execution: one process per GPU, columns sharded by row range --------
 * A plan whose outputs are global folds keeps its mergeable state in `n_words` int64
 * words, each tagged with a VDL_REDUCE_* operator.  Each rank runs the local phase over
 * its row range, the caller merges the words across ranks (RCCL all-reduce through
 * torch.distributed, one call per operator class), and every rank finalises. */
int  vdl_plan_partial_spec(const vdl_plan *plan, int64_t *n_words, const int32_t **reduce_ops);
/* Local phase, asynchronous on the context stream; dev_partials = caller-owned device
 * buffer of n_words int64 (fully overwritten). */
int  vdl_run_local(vdl_ctx *ctx, vdl_plan *plan, void *dev_partials);
/* After the merge: produce the outputs from the (merged) words; synchronises. */
int  vdl_finalize(vdl_ctx *ctx, vdl_plan *plan, const void *dev_partials);
/* Placement for plans that do not fuse: `table` is split by rows over the ranks, every other table is replicated.
 * With it, vdl_plan_partial_spec / vdl_run_local / vdl_finalize also serve general plans whose outputs hang off
 * GLOBAL folds over that table (a join followed by an ungrouped aggregate: TPC-H Q14, Q19): three words per fold
 * {value, first slot, count}, everything below the folds checked to be row-local, the statements above them run on
 * the merged scalars.  VDL_ERR_UNSUPPORTED with the reason otherwise.  Also what vdl_exchange_spec records. */
int  vdl_plan_set_sharded_table(vdl_plan *plan, const char *table);
/* Global index of this rank's first row (default 0); row ids in VDL_REDUCE_FIRST words are global. */
int  vdl_plan_set_row_offset(vdl_plan *plan, int64_t row0);
/* Second merge phase of VDL_REDUCE_FIRST words (see the enum); asynchronous on the context stream. */
int  vdl_resolve_first(vdl_ctx *ctx, vdl_plan *plan, void *dev_partials);
/* Pipelined form (two slots, 0 and 1): `begin` enqueues the copy of the merged words to a pinned host
 * slot and returns at once; `end` waits for that copy only -- younger launches on the stream keep
 * running -- and produces the outputs.  Lets a driver overlap the host side of query k with the
 * kernels of query k+1. */
int  vdl_finalize_begin(vdl_ctx *ctx, vdl_plan *plan, const void *dev_partials, int slot);
int  vdl_finalize_end(vdl_ctx *ctx, vdl_plan *plan, int slot);

/* ---- sharded Partition (joins / sparse GROUP BY, e.g. TPC-H Q3): row exchange -------------------
 * For plans that are not fused but whose outputs depend on the sharded table only through
 * Scatter(x, _, Partition(key, RangeC min cnt 1)) -- the group-by lowering of
 * /root/reference/src/Vlite.hs:1056-1060,1082-1098 -- every rank
 *   1. vdl_exchange_begin : runs the statements up to the partition key and the scattered vectors on
 *      its own rows and reports how many rows go to each rank (rank r owns the keys of
 *      [min + r*cnt/world, min + (r+1)*cnt/world)); rows keep their order inside each destination;
 *   2. vdl_exchange_pack  : writes the n_send = sum(counts) rows, grouped by destination, into a
 *      caller-owned device buffer of n_columns x n_send int64 (column c starts at c * n_send):
 *      key, scattered vectors, one validity word;
 *   3. (caller) all-to-all of every column over RCCL (torch.distributed.all_to_all_single with the
 *      counts as split sizes);
 *   4. vdl_exchange_finish: runs Partition / Scatter / Fold / MaterializeCompact on the received
 *      rows (n_columns x n_recv int64, same layout).  The outputs of rank 0, 1, ... concatenate to the
 *      unsharded result (keys ascend across ranks; stability makes FoldChoose pick the same row).
 * Dimension tables must be replicated on every rank; only the partitioned table is sharded.
 * vdl_exchange_pack returns when the send buffer is complete; the received rows must be complete
 * when vdl_exchange_finish is called (synchronise the collective's stream first unless the engine
 * runs on that stream, vdl_set_stream).
 * vdl_exchange_spec checks the structure; with sharded_table != NULL ("lineitem") it also verifies
 * that everything below the Partition is row-local over that table (element-wise operators,
 * constants, Gathers out of replicated vectors), lets the statements above the Partition read the
 * replicated tables' columns (the plan remembers the placement for vdl_exchange_begin), and returns
 * VDL_ERR_UNSUPPORTED with the reason
 * otherwise.  world <= 128. */
int  vdl_exchange_spec(const vdl_plan *plan, const char *sharded_table, int *n_columns);
int  vdl_exchange_begin(vdl_ctx *ctx, vdl_plan *plan, int world, int64_t *counts_host /* world */);
int  vdl_exchange_pack(vdl_ctx *ctx, vdl_plan *plan, void *dev_send);
int  vdl_exchange_finish(vdl_ctx *ctx, vdl_plan *plan, const void *dev_recv, int64_t n_recv);

/* ---- multi-GPU behind this boundary: one process per GPU, the context owns the communicator --------------
 * (SURVEY.md section 8(b),(e).)  A Haskell host -- or vdlrun --gpus N, or bench.py -- starts one process per GPU; each opens
 * its context on its device, holds its row range of the sharded table (and the replicated tables in full), joins the
 * communicator and calls vdl_run_sharded(); the collectives happen inside.
 *
 *   vdl_comm_unique_id : any one rank makes the 128-byte id (ncclGetUniqueId) and the host hands the bytes to the others
 *                        (a file, a pipe, an environment variable, MPI, a torch store: any channel);
 *   vdl_comm_init      : RCCL communicator over xGMI on the context's device (librccl is opened here, not at load time);
 *   vdl_comm_init_host : instead of RCCL, collectives supplied by the caller over HOST memory (hosts that already have
 *                        MPI / gloo; the tests' in-process stand-in).  The engine stages through pinned buffers.  These two
 *                        callbacks are the only ones in this interface; both are called by every rank, in the same order.
 *
 * vdl_run_sharded picks the route from the plan:
 *   outputs = global / dense-domain grouped folds (vdl_plan_partial_spec succeeds: fused plans, or general plans after
 *   vdl_plan_set_sharded_table): local phase -> ONE all-gather of the partial words -> merge kernel -> finalise; every rank
 *   ends with the full result.  FoldChoose words travel as (global row id, value) pairs: no second round.
 *   plans with a Partition (vdl_plan_set_sharded_table names the row-sharded table): local phase -> ONE all-gather of
 *   {status, rows per destination} -> ONE grouped send / receive of all columns -> local tail; rank r ends with the
 *   groups of key range r, and the ranks' outputs concatenate in rank order to the unsharded result.
 * (more routes: below, at vdl_plan_sharded_route)
 * vdl_run_sharded_begin / _end split the fold route for pipelined callers (slots 0 / 1): `begin` queues the scan on the
 * engine stream and merge + copy-out behind it on the communication stream and returns; `end` waits for that slot's copy
 * only, so the collective of query k hides behind the scan of query k+1. */
#define VDL_COMM_ID_BYTES 128
typedef struct vdl_comm_host {
    void *user;
    /* every rank contributes `bytes` from `send`; `recv` (world * bytes) gets rank r's block at r * bytes.  0 = ok. */
    int (*all_gather)(void *user, const void *send, void *recv, size_t bytes);
    /* rank-major blocks: send_bytes[r] bytes go to rank r, recv_bytes[r] bytes arrive from rank r.  0 = ok. */
    int (*all_to_all)(void *user, const void *send, const size_t *send_bytes, void *recv, const size_t *recv_bytes);
} vdl_comm_host;
int  vdl_comm_unique_id(void *id_out /* VDL_COMM_ID_BYTES */);
int  vdl_comm_init(vdl_ctx *ctx, int rank, int world, const void *id /* VDL_COMM_ID_BYTES */);
int  vdl_comm_init_host(vdl_ctx *ctx, int rank, int world, const vdl_comm_host *transport);
int  vdl_comm_info(const vdl_ctx *ctx, int *rank, int *world, const char **transport /* "rccl" | "host" */);
void vdl_comm_free(vdl_ctx *ctx);                       /* also done by vdl_close */
/* A third route:
 *   fused plans with a semi-join set (EXISTS / IN, TPC-H Q4) whose source table is the sharded one and whose scans read replicated
 *   tables: every rank builds the set from its rows -> ONE all-gather of the sets -> OR kernel -> the scans run everywhere
 *   against the complete set; every rank ends with the full result.
 * A fourth, for plans the exchange cannot serve (two Partitions, folds over grouped results: TPC-H Q16) whose work on the sharded
 *   table is a fused front (filter + projection in one scan): every rank runs the front over its rows -> all-gather of the row
 *   counts -> all-gather of {status, survivors} -> ONE grouped send / receive of the survivors' vectors to every rank (rank after
 *   rank = row order) -> the statements above the front run everywhere on the complete vectors; every rank ends with the full
 *   result.  Tried after the exchange; the row-id conditions of the front count from the table's first row.
 * A fifth, the "chain" (TPC-H Q18: a GROUP BY over ALL rows of the sharded table whose groups only feed position sets --
 *   Scatter(constant, size, a value of the group): the semi-join set of `in (select .. group by .. having ..)` -- and a rest that reads the
 *   sets and the table a second time): the rows travel to the owners of their key range as on the exchange route and every owner runs the
 *   GROUP BY on complete groups -> all-gather of {status, positions found, length} + ONE grouped send / receive per set: every rank
 *   builds the same sets -> the rest runs with the sets given: per-row work on each rank's OWN rows, all-gather of {status, rows} and
 *   ONE grouped send / receive of the rows that reach the next Partition (rank after rank = row order), the tail on every rank; every
 *   rank ends with the full result (VDL_NO_CHAIN_ROUTE=1 switches it off).
 * The last resort, for a plan none of the five serves: the sharded table's columns the plan loads are all-gathered ONCE per
 *   catalog state into plan-owned buffers, and every rank runs the whole query over them -- the query itself does not scale, later
 *   runs move nothing, every rank ends with the full result ("replicate"; VDL_NO_REPLICATE_ROUTE=1 turns it into the refusal with the
 *   reasons).
 * vdl_plan_sharded_route tells which route a plan takes ("fold" | "set" | "exchange" | "front" | "chain" | "replicate") and whether every rank
 * ends with the whole answer (replicated = 1) or with its slice (0: concatenate the ranks' outputs in rank order; the exchange
 * route only, and not when an order it can merge is switched on with vdl_plan_set_order_sharded: every rank then ends with the same
 * ordered rows). */
int  vdl_plan_sharded_route(vdl_ctx *ctx, vdl_plan *plan, const char **route, int *replicated);
int  vdl_run_sharded(vdl_ctx *ctx, vdl_plan *plan);     /* results through vdl_output as after vdl_run */
int  vdl_run_sharded_begin(vdl_ctx *ctx, vdl_plan *plan, int slot);
int  vdl_run_sharded_end(vdl_ctx *ctx, vdl_plan *plan, int slot);
/* ---- ORDER BY / LIMIT in a sharded run ----
 * vdl_plan_set_order_sharded(plan, on): with on != 0, vdl_run_sharded, vdl_run_sharded_begin and vdl_run_sharded_end accept a plan
 * with an order set, and EVERY rank ends with the same ordered, cut answer -- the one vdl_run gives for the unsharded data
 * (vdl_plan_sharded_route then reports replicated = 1 on every route).  on = 0 (the default, and what vdl_plan_set_order leaves behind)
 * keeps the refusal.  vdl_run_local and vdl_exchange_begin refuse either way: their callers run their own collectives, and the
 * merge lives in vdl_run_sharded; the message says so.
 *   - routes where every rank holds the whole result (fold, set, front, chain, replicate): the order step runs on each rank as in
 *     vdl_run, in vdl_run_sharded_end for the pipelined pair.  No further collective; vdl_plan_order_note as after vdl_run.
 *   - the exchange route, 0 < limit <= 4096: rank r selects its first L_r = min(limit, m_r) of its m_r result rows and writes
 *     them as a candidate block (K order words u = key ^ flip and every output, in its sorted order); ONE all-gather of {status, L_r,
 *     m_r} -- if the tail or the order step failed anywhere, every rank returns an error here (the failing rank its own) and no data
 *     travels --; ONE grouped send / receive of the blocks; one kernel ranks every candidate among the `world` sorted runs by binary
 *     search and writes the first L = min(limit, sum m_r) rows of every output.  The ranks' results concatenate in rank order, so
 *     (rank, place in the rank's run) stands for the row's position: ties come out as in the unsharded run.  A text key's heap must
 *     be replicated: a heap column of the sharded table is refused, VDL_ERR_UNSUPPORTED naming key and heap.  vdl_plan_order_note
 *     = the local note + " | merge world=W candidates=N rows=L"; "timeInMicrosecondsForOrder" is the local selection,
 *     "timeInMicrosecondsForOrderMerge" the staging and the merge kernel (device events; the collective is not in it).
 *   - the exchange route with limit 0 or limit > 4096 would have to gather every result row: VDL_ERR_UNSUPPORTED, the message naming
 *     the limit, the bound and the route, before any collective (and before a device is needed). */
int  vdl_plan_set_order_sharded(vdl_plan *plan, int on);
/* The merge rule on the host, device-free: `world` sorted runs of counts[r] candidates each, one after the other (N = sum counts);
 * words[k * N + j] = order word k of candidate j (n_keys <= 8; unsigned, ascending).  Candidate j of run r takes the place
 *   (index in its run) + sum over q < r of |{x in run q : x <= j}| + sum over q > r of |{x in run q : x < j}|
 * under the lexicographic comparison of the words -- the order of (u_1, .., u_K, run, index).  The first L = min(limit or N, N) places:
 * run_out[i], index_out[i] = the candidate at place i; *n_out = L (may be NULL). */
int  vdl_order_merge_host(int world, int n_keys, const int64_t *counts, const uint64_t *words, int64_t limit, int64_t *run_out,
                          int64_t *index_out, int64_t *n_out);
/* The merge rule of the gathered partial words on the host (what the device kernel computes): `gathered` holds, per rank, a block
 * of `stride_words` int64 -- n_words words, the same words with VDL_REDUCE_FIRST entries resolved to values and, in the blocks
 * vdl_run_sharded itself gathers, ONE status word of the rank's local phase (stride_words = 2 * n_words + 1; pass 0 for bare blocks
 * of 2 * n_words).  status_out (may be NULL; needs the status word): [0] = the first non-zero status over the ranks, [1] = that
 * rank (-1: every local phase succeeded).  For hosts / tests that want to check a transport without a GPU. */
int  vdl_comm_merge_host(int world, int64_t n_words, const int32_t *ops, const int64_t *gathered, int64_t stride_words, int64_t *out,
                         int64_t *status_out);
/* ---- wide sums in a sharded run ----
 * vdl_plan_set_wide_sums_sharded(plan, on): with on != 0 and vdl_plan_set_wide_sums at 1 or 2, vdl_run_sharded, vdl_run_sharded_begin and
 * vdl_run_sharded_end accept a plan that fuses as a whole (vdl_plan_is_fused, no semi-join set) on the fold route, and EVERY rank ends
 * with what vdl_run over the whole table delivers under the same mode: the low words in vdl_output, the high words in vdl_output_high,
 * scalar outputs (avg) evaluated over the exact merged values.  on = 0 (the default; VDL_WIDE_SHARDED=1 in the environment sets it at
 * vdl_parse; vdl_plan_set_wide_sums(plan, 0) clears it) keeps the refusal of every sharded entry point.
 *   - A rank's block of the ONE all-gather is [n_words raw][n_words resolved][status][n_words high words of the raw words]: 3 * n_words + 1
 *     int64, the first 2 * n_words + 1 as without the switch.  The merge adds a SUM word's (lo, hi) pairs with carry in rank order
 *     (deterministic); MIN, MAX and FIRST words are merged as ever and carry the sign extension; a failed rank sends zeros.
 *   - Mode 2 is checked on the MERGED values, in vdl_run_sharded_end: a rank whose own partial sum leaves int64 while the total fits is no
 *     failure; a total that does not fit fails on every rank with VDL_ERR_OVERFLOW and vdl_run's message (field, group, decimal value).
 *   - With vdl_plan_set_order_sharded also on, the order step runs after the merge as it does without the switch and permutes the high
 *     vectors with the low ones.
 *   - vdl_plan_wide_note names the scans and ends in "; merged over N ranks".
 *   - Still refused, VDL_ERR_UNSUPPORTED naming the route, before a kernel or a collective runs and from the plan alone (every rank
 *     decides the same): a fused plan with a semi-join set (the set route); a plan that does not fuse as a whole or whose fusion is off
 *     -- sharded through its global folds (k_fold_global) or on the exchange, front, chain or replicate route (k_group_fold /
 *     k_seg_fold); and the entry points that leave the collectives to their caller -- vdl_run_local, vdl_finalize*, vdl_resolve_first,
 *     vdl_exchange_begin -- except inside vdl_run_sharded's own calls.  A fused plan whose rows carry group keys outside the pivots
 *     fails as it does unsharded.
 * vdl_comm_merge_host_wide: the merge rule of such blocks on the host (what the device kernel computes); stride_words >= 3 * n_words + 1
 * (0 = exactly that), rank r's high word of word i at gathered[r * stride_words + 2 * n_words + 1 + i]; out_lo is what vdl_comm_merge_host
 * gives for the blocks' first 2 * n_words + 1 words; status_out as there. */
int  vdl_plan_set_wide_sums_sharded(vdl_plan *plan, int on);
int  vdl_plan_wide_sums_sharded(const vdl_plan *plan);
int  vdl_comm_merge_host_wide(int world, int64_t n_words, const int32_t *ops, const int64_t *gathered, int64_t stride_words, int64_t *out_lo,
                              int64_t *out_hi, int64_t *status_out);
/* ---- batched runs, sharded (DESIGN.md section 7 "Batches") ----
 * vdl_run_batch_sharded: n plans in ONE sharded call.  After VDL_OK every plan holds, on every rank, what vdl_run_sharded of that plan
 * alone would have left, bit for bit; no other entry point changes.  Every plan is classified from the plan alone, so every rank
 * decides the same, before a kernel or a collective runs:
 *   shared : the plan fuses as a whole, builds no semi-join set, takes the fold route and has wide sums off.  The shared plans' partial
 *            words travel in ONE all-gather and are merged by ONE launch (k_merge_words_batch), whatever their number.  A rank's
 *            block is the concatenation, in call order, of one segment per shared plan: [raw n_words][the words again with FoldChoose
 *            entries resolved -- only if the plan has a VDL_REDUCE_FIRST word][status]; h = (first ? 2 : 1) * n_words + 1 words.
 *            The local phase is per rank and free in its grouping: shared plans whose one scan is a global aggregate scan go
 *            through vdl_run_batch's grouping and batch kernels, their slots' words written straight into the send block; every
 *            other shared plan (a grouped scan -- also under vdl_set_batch_grouped --, lookup tables, no partner on this rank) runs its
 *            own scans into its segment.  Ranks may group differently; the collective does not depend on it.
 *   own    : everything else -- the set, exchange, front, chain and replicate routes, unfused fold plans, wide plans that
 *            vdl_run_sharded accepts -- runs through vdl_run_sharded after the shared part, one at a time, in call order.
 * An order is allowed only with vdl_plan_set_order_sharded (a shared plan's is applied on the host after the merge); an order without
 * it, and a wide plan vdl_run_sharded would refuse, fail the whole call up front, the message naming the plan's index.  Argument
 * errors as vdl_run_batch's; no communicator: VDL_ERR_ARG.
 * Failures: a plan whose local phase fails on a rank -- a batch scan that throws fails its batch's plans there -- still takes part in
 * the collective (its segment zeroed, its status set).  Every rank reads the same merged status words and the call fails with the
 * LOWEST failing plan index: on the failing rank with its own code and message, elsewhere with VDL_ERR_UNSUPPORTED ("sharded run: the
 * local phase failed on rank r ..."), both prefixed "plan i: ".  The other shared plans keep their answers; no own plan is started.
 * Out of scope: a pipelined begin / end pair, wide sums in a batch, one pass shared between grouped plans.
 * vdl_batch_sharded_layout (no device, no communicator needed): per plan its segment's offset (-1: an own plan) and height (0), and
 * the block's words.  vdl_plan_batch_sharded_note: "collective 0: words [<off>,<off+h>) of <B>" or "own: <route> route", of the last
 * of the two calls; vdl_plan_batch_note says, in vdl_run_batch's words, how this rank's local phase grouped a shared plan.
 * vdl_comm_merge_host_batch: the merge rule of such blocks on the host (what k_merge_words_batch computes): plan q's segment at
 * offsets[q] of every rank's block_words words, ops_concat / out_concat the plans' operators / merged words one after the other,
 * status_out (may be null) {first non-zero status, its rank or -1} per plan. */
int  vdl_run_batch_sharded(vdl_ctx *ctx, vdl_plan *const *plans, int n);
int  vdl_batch_sharded_layout(vdl_ctx *ctx, vdl_plan *const *plans, int n, int64_t *offsets, int64_t *heights, int64_t *block_words);
const char *vdl_plan_batch_sharded_note(const vdl_plan *plan);
int  vdl_comm_merge_host_batch(int world, int n, const int64_t *n_words, const int64_t *offsets, const int32_t *ops_concat, const int64_t *gathered,
                               int64_t block_words, int64_t *out_concat, int64_t *status_out);

#ifdef __cplusplus
}
#endif
#endif /* VDL_H */
