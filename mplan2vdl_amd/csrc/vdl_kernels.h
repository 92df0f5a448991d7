// vdl_kernels.h -- launch wrappers for the HIP kernels (gfx950): vdl_kernels.hip (fused scan, column generator),
// vdl_mscan.hip (multi-aggregate / grouped scan), vdl_ops.hip (per-operator kernels), vdl_partition.hip.
// All launchers are asynchronous on the given stream and return the hipError_t of the launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vdl_fuse.h"

namespace vdl {

// ---- operand descriptor of the per-operator kernels --------------------------------
// A vector operand is a column of 1/2/4/8-byte signed integers, or a virtual range
// (RangeV / RangeC never touch memory: /root/reference/src/Vdl.hs:428-434 notes the
// backend "only materializes what's needed").
enum SrcKind : int { SRC_I64 = 0, SRC_I32 = 1, SRC_I16 = 2, SRC_I8 = 3, SRC_RANGE = 4 };
struct Src {
    const void *p = nullptr;
    int kind = SRC_I64;
    int64_t from = 0, step = 0;
};

// ---- fused scan ----------------------------------------------------------------------
struct ScanArgs {
    int ncol = 0, nagg = 0;
    int64_t n = 0;
    const void *ptr[kMaxScanCols] = {};
    int width[kMaxScanCols] = {};            // bytes: 1, 2, 4, 8
    int filtered[kMaxScanCols] = {};         // 0: column has no range filter
    int64_t lo[kMaxScanCols] = {}, hi[kMaxScanCols] = {};
    int kind[kMaxScanAggs] = {};             // AGG_SUM / AGG_MIN / AGG_MAX
    uint32_t used[kMaxScanAggs] = {};        // bit c: column c contributes a factor
    uint32_t plain[kMaxScanAggs] = {};       // bit c: that factor is the bare column (a=0, s=1)
    int64_t fa[kMaxScanAggs][kMaxScanCols] = {}, fs[kMaxScanAggs][kMaxScanCols] = {};
    int64_t constant[kMaxScanAggs] = {};     // datum when the aggregate has no column factor
    int64_t *block_partials = nullptr;       // [grid][1 + nagg]
    int never = 0;
    int chunked = 0;                         // tile->block mapping: 0 grid-stride, 1 contiguous chunks
};

struct ScanLaunch { int grid = 0, block = 0, variant = 0; };
// Chooses template instantiation and grid for (ncol, nagg) on this device.
ScanLaunch scan_launch_config(ScanArgs &a, int num_cus);
hipError_t launch_scan(const ScanArgs &a, const ScanLaunch &cfg, hipStream_t s);
// Reduces the per-block partials into words[0..nagg] = {count, agg0, ...}.
hipError_t launch_scan_finish(const int64_t *block_partials, int nblocks, int nagg, const int *kinds_dev_or_null,
                              const ScanArgs &a, int64_t *words, hipStream_t s);
const char *scan_kernel_name(const ScanLaunch &cfg);

// ---- multi-aggregate fused scans (vdl_mscan.hip): global and grouped (dense-domain GROUP BY) ----
ScanLaunch mscan_launch_config(const MScanCols &cols, MScanDesc &d, bool grouped, int num_cus);
const char *mscan_kernel_name(const ScanLaunch &cfg);
// out: global form 1 + nagg words {row count, aggregates}; grouped form pcount * (nagg + 1) + 1 words: per
// bucket {row count, aggregates...}, last word = rows whose key fell outside [pmin, pmin + pcount).
// resolve_first: turn AGG_FIRST row ids into column values (single rank only).
// jit_fn: the scan kernel specialised for this plan (vdl_jit.cpp) instead of the precompiled variant cfg names
// out_hi: a wide-sums scan (d.wide) leaves bits 64..127 of every word of `out` at the same place of out_hi -- the
// exact high word of a SUM aggregate, the sign extension of every other word (an AGG_FIRST word: of the row id; the host extends the value)
hipError_t launch_mscan(const MScanCols &cols, const MScanDesc &d, const MScanDesc *dev_desc, const ScanLaunch &cfg, bool grouped,
                        bool never, int64_t *out, bool resolve_first, hipStream_t s, hipFunction_t jit_fn = nullptr, int64_t *out_hi = nullptr);
int mscan_sums(const MScanDesc &d);                                  // its SUM aggregates: the high words a wide scan carries per block / bucket
int64_t mscan_partial_words(const MScanDesc &d, bool grouped);       // words of ONE block's partials (MScanDesc::block_partials), wide or not
// the wide-sums build of the precompiled kernels (vdl_mscan_wide.hip): variant for variant the shapes of vdl_mscan.hip
const void *mscan_wide_fn(int variant);
hipError_t launch_mscan_wide_kernel(int variant, int grid, int block, size_t lds_bytes, hipStream_t s, const MsArgs &a, const MScanDesc *dev_desc);
hipError_t launch_mscan_finish_wide(const MScanDesc &d, const MScanDesc *dev_desc, int nblocks, bool grouped, int64_t *out, int64_t *out_hi, hipStream_t s);
// A batched scan (vdl_run_batch): `fn` is the kernel specialised for k plans that share `cols` (vdl_jit.cpp, Shape::batch), b.d[q] slot
// q's descriptor on the device, b.partials room for grid x k x (1 + nagg) words; the finish step folds the blocks' partials and leaves slot
// q's 1 + nagg words at outs[q].  d: any slot's descriptor on the host (the aggregates' kinds are the same in all of them).
// grouped: a grouped batch (2 .. kMaxBatchGrouped plans; d.replicas = the replicas the kernel was built for): launched with
// mscan_batch_lds_bytes of dynamic LDS, b.partials room for grid x k x (pcount * (1 + nagg) + 1) words; slot q's pcount * (1 + nagg) + 1 words
// end up at outs[q] as launch_mscan leaves them, FoldChoose resolved.
hipError_t launch_mscan_batch(const MScanCols &cols, const MScanDesc &d, const MsBatch &b, int k, int grid, int64_t *const *outs, hipStream_t s, hipFunction_t fn,
                              bool grouped = false);
size_t mscan_batch_lds_bytes(const MScanDesc &d, int k);
// for the specialiser: the by-value arguments, the chosen variant's shape, the dynamic LDS of a launch
MsArgs mscan_args(const MScanCols &cols);
void mscan_variant_shape(const ScanLaunch &cfg, int *nc, int *u, bool *vec, bool *grouped, bool *der);
size_t mscan_lds_bytes(const MScanDesc &d, bool grouped);
// Projection scans (ProjPlan, vdl_fuse.h).  launch_project_select: a selection over a table's rows as a bitmap (d.bitmap_only = 1:
// a dimension scan, out_ptr[0] = the bitmap) or as bits set in a semi-join set (d.bitmap_only = 2).
int64_t project_tiles(int64_t n);
// groups (64 rows) of a step image of n rows, padded to whole tiles of the projection scans (vdl_column_image.h Steps)
int64_t project_step_groups(int64_t n);
hipError_t launch_project_select(const MScanCols &cols, const MScanDesc *dev_desc, int num_cus, hipStream_t s, hipFunction_t jit_fn = nullptr);
bool project_select_vec(const MScanCols &cols);          // the 16-byte-load form applies (alignment of the deciding columns)
// the fused front in ONE pass (vdl_mscan_body.h: project_front_body): scols / dev_sdesc = the deciding columns as the select pass saw
// them (out_ptr[0] = the selection's bitmap or null), tcols / dev_tdesc = every column with the output vectors (out_idx, out_ptr, out_cap);
// look = project_look_bytes(n) bytes of scratch; the survivors' number is left at total_dev and (if not null) in pinned total_host
int64_t project_look_bytes(int64_t n);
hipError_t launch_project_front(const MScanCols &scols, const MScanDesc *dev_sdesc, const MScanCols &tcols, const MScanDesc *dev_tdesc, void *look,
                                int64_t *total_dev, int64_t *total_host, int num_cus, hipStream_t s, hipFunction_t jit_fn = nullptr);
// sharded FoldChoose: after the MIN all-reduce of the row-id words, the owning rank substitutes the value, others 0
hipError_t launch_mscan_resolve_first(const MScanCols &cols, const MScanDesc &d, const MScanDesc *dev_desc, int64_t *table, hipStream_t s);

// ---- synthetic data --------------------------------------------------------------------
hipError_t launch_gen_column(void *out, int elem_bytes, int64_t row0, int64_t n, uint64_t seed, uint64_t col_id,
                             int64_t lo, int64_t hi, int64_t mul, int64_t add, hipStream_t s);
// frame-of-reference images of columns (vdl_image.hip; the rules: vdl_column_image.h): out3 = {min, max} as int64 ^ 2^63, then the
// decimal trailing zeros all values share with the first row (19: all equal); then e = (v - base) / scale into img (1, 2 or 4 bytes)
hipError_t launch_image_stats(const void *col, int elem_bytes, int64_t n, unsigned long long *out3, hipStream_t s);
hipError_t launch_image_encode(const void *col, int elem_bytes, int64_t n, int64_t base, int64_t scale, void *img, int img_bytes, hipStream_t s);
// the bit-packed image (vdl_column_image.h Packed) of a byte image: img::packed_dwords(n, bits) dwords at `out`
hipError_t launch_image_pack(const void *img, int img_bytes, int64_t n, int64_t emin, int bits, void *out, hipStream_t s);
// the step image (vdl_column_image.h Steps): `padded_groups` head words (project_step_groups(n)) and as many anchors behind them at
// `image`; out2[0] (zeroed by the caller) is raised when some step is not 0 or 1, out2[1] = v[0]
hipError_t launch_image_steps(const void *col, int elem_bytes, int64_t n, int64_t padded_groups, void *image, unsigned long long *out2, hipStream_t s);

// ---- per-operator kernels -----------------------------------------------------------------
// validity bitmaps: bit (i & 63) of word (i >> 6); nullptr = every slot holds a value.
hipError_t launch_binary(int op, Src a, Src b, int64_t *out, int64_t n, hipStream_t s);
// A tree of element-wise operators over up to kExprLeaves vectors of one length, in postfix order, evaluated in one
// pass (the general path fuses chains of single-use Binary statements into this instead of one kernel per operator).
constexpr int kExprLeaves = 12, kExprInstrs = 48, kExprDepth = 8;
// operators that exist only inside fused trees: the emitter's sugar (a >= b is printed as LogicalOr(Greater(a,b), Equals(b,a)),
// /root/reference/src/Vdl.hs:139-152) recognised back, one interpreted instruction instead of three
enum : int { X_GE = 32, X_NE = 33 };
struct ExprProg {
    int n_instr = 0, n_leaf = 0;
    Src leaf[kExprLeaves];
    signed char code[kExprInstrs] = {};      // >= 0: apply BinOp code to the two topmost values; < 0: push leaf (-code - 1)
};
hipError_t launch_expr(const ExprProg &prog, int64_t *out, int64_t n, hipStream_t s);
hipError_t launch_poison(void *p, size_t bytes, uint64_t seed, hipStream_t s);     // VDL_POISON=rand (debugging)
hipError_t launch_and_words(const uint64_t *a, const uint64_t *b, uint64_t *out, int64_t nwords, hipStream_t s);
// A filter predicate -- comparisons between stored vectors joined by LogicalAnd / LogicalOr -- evaluated straight into
// the selection bitmap: a comparison of 64 rows is one 64-bit mask (v_cmp writes it), the connectives work on masks.
// Postfix: code >= 0 pushes comparison #code, P_AND / P_OR combine the two topmost masks.
constexpr int kPredCmps = 16, kPredInstrs = 32, kPredDepth = 8;
enum : int { P_GT = 0, P_EQ = 1, P_GE = 2, P_NE = 3, P_AND = -1, P_OR = -2 };
struct PredProg {
    int n_instr = 0, n_cmp = 0;
    Src a[kPredCmps], b[kPredCmps];
    signed char op[kPredCmps] = {};
    signed char code[kPredInstrs] = {};
};
// out bit i = predicate(i) & valid bit i (valid null = every slot)
hipError_t launch_pred(const PredProg &prog, const uint64_t *valid, uint64_t *out, int64_t n, hipStream_t s);
// global fold record {value, first slot, count} <-> three words that merge across shards (reduce: 0 sum, 1 min, 2 max)
// Merge of the partial words gathered from all ranks (vdl_comm.cpp).  Layout: rank r's block is 2 * n_words int64 at
// g + r * 2 * n_words -- the words, then the words again with FoldChoose (VDL_REDUCE_FIRST) entries resolved to the value
// at that rank's own smallest row id.  SUM / MIN / MAX fold the first halves; FIRST takes the value of the rank holding
// the smallest global row id (0 when no rank has a row in the group).  Host and device use this one definition.
#if defined(__HIPCC__)
#define VDL_HD __host__ __device__
#else
#define VDL_HD
#endif
// (`stride`: int64 words per rank in `g`: 2 * n_words, plus whatever the caller keeps behind them -- the status word of the
// sharded fold route)
VDL_HD inline int64_t merge_word(const int64_t *g, int world, int64_t n_words, int op, int64_t i, int64_t stride) {
    if (op == 4 /* VDL_REDUCE_FIRST */) {
        int64_t best = INT64_MAX, val = 0;
        for (int r = 0; r < world; r++) {
            const int64_t id = g[(int64_t)r * stride + i];
            if (id < best) { best = id; val = g[(int64_t)r * stride + n_words + i]; }
        }
        return val;
    }
    int64_t acc = g[i];
    for (int r = 1; r < world; r++) {
        const int64_t x = g[(int64_t)r * stride + i];
        if (op == 2 /* MIN */) acc = x < acc ? x : acc;
        else if (op == 3 /* MAX */) acc = x > acc ? x : acc;
        else acc = (int64_t)((uint64_t)acc + (uint64_t)x);
    }
    return acc;
}
// The wide form (vdl_plan_set_wide_sums_sharded; DESIGN.md section 5.17 "Sharded runs"): a rank's block carries, BEHIND the status word,
// the high words of its raw words -- hi of word i at 2 * n_words + 1 + i, stride >= 3 * n_words + 1.  A word that merge_word adds is
// added as a (lo, hi) pair with carry, rank after rank (a fixed order: deterministic); a MIN, MAX or FIRST word is merged as above and
// its high word is the sign extension of the merged low word.  The value returned is merge_word's in every case.
VDL_HD inline int64_t merge_word_wide(const int64_t *g, int world, int64_t n_words, int op, int64_t i, int64_t stride, int64_t *hi_out) {
    if (op == 2 || op == 3 || op == 4) {
        const int64_t v = merge_word(g, world, n_words, op, i, stride);
        *hi_out = v >> 63;
        return v;
    }
    uint64_t lo = 0, hi = 0;
    for (int r = 0; r < world; r++) {
        const uint64_t xl = (uint64_t)g[(int64_t)r * stride + i], xh = (uint64_t)g[(int64_t)r * stride + 2 * n_words + 1 + i];
        lo += xl;
        hi += xh + (lo < xl ? 1u : 0u);
    }
    *hi_out = (int64_t)hi;
    return (int64_t)lo;
}
// Wide sums in the per-operator folds (vdl_plan_set_wide_sums_tail; DESIGN.md section 5.17 "The tail").  A term x is split as
// x = H * 2^32 + L, L = x & 0xffffffff, H = x >> 32; over at most 2^31 terms the plain sums SL of the L (in [0, 2^63)) and SH of the H
// (|SH| < 2^62) cannot wrap.  The exact sum SH * 2^32 + SL as a pair: lo = bits 0..63 -- the wrapped int64 sum of the terms, by
// construction --, hi = bits 64..127.
VDL_HD inline void wide_join_halves(int64_t sl, int64_t sh, int64_t *lo, int64_t *hi) {
    const uint64_t base = (uint64_t)sh << 32, l = base + (uint64_t)sl;
    *lo = (int64_t)l;
    *hi = (sh >> 32) + (l < base ? 1 : 0);
}
// ... from the wrapped sum itself and SH: SL = wrapped - (SH << 32) modulo 2^64, exactly, because SL < 2^63
VDL_HD inline void wide_join_low(int64_t wrapped, int64_t sh, int64_t *lo, int64_t *hi) {
    wide_join_halves((int64_t)((uint64_t)wrapped - ((uint64_t)sh << 32)), sh, lo, hi);
}
constexpr int64_t kWideFoldMaxEntries = (int64_t)1 << 31;      // entries one wide fold takes: beyond it SH could wrap
// The folds that take a high output (launch_fold_global, launch_fold_runs, launch_group_fold below) run the wide forms of their kernels
// for it (vdl_fold_wide.hip): one load per term, the wrapped sum and the sum of the high halves side by side, joined per result.
// What goes with them: sign: hi[i] = lo[i] >> 63.  fits: flag[0] (INT64_MAX before) = the first i < n holding a value (valid null = all
// do) with hi[i] != lo[i] >> 63; fits_record: flag[0] = 0 when the record's value does not fit.
hipError_t launch_wide_sign(const int64_t *lo, int64_t *hi, int64_t n, hipStream_t s);
hipError_t launch_wide_fits(const int64_t *lo, const int64_t *hi, const uint64_t *valid, int64_t n, int64_t *flag, hipStream_t s);
hipError_t launch_wide_fits_record(const int64_t *rec, const int64_t *hi, int64_t *flag, hipStream_t s);
// gathered: `stride` words per rank = n_words raw, n_words resolved, then (stride > 2 * n_words) the rank's status word.
// status_out (may be null; needs that word): [0] = the first non-zero status over the ranks (0 = every rank's local phase
// succeeded), [1] = that rank.
// OR of the ranks' semi-join sets: gathered holds, per rank, `words` set words then ONE word = the rows of the set's source table on
// that rank; out = the union, with the bits at and beyond the table's GLOBAL length (the sum of those words) cleared -- the Scatter
// the set stands for is that long, positions beyond it are dropped (Vlite.hs:1212-1222).
hipError_t launch_or_sets(const uint64_t *gathered, int world, int64_t words, uint64_t *out, hipStream_t s);
hipError_t launch_merge_words(const int64_t *gathered, int world, int64_t n_words, int64_t stride, const int32_t *ops, int64_t *out,
                              int64_t *status_out, hipStream_t s);
// the merge of a sharded batch (vdl_run_batch_sharded): rank blocks of block_words = the plans' segments one after the other, each
// [raw nw][resolved nw, only where the plan has a FIRST word][status]; seg (device) = {offset, nw, index of its first word in out} per plan,
// n plans, total_words = the sum of the nw; out = every plan's merged words one after the other, status_out = 2 words per plan
hipError_t launch_merge_words_batch(const int64_t *gathered, int world, int64_t block_words, const int64_t *seg, int n, int64_t total_words, const int32_t *ops,
                                    int64_t *out, int64_t *status_out, hipStream_t s);
// the wide merge (vdl_mscan_wide.hip): out / out_hi = merge_word_wide of every word, status_out as launch_merge_words; one lane per word
hipError_t launch_merge_words_wide(const int64_t *gathered, int world, int64_t n_words, int64_t stride, const int32_t *ops, int64_t *out,
                                   int64_t *out_hi, int64_t *status_out, hipStream_t s);
hipError_t launch_fold_words(const int64_t *rec, int reduce, int64_t row0, int64_t *out, hipStream_t s);
hipError_t launch_fold_record(const int64_t *words, int64_t *rec, hipStream_t s);
// Gather out of a sparse vector without densifying it: counts[w] = popcount of bitmap word w (the caller turns them into
// exclusive prefix sums = wrank), then out[i] = entries[wrank[p/64] + popcount(word below bit p)] for p = pos[i] selected.
hipError_t launch_word_counts(const uint64_t *bitmap, int64_t nwords, int64_t *counts, hipStream_t s);
hipError_t launch_gather_ranked(const int64_t *entries, const uint64_t *bitmap, const int64_t *wrank, int64_t nsrc, Src pos, const uint64_t *vpos,
                                int64_t n, int64_t *out, uint64_t *vout, hipStream_t s);
// A first-level filter evaluated straight off its columns: bit i = every column's value lies in one of its intervals
struct FilterArgs {
    int ncol = 0, never = 0;
    Src col[kMaxFilterCols];
    int nint[kMaxFilterCols] = {};
    int64_t lo[kMaxFilterCols][kMaxFilterIvs] = {}, hi[kMaxFilterCols][kMaxFilterIvs] = {};
};
hipError_t launch_filter_columns(const FilterArgs &a, uint64_t *out, int64_t n, hipStream_t s);
// FoldSelect with unit-length runs: out bitmap = (d != 0) & vd & vc
hipError_t launch_select_bitmap(Src d, const uint64_t *vd, const uint64_t *vc, uint64_t *out, int64_t n, hipStream_t s);
// The three fold routes.  kind: 0 sum, 1 min, 2 max, 3 count, 4 choose (first value).  Each has ONE launcher for its plain and its wide
// form: a high output that is not null asks for kind 0 only, selects the wide kernels (at most kWideFoldMaxEntries entries) and holds, on
// return, bits 64..127 of every exact sum whose bits 0..63 -- the same words as the plain form's -- are in the low output.
//
// Global (single-run) fold of `d` over slots valid in both bitmaps: result = fold_record_words(wide) words,
// result[0] = value, result[1] = first slot whose control is valid (or -1), result[2] = number of data folded, and with result_hi
// result[3] = the value's high word (0 when nothing was folded), which is in result_hi[0] as well, for the readers that take a vector's
// high words as a buffer of their own.  scratch: fold_global_scratch_words(wide) int64.
int64_t fold_record_words(bool wide);
int64_t fold_global_scratch_words(bool wide);
hipError_t launch_fold_global(int kind, Src d, const uint64_t *vd, const uint64_t *vc, int64_t n, int64_t *scratch, int64_t *result, hipStream_t s,
                              int64_t *result_hi = nullptr);
// element-wise op on two one-hot (fold result) vectors: valid iff both valid and same slot
hipError_t launch_onehot_binary(int op, const int64_t *a, const int64_t *b, int64_t *out, hipStream_t s);
// broadcast-constant operand: b_is_const selects (a op k) / (k op a)
hipError_t launch_onehot_const(int op, const int64_t *a, int64_t k, int const_left, int64_t *out, hipStream_t s);
// one-hot -> dense n-slot vector (values + bitmap)
hipError_t launch_onehot_dense(const int64_t *oh, int64_t *out, uint64_t *valid, int64_t n, hipStream_t s);

// MaterializeCompact: out[rank(i)] = v[i] for valid i, slot order kept.
// block_counts: ceil(n / compact_tile()) int64; returns total in block_counts[nblocks] (device).
int64_t compact_tile();
hipError_t launch_compact_count(const uint64_t *valid, int64_t n, int64_t *block_counts, hipStream_t s);
hipError_t launch_compact_scan(int64_t *block_counts, int64_t nblocks, hipStream_t s, int64_t *host_total = nullptr);
// k words of device memory into pinned host memory and then `seq` into the pinned flag word, with system-scope stores (the host polls)
hipError_t launch_post_words(const int64_t *src, int64_t k, int64_t *pinned_dst, int64_t *pinned_flag, int64_t seq, hipStream_t s);   // exclusive scan in place, total at [nblocks]
hipError_t launch_compact_offsets(const uint64_t *valid, int64_t n, int64_t *block_counts, hipStream_t s, int64_t *host_total = nullptr);   // host_total: pinned host word that also receives the total   // count + scan (one launch for small n)
hipError_t launch_compact_write(Src v, const uint64_t *valid, int64_t n, const int64_t *block_offsets, int64_t *out, hipStream_t s, int64_t *out_pos = nullptr /* also: the slot number of every packed entry */);

// Gather / Scatter / Partition / segmented folds
hipError_t launch_gather(Src src, const uint64_t *vsrc, int64_t nsrc, Src pos, const uint64_t *vpos, int64_t n,
                         int64_t *out, uint64_t *vout, hipStream_t s);
hipError_t launch_scatter(Src src, const uint64_t *vsrc, Src pos, const uint64_t *vpos, int64_t n, int64_t nout,
                          int64_t *out, uint64_t *vout /* pre-zeroed; null = not wanted */, hipStream_t s);
hipError_t launch_fill_words(uint64_t *p, uint64_t v, int64_t nwords, hipStream_t s);
// FoldSelect (unit runs) straight over Gather(src, pos): out bit i = vc[i] & (src[pos[i]] exists and != 0); the gathered vector is never stored
hipError_t launch_select_gather(Src src, const uint64_t *vsrc, int64_t nsrc, Src pos, const uint64_t *vpos, const uint64_t *vc, uint64_t *out,
                                int64_t n, hipStream_t s);
// bitmap[idx[k]] = 1 for k < m (bitmap pre-zeroed; idx ascending, so neighbours often share a word)
hipError_t launch_set_bits(const int64_t *idx, int64_t m, uint64_t *bitmap, hipStream_t s, int64_t nbits = INT64_MAX /* entries outside [0, nbits) set nothing */);

// FoldSelect over general runs (vdl_engine.cpp: fold_select_runs): head flags of the runs of `ctl` (m entries, all valid),
// then the sort key 2 * run + (entry not selected) and the bitmap of selected entries
hipError_t launch_run_heads(const int64_t *ctl, int64_t m, int64_t *flags, int64_t *flags_copy, hipStream_t s);
hipError_t launch_fsel_keys(const int64_t *excl_heads, const int64_t *flags, const int64_t *d, const uint64_t *vd, int64_t m,
                            int64_t *keys, uint64_t *selected, hipStream_t s);

// device-wide exclusive prefix sum (in place); sums = prefix_sum_blocks(n) + 1 int64 of scratch
int64_t prefix_sum_blocks(int64_t n);
hipError_t launch_prefix_sum(int64_t *x, int64_t n, int64_t *sums, hipStream_t s);

// Partition with pivots RangeC pmin pcount 1 (bucket = clamp(data - pmin, 0, pcount)); see vdl_partition.hip
int64_t partition_tiles(int64_t n);
int partition_passes(int64_t pcount);
// flag[0] (pre-zeroed by the caller) becomes 1 when d[i] > d[i+1] somewhere: the data is not in non-decreasing order
hipError_t launch_sorted_check(Src d, int64_t n, int64_t *flag, hipStream_t s);
// The same pass also leaves the RUN HEADS of the (fully valid) vector: heads bit i = (i == 0 or d[i] != d[i-1]) -- what the folds of
// the GROUP BY that this Partition serves need when the data turns out to be in order (their control vector is then this
// vector, unmoved).  flag[0] / flag[1] as above (pre-set to 0 / INT64_MIN).
hipError_t launch_sorted_heads(Src d, int64_t n, uint64_t *heads /* (n + 63) / 64 words */, int64_t *flag /* 3 words: descends, largest, smallest */, hipStream_t s);
// ... with the heads counted per compaction tile, the counts scanned in place (counts[nb] = total, then {descends, largest, smallest}) and
// those four words posted into pinned host memory behind `seq` -- one launch.  `state`: words owned by the caller between launches,
// once prepared by launch_sorted_state_init.  Serves int64 vectors at 16-byte aligned addresses (sorted_heads_counted_serves).
bool sorted_heads_counted_serves(Src d, int64_t n);
int64_t sorted_heads_state_words();
int64_t sorted_heads_counts_words(int64_t n);
hipError_t launch_sorted_state_init(int64_t *state /* sorted_heads_state_words() */, hipStream_t s);
hipError_t launch_sorted_heads_counted(const int64_t *d, int64_t n, uint64_t *heads, int64_t *counts /* sorted_heads_counts_words(n) */, int64_t *state, int64_t *pinned_dst /* 4 words */,
                                       int64_t *pinned_flag, int64_t seq, hipStream_t s);
// Every fold of one GROUP BY in one launch, results PACKED (one per run, in run order): fold j reduces data[j] over the runs whose
// heads are given (m entries, all holding a value; entry 0 is a head) and writes out[j][g] for the g-th run.  offsets = exclusive
// prefix of the head counts per compaction tile (launch_compact_count + launch_compact_scan over `heads`).  kind: 0 sum, 1 min,
// 2 max, 3 count, 4 choose (first value).  out[j] of kinds 0-3 must hold the reduction's identity (0 / INT64_MAX / INT64_MIN / 0).
// out_hi (null: the plain kernel): a.nfold pointers, out_hi[j] = where the high words of FoldSum member j go (pre-filled with zeros like
// out[j]; null for the members that are no wide sum), `groups` = the number of runs, i.e. of words behind each.
constexpr int kMaxGroupFolds = 16;
struct GroupFoldArgs {
    int nfold = 0;
    int kind[kMaxGroupFolds] = {};
    Src data[kMaxGroupFolds];
    int64_t *out[kMaxGroupFolds] = {};
};
hipError_t launch_group_fold(const GroupFoldArgs &a, const uint64_t *heads, int64_t m, const int64_t *offsets, hipStream_t s, int64_t *const *out_hi = nullptr,
                             int64_t groups = 0);
size_t partition_scratch_bytes(int64_t n, int64_t pcount);
hipError_t launch_partition(Src data, const uint64_t *valid, int64_t n, int64_t pmin, int64_t pcount, void *scratch /* partition_scratch_bytes(n, pcount) */,
                            uint64_t *keys_a, int64_t *slots_a, uint64_t *keys_b, int64_t *slots_b,
                            int64_t *n_valid_dev, int64_t *pos_out, hipStream_t s, int64_t max_bucket = -1 /* largest bucket known to occur */,
                            int64_t *order_out = nullptr /* instead of pos_out: the slots in rank order (order[pos[slot]] = slot), stored sequentially */,
                            int64_t *sorted_keys_out = nullptr /* with order_out: bucket + pmin in rank order (= the keys, when all lie inside the pivots) */);

// Fold over a general control vector: launch_fold_heads leaves the run heads (first slot of every run, EPS control slots skipped) and
// the per-word lookup, launch_fold_runs folds `d` over them -- several folds share one control vector's heads.  out[head] = the run's
// result, vout (pre-zeroed) = the heads of runs that folded something, out_hi[head] = the high word of out[head].
// heads: nwords uint64; wordhd: nwords + maxscan_blocks(nwords) int64
int64_t maxscan_blocks(int64_t n);
hipError_t launch_fold_heads(Src ctl, const uint64_t *vc, int64_t n, uint64_t *heads, int64_t *wordhd, hipStream_t s);
hipError_t launch_fold_runs(int kind, Src d, const uint64_t *vd, const uint64_t *vc, const uint64_t *heads, const int64_t *wordhd, int64_t n,
                            int64_t *out, uint64_t *vout, hipStream_t s, int64_t *out_hi = nullptr);

// ---- row exchange for sharded Partition (see vdl_partition.hip) ------------------------------------
constexpr int kMaxExSources = 62;
constexpr int kMaxExWorld = 128;          // ranks in one exchange (vdl_exchange_begin)
// CrossProductOuter / Inner (Vdl.hs:412-416; Vlite.hs:278-289): positions i / k and i % k over n = m * k slots
hipError_t launch_cross(int64_t n, int64_t k, int inner, int64_t *out, hipStream_t s);
// Like (Vdl.hs:444-447): out[i] = string at byte offset data[i] of `heap` matches the SQL LIKE pattern
struct LikePattern { unsigned char p[256]; int len; };
hipError_t launch_like(Src data, const uint64_t *vdata, int64_t n, Src heap, const uint64_t *vheap, int64_t heap_n, const LikePattern &pat,
                       int64_t *out, hipStream_t s);
constexpr int kExBins = 4096;              // at most this many equal, power-of-two-wide slices of the pivots' domain in which a rank counts its keys (hist: kExBins + 1 words, the last = keys outside the pivots; pre-zeroed)
hipError_t launch_ex_hist(Src key, const uint64_t *vkey, int64_t n, int64_t pmin, int64_t pcount, int64_t *hist, hipStream_t s);
// Routing of a sharded Partition's rows (vdl_partition.hip "routing"): where every row goes, the rows per destination, and the packed send buffer.
struct ExRoute {
    Src key; const uint64_t *vkey = nullptr;
    int64_t n = 0, pmin = 0, pcount = 0;                    // pcount <= 0: every row with a key takes part and goes to destination 0
    int world = 1, shift = 0;                               // shift = ex_route_shift(pcount): the width of a slice of the domain
    const int32_t *owner = nullptr;                         // slice of the domain -> rank (kExBins entries; the balanced cut of vdl_run_sharded), or null: the domain cut evenly
};
constexpr int kExPackCols = 8;             // columns one launch of the pack writes
struct ExCols {
    int ncol = 0, first = 0;               // columns first .. first + ncol - 1 of the send buffer
    Src src[kExPackCols];
    int mask_at = -1, nvalid = 0;          // mask_at >= 0: this launch also writes the mask column there: bit v = valid[v] holds a value in the row
    const uint64_t *valid[kMaxExSources] = {};
};
int64_t ex_route_tiles(int64_t n);
int ex_route_shift(int64_t pcount);
hipError_t launch_ex_route(const ExRoute &R, int64_t *tileoff /* world x ex_route_tiles(n) */, int64_t *counts /* 2 world + 1, pre-zeroed: rows per destination, keys outside the pivots, where each destination's rows begin */, hipStream_t s);
hipError_t launch_ex_pack_all(const ExRoute &R, const ExCols &C, const int64_t *tileoff, const int64_t *counts /* as launch_ex_route left them */, int64_t n_send, int64_t *out, hipStream_t s);
hipError_t launch_ex_unmask(const int64_t *mask, int64_t n, int j, uint64_t *valid, hipStream_t s);

// ---- ORDER BY / LIMIT over result columns in HBM (vdl_order.hip) ---------------
// A key's order word is u = key ^ flip: kOrdFlipAsc makes signed ascending = unsigned ascending, kOrdFlipDesc also complements.
constexpr uint64_t kOrdFlipAsc = 0x8000000000000000ull, kOrdFlipDesc = 0x7fffffffffffffffull;
constexpr int kOrdMaxKeys = 8;
constexpr int kOrdDigitBits = 11, kOrdBins = 1 << kOrdDigitBits;      // digit of a selection round
constexpr int kOrdTopMax = 4096;                                       // limits up to here take the selection, larger ones (and 0) the full sort
constexpr int kOrdBoundary = 4096;                                     // C: the selection stops once the boundary bin holds at most this many rows
constexpr int kOrdStateHead = 8, kOrdStateWords = kOrdStateHead + kOrdBins;   // state: [0] max(~u) [1] max(u) [2] bin [3] rows below it [4] rows in it | histogram
constexpr int kOrdGatherMax = 24;                                      // outputs one gather launch writes
struct OrdKeys { int n = 0; const int64_t *key[kOrdMaxKeys] = {}; uint64_t flip[kOrdMaxKeys] = {}; };
struct OrdGather { int n = 0; const int64_t *src[kOrdGatherMax] = {}; int64_t *dst[kOrdGatherMax] = {}; };
// min / max of u over the rows of `active` (null = all m): state[0] = max(~u), state[1] = max(u); both words zero before the launch
hipError_t launch_order_minmax(const int64_t *key, uint64_t flip, const uint64_t *active, int64_t m, uint64_t *state, hipStream_t s);
// one selection round over the rows of `active` whose bits [hi_shift, 64) equal prefix (hi_shift = 64: every row): histogram of bits
// [shift, shift + width), then state[2..4] = {bin holding the need-th such row, rows in the bins below it, rows in it}; histogram (zero before) zero after
hipError_t launch_order_round(const int64_t *key, uint64_t flip, const uint64_t *active, int64_t m, int hi_shift, uint64_t prefix, int shift, int width,
                              int64_t need, uint64_t *state, hipStream_t s);
// rows of active_in (null = all) with bits [hi_shift, 64) == prefix -> active_out, < prefix -> OR-ed into below ((m + 63) / 64 words each)
hipError_t launch_order_close(const int64_t *key, uint64_t flip, const uint64_t *active_in, int64_t m, int hi_shift, uint64_t prefix, uint64_t *active_out,
                              uint64_t *below, hipStream_t s);
// n <= kOrdTopMax + kOrdBoundary candidate rows `pos`: index_out[r] = the candidate of rank r < keep under (keys, position); staged: K.n * n words
hipError_t launch_order_rank(const OrdKeys &K, const int64_t *pos, int64_t n, int64_t keep, uint64_t *staged, int64_t *index_out, hipStream_t s);
hipError_t launch_order_gather(const OrdGather &G, const int64_t *index, int64_t n, hipStream_t s);      // dst[o][i] = src[o][index[i]], i < n
// ---- the merged order of a sharded run (DESIGN.md section 5.9 "sharded runs"): every rank's first rows, gathered, are `world` sorted runs ----
// Candidate block of one rank: column c < B.n of the n chosen rows, column-major -- out[c * n + i] = src[c][index[i]] ^ flip[c] (index
// null = the rows as they stand).  The K order words (flip = the key's) stand first, every output's value (flip 0) behind them.
constexpr int kOrdBlockCols = kOrdMaxKeys + kOrdGatherMax;
struct OrdBlock { int n = 0; const int64_t *src[kOrdBlockCols] = {}; uint64_t flip[kOrdBlockCols] = {}; };
hipError_t launch_order_block(const OrdBlock &B, const int64_t *index, int64_t n, int64_t *out, hipStream_t s);
// The gathered runs: run r is candidates [off[r], off[r + 1]) of N = off[world], its order words at w[k * N + j], k < nk, ascending
// under (u_1, .., u_K) with ties in the run's own order.
struct OrdRuns { int world = 0, nk = 0; int64_t off[kMaxExWorld + 1] = {}; };
// The rule, shared by the kernel and vdl_order_merge_host: candidate j of run r takes the place
//     (j - off[r]) + sum over runs q < r of |{x in q : x <= j}| + sum over runs q > r of |{x in q : x < j}|
// -- each count one binary search under the full comparator -- which is its rank under (u_1, .., u_K, run, place in the run): the
// order of section 5.9 over the ranks' results one after the other.  Places are a permutation of 0 .. N-1.
VDL_HD inline int64_t ord_merge_place(const OrdRuns &R, const uint64_t *w, int64_t j) {
    const int64_t N = R.off[R.world];
    uint64_t mine[kOrdMaxKeys];
#pragma unroll
    for (int k = 0; k < kOrdMaxKeys; k++) mine[k] = k < R.nk ? w[(int64_t)k * N + j] : 0;
    int r = 0;
    int64_t first = 0;                                                  // (off[] is only ever indexed by the loop counter: it stays in the kernel's arguments)
    for (int q = 1; q < R.world; q++)
        if (j >= R.off[q]) { r = q; first = R.off[q]; }                 // the last run that begins at or before j: the one that holds it
    int64_t place = j - first;
    for (int q = 0; q < R.world; q++) {
        int64_t lo = R.off[q], hi = q == r ? lo : R.off[q + 1];
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            bool less = false, decided = false;
#pragma unroll
            for (int k = 0; k < kOrdMaxKeys; k++) {
                if (k < R.nk && !decided) {
                    const uint64_t o = w[(int64_t)k * N + mid];
                    less = o < mine[k];
                    decided = o != mine[k];
                }
            }
            if (decided ? less : q < r) lo = mid + 1; else hi = mid;
        }
        place += lo - R.off[q];
    }
    return place;
}
// one lane per candidate: a candidate whose place is below `keep` writes its row of every output, dst[o][place] = src[o][j]
hipError_t launch_order_merge(const OrdRuns &R, const OrdGather &G, const uint64_t *w, int64_t keep, hipStream_t s);
// full order: out[i] = u(key[perm[i]]) - umin (perm null = identity) whole (half 0) / low 32 bits (1) / high 32 bits (2); out[i] = perm[order[i]]
hipError_t launch_order_sortkey(const int64_t *key, uint64_t flip, const int64_t *perm, int64_t m, uint64_t umin, int half, int64_t *out, hipStream_t s);
hipError_t launch_order_compose(const int64_t *perm, const int64_t *order, int64_t m, int64_t *out, hipStream_t s);

// ---- collation index of a string heap: heap offset -> dense rank in text order (vdl_collate.hip) ---------------
constexpr int kCollateMaxBytes = 256;                                  // the longest string an index is built for
// the table has one int32 per 2^gshift heap bytes (gshift = 3 for heaps whose strings all start at multiples of 8): 0 = the byte is NUL
// (the empty string), -1 = no string starts here, otherwise the rank of the string that does (1 = the smallest non-empty string)
inline int64_t collate_table_slots(int64_t heap_n, int gshift) { return (heap_n + ((int64_t)1 << gshift) - 1) >> gshift; }
hipError_t launch_collate_mark(const int8_t *heap, int64_t n, uint64_t *starts /* (n + 63) / 64 words */, hipStream_t s);
// off: the d start offsets, ascending.  state (two words, zero before): [0] the longest string in bytes, [1] the OR of the offsets
hipError_t launch_collate_lengths(const int8_t *heap, int64_t n, const int64_t *off, int64_t d, uint64_t *state, hipStream_t s);
// words[j * d + i] = bytes [8j, 8j + 8) of string i, big-endian, zero from its NUL on; nwords * 8 >= the longest string
hipError_t launch_collate_words(const int8_t *heap, int64_t n, const int64_t *off, int64_t d, int nwords, uint64_t *words, hipStream_t s);
// perm: the strings in text order (null = as they stand).  flags: d + 1 words; an exclusive prefix sum over them leaves the rank of
// sorted place r in flags[r + 1], and so the number of distinct strings in flags[d]
hipError_t launch_collate_heads(const uint64_t *words, const int64_t *perm, int64_t d, int nwords, int64_t *flags, hipStream_t s);
hipError_t launch_collate_table(const int8_t *heap, int64_t n, int gshift, const int64_t *off, const int64_t *perm, const int64_t *ranks /* the scanned flags */,
                                int64_t d, int32_t *table /* collate_table_slots(n, gshift) */, hipStream_t s);
// the order step's text key: ranks[i] of the string code[i] names, -1 for a code that names none; state (two words, zero before): [0] = such rows, [1] = ~(the first of them)
hipError_t launch_order_textkey(const int64_t *code, int64_t m, const int8_t *heap, int64_t n, const int32_t *table, int gshift, int64_t *ranks, uint64_t *state,
                                hipStream_t s);


// ---- internal: what launch_fold_global / launch_fold_runs / launch_group_fold (vdl_ops.hip) call for a high output (vdl_fold_wide.hip,
// a translation unit of its own: vdl_ops.o holds no wide instantiation).  Nobody else calls these. ----
hipError_t launch_wide_fold_global(Src d, const uint64_t *vd, const uint64_t *vc, int64_t n, int64_t *scratch, int64_t *result, int64_t *result_hi, hipStream_t s);
hipError_t launch_wide_fold_runs(Src d, const uint64_t *vd, const uint64_t *vc, const uint64_t *heads, const int64_t *wordhd, int64_t n, int64_t *out, int64_t *out_hi,
                                 uint64_t *vout, hipStream_t s);
hipError_t launch_wide_group_fold(const GroupFoldArgs &a, int64_t *const *out_hi, int64_t groups, const uint64_t *heads, int64_t m, const int64_t *offsets, hipStream_t s);

}  // namespace vdl
