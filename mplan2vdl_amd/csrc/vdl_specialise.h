// vdl_specialise.h -- run-time specialisation of the fused aggregate scans (vdl_specialise.cpp): what vdl_engine.cpp calls.
// Which forms exist is ScanForm (vdl_scan_form.h).
#pragma once
#include "vdl_engine_internal.h"

namespace vdl {
namespace eng {

// at bind time: scan s of the bound plan in its specialised kernel (VDL_JIT_LATE: in that form, where the scan has it).  On success the
// kernel, its grid and `kname` replace the precompiled variant's; on failure the variant stays and the note says why
bool specialise_scan(vdl_ctx *c, vdl_plan *p, size_t s, bool grouped, std::string *kname);
// vdl_plan_set_jit(plan, 2), at the first run: every specialised scan in the candidate forms, timed; the quickest stays
void tune_specialised(vdl_ctx *c, vdl_plan *p, int64_t *dev_words);
// vdl_plan_scan_traffic: HBM bytes one launch of the dominant scan moves; detail: "column=bytes ..."
int64_t scan_bytes_moved(vdl_ctx *c, vdl_plan *p, std::string &detail);
// vdl_plan_jit_check of a fused plan: every scan's specialised kernel built (not loaded) against the columns registered now
void jit_check_scans(vdl_ctx *c, vdl_plan *p);
// one build of specialised code for `role` of the plan ("scan 0", "front", "dim3") and where its code came from; what the note says
// about the role's builds so far: "from cache: 2 of 3 builds of scan 0; "
void count_build(vdl_plan *p, const std::string &role, jit::Origin from);
std::string builds_text(const vdl_plan *p, const std::string &role);


// ---- batched runs (vdl_run_batch, vdl_batch_jit_check): plans that differ in their literals alone share one pass over the columns ----
// why a plan cannot share a scan with any other, in the words its batch note carries; "" = it may
// (grouped_on: vdl_set_batch_grouped -- a plan whose one scan is a grouped scan over table columns may share a grouped batch)
// (joins_on: vdl_set_batch_joins -- the one scan may have derived columns and a prelude: a join batch)
std::string batch_alone_reason(const vdl_plan *p, bool grouped_on = false, bool joins_on = false);
// a plan's one scan as a batch sees it: its eager binding (made here, the plan's own bound state is not touched) and the two keys that
// decide which plans go together -- the columns (addresses, widths, images, rows, row offset) and the shape of the generated code
// under run-time bounds (jit::entry_name: the descriptor's text with the ranges' shapes in place of their values)
struct BatchMember {
    vdl_plan *p = nullptr;
    int index = 0;                              // the plan's place in the caller's list
    MScanCols cols;
    std::shared_ptr<MScanDesc> desc;
    ScanLaunch cfg;
    bool grouped = false;                       // the scan is the plan's one grouped scan
    bool derived = false;                       // the scan has derived columns: a join batch (vdl_set_batch_joins)
    int replicas_alone = 1;                     // ... and has that many table replicas when the plan runs alone
    std::string cols_key, shape_key;
    // join batches: the canonical text of the prelude items the scan refers to (equal text: equal lookup tables, built once per batch)
    // and the leaf bounds of its conditions (a condition is computed once per row, from slot 0's descriptor)
    std::string prelude_key, form_key;
};
void batch_bind(vdl_ctx *c, vdl_plan *p, BatchMember &m);
// join batches: [k] = prelude item k is left open for the batch -- every row selected, nothing scanned -- because the plan's own scan
// applies its filters with the same bounds (vdl_specialise.cpp says when)
std::vector<char> batch_open_items(const vdl_plan *p);
// the widest batch for scans of this many aggregates: kMaxBatch, or what kMaxBatchWords accumulators per lane allow
int batch_cap(int nagg);
// ... and under VDL_BATCH_WIDTH=k, which caps the width of any batch
int batch_cap_asked(int nagg);
// grouped batches: the widest batch (kMaxBatchGrouped .. 2, under VDL_BATCH_WIDTH) whose 2^K - 1 class tables leave the scan enough
// replicas in 64 KiB of LDS, 0 = not even two plans fit; the replicas a batch of k plans runs with (0: it does not fit)
int batch_group_cap(const MScanDesc &d, int replicas_alone);
int batch_group_replicas(const MScanDesc &d, int k);
// one batch of 2 .. batch_cap plans of one group: its kernel built (kept with the context, per shape, columns and width: a second batch
// of the same kind compiles and loads nothing) and, unless check_only, launched on the context's stream between the two events (may
// be null) -- slot q's 1 + nagg words end up at outs[q].  Returns the kernel's name, "k_mscan_specialised<...,batch<K>,rtb>".
// tune: the candidate forms timed first (eager at 2, 3, 4 row pairs per lane, every column packed at 2, 4 per slice; VDL_JIT_PIN pins)
// A grouped batch (ms[0]->grouped): the eager form only (tuned: at 2, 3, 4), slot q's pcount * (1 + nagg) + 1 words at outs[q].
// code_bytes: the size of the kernel's code object.
std::string batch_scan(vdl_ctx *c, const std::vector<BatchMember *> &ms, bool tune, bool check_only, int64_t *const *outs, hipEvent_t ev0, hipEvent_t ev1,
                       size_t *code_bytes = nullptr);

}  // namespace eng
}  // namespace vdl
