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

}  // namespace eng
}  // namespace vdl
