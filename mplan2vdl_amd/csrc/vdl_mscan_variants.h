// vdl_mscan_variants.h -- the precompiled instantiations of the multi-aggregate fused scans, as one list: vdl_mscan.hip makes its
// table of k_mscan from it, vdl_mscan_wide.hip the table of the wide-sums build (k_mscan_wide) -- entry by entry the same shapes, so
// that a ScanLaunch::variant names the same shape in both.
// MS(NC, U, VEC, NT, GROUPED): scans over table columns; MSJ(...): scans with derived columns (FK lookups: fused join scans)
#pragma once
#define VDL_MS_VARIANTS(MS, MSJ) \
    MS(4, 6, true, true, false),  MS(8, 4, true, true, false), \
    MS(4, 4, false, false, false), MS(8, 4, false, false, false), \
    MS(4, 6, true, true, true),   MS(8, 2, true, true, true),   MS(8, 4, true, true, true), \
    MS(4, 4, false, false, true),  MS(8, 4, false, false, true), \
    MS(8, 1, true, true, true),   MS(8, 3, true, true, true),      /* VDL_GROUP_U sweeps (tools/q1_ab.sh) */ \
    MSJ(8, 4, true, true, false), MSJ(8, 4, false, false, false), \
    MSJ(8, 2, true, true, true),  MSJ(8, 2, false, false, true), \
    MSJ(12, 2, true, true, false), MSJ(12, 2, false, false, false), \
    MSJ(12, 1, true, true, true),  MSJ(12, 1, false, false, true)      /* (U = 2 spills 720 B/lane in the grouped form) */
