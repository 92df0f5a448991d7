// vdl_scan_form.h -- the forms a run-time-specialised aggregate scan comes in (vdl_specialise.cpp builds and times them).
// Host only: the device code knows a form by its kernel arguments (MsArgs: stages, lazy, queued, packed), not by this type.
#pragma once
#include "vdl_scan_desc.h"

namespace vdl {

struct ScanForm {
    // EAGER: every column with the tile
    // STAGED: `eager_filters` filter columns with the tile, the other columns late, for the rows still in (MsArgs::stages)
    // QUEUE: one filter column with the tile, the rows still in queued per wave and finished 64 at a time
    // PACKED: the filter columns from their bit-packed images and the aggregate inputs late from their byte images, or (`every_column`)
    //         every column from its packed image and nothing late; over a binding of its own
    enum Kind { EAGER, STAGED, QUEUE, PACKED } kind = EAGER;
    static constexpr int kAllFilters = kMaxVCols;       // STAGED: only aggregate inputs and the sources of derived columns read late
    int eager_filters = 0;          // STAGED: 1, 2 or kAllFilters
    bool every_column = false;      // PACKED
    int u = 0;                      // row pairs per lane (PACKED: per slice); 0 = the launch configuration's (PACKED: VDL_JIT_U, else 2)

    // The numbers of VDL_JIT_LATE and of "late=" in VDL_JIT_PIN, which tests, tools and profiles speak:
    //   0 = everything with the tile   1, 2 = that many filter columns eager   3 = the queue form
    //   4 = every filter column eager  5 = filters bit-packed + inputs late    6 = every column bit-packed
    static ScanForm from_code(int code, int u = 0) {
        ScanForm f;
        f.u = u;
        f.kind = code <= 0 ? EAGER : code == 3 ? QUEUE : code >= 5 ? PACKED : STAGED;
        if (f.kind == STAGED) f.eager_filters = code == 4 ? kAllFilters : code;
        f.every_column = code >= 6;
        return f;
    }
    // what kernel names, the tuner's `tried` list and profiles call the form
    const char *suffix() const {
        return kind == EAGER ? "" : kind == QUEUE ? ",queue" : kind == PACKED ? (every_column ? ",packed" : ",packed,late")
             : eager_filters == kAllFilters ? ",lateall" : eager_filters > 1 ? ",late2" : ",late";
    }
};

}  // namespace vdl
