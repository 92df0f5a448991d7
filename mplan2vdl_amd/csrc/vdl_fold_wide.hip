// vdl_fold_wide.hip -- wide sums in the per-operator folds for gfx950 (vdl_plan_set_wide_sums_tail; DESIGN.md section 5.17 "The tail").
// A translation unit of its own: vdl_ops.o holds no wide instantiation.
//
// The split.  Every int64 term is x = H * 2^32 + L with L = x & 0xffffffff and H = x >> 32 (arithmetic).  Over at most 2^31 entries the
// plain int64 sum SH of the H never wraps (|SH| < 2^62), so the exact sum S = SH * 2^32 + SL needs no carry chain and no returning
// atomic while it is accumulated.  The low word of S is the wrapped int64 sum of the terms -- what the plain folds deliver -- and SL,
// which lies in [0, 2^63), is wrapped - (SH << 32) modulo 2^64 exactly.  So a wide fold carries TWO ordinary sums per result, both
// derived from ONE load of the term: the wrapped sum of x and the sum of x >> 32; wide_join_low makes bits 64..127 once per result.
// Order-independent and deterministic, because both sums are.
//
// k_wide_seg_fold and k_wide_fold_global_finish are the WIDE = true forms of the bodies in vdl_fold_body.h, k_wide_fold_global and
// k_wide_group_fold those of the texts in vdl_fold_global.inc and vdl_group_fold.inc; the WIDE = false forms are the kernels of vdl_ops.hip.
// One text each, so the same layouts, chunks, segments, carried runs and atomics.
//
// Nobody calls the three fold launchers here by name but launch_fold_global, launch_fold_runs and launch_group_fold of vdl_ops.hip, for a
// call that brings a high output (vdl_kernels.h: one interface per route for both forms).  Each returns FINISHED high words: the finish
// step of the global fold joins, the segmented fold joins at the heads, the group fold runs k_wide_join over its packed results.
#include "vdl_device.h"
#include "vdl_fold_body.h"
#include "vdl_kernels.h"

namespace vdl {

// k_wide_group_fold's argument block: GroupFoldArgs and one high output per member, which the plain kernel's block does not carry
struct WideGroupFoldArgs {
    GroupFoldArgs g;
    int64_t *out_hi[kMaxGroupFolds] = {};
};

namespace {

constexpr int kWfBlock = 256;

// hi[i]: in = the sum of the high stream of result i, out = bits 64..127 of the exact sum whose bits 0..63 are lo[i]
__global__ __launch_bounds__(kWfBlock) void k_wide_join(const int64_t *__restrict__ lo, int64_t *__restrict__ hi, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kWfBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWfBlock) {
        int64_t l, h;
        wide_join_low(lo[i], hi[i], &l, &h);
        hi[i] = h;
    }
}

// hi[i] = the sign extension of lo[i]: the high word of a value that is no wide sum
__global__ __launch_bounds__(kWfBlock) void k_wide_sign(const int64_t *__restrict__ lo, int64_t *__restrict__ hi, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kWfBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWfBlock) hi[i] = lo[i] >> 63;
}

// The fits check: flag[0] (INT64_MAX before) = the first position i < n that holds a value (valid null = every one does) whose high
// word is not the sign extension of its low word.  One atomic per wave that found one.
__global__ __launch_bounds__(kWfBlock) void k_wide_fits(const int64_t *__restrict__ lo, const int64_t *__restrict__ hi, const uint64_t *__restrict__ valid, int64_t n,
                                                       int64_t *flag) {
    int64_t first = INT64_MAX;
    for (int64_t i = (int64_t)blockIdx.x * kWfBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWfBlock) {
        const bool held = !valid || ((valid[i >> 6] >> (i & 63)) & 1ull);
        if (held && hi[i] != (lo[i] >> 63) && i < first) first = i;
    }
    first = wave_reduce(first, R_MIN);
    if ((threadIdx.x & (kWave - 1)) == 0 && first != INT64_MAX) atomicMin((long long *)flag, (long long)first);
}
__global__ void k_wide_fits_record(const int64_t *rec, const int64_t *hi, int64_t *flag) {
    if (rec[2] > 0 && hi[0] != (rec[0] >> 63)) flag[0] = 0;
}

// ---- k_fold_global, FoldSum, wide: per-block partials {sum, first control slot, count, sum of the high halves}, then one block ----
__global__ __launch_bounds__(256) void k_wide_fold_global(Src d, const uint64_t *vd, const uint64_t *vc, int64_t n, int64_t *scratch) {
    constexpr bool WIDE = true;
    constexpr int kind = 0;
#include "vdl_fold_global.inc"
}
__global__ __launch_bounds__(256) void k_wide_fold_global_finish(const int64_t *scratch, int nblocks, int64_t *result, int64_t *result_hi) {
    fold_global_finish_body<true>(0, Src{}, scratch, nblocks, result, result_hi);
}

// ---- k_seg_fold, FoldSum, wide: out[head] = the wrapped sum of the run, out_hi[head] = the sum of its high halves (joined afterwards) ----
__global__ void k_wide_init_heads(const uint64_t *heads, int64_t nw, int64_t *out, int64_t *out_hi) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += stride) {
        uint64_t m = heads[w];
        while (m) { const int b = __ffsll((long long)m) - 1; out[(w << 6) + b] = 0; out_hi[(w << 6) + b] = 0; m &= m - 1; }
    }
}
// the join at the heads: out_hi[head] becomes bits 64..127 of the run's exact sum
__global__ void k_wide_join_heads(const uint64_t *heads, int64_t nw, const int64_t *out, int64_t *out_hi) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += stride) {
        uint64_t m = heads[w];
        while (m) {
            const int64_t i = (w << 6) + __ffsll((long long)m) - 1;
            int64_t l, h;
            wide_join_low(out[i], out_hi[i], &l, &h);
            out_hi[i] = h;
            m &= m - 1;
        }
    }
}
__global__ __launch_bounds__(256) void k_wide_seg_fold(Src d, const uint64_t *vd, const uint64_t *vc, const uint64_t *heads, const int64_t *wordhd, int64_t n,
                                                       int64_t *out, int64_t *out_hi, uint64_t *vout) {
    seg_fold_body<true>(0, d, vd, vc, heads, wordhd, n, out, out_hi, vout);
}

// ---- k_group_fold, wide: a FoldSum member with out_hi set leaves the sum of its high halves there (joined afterwards) ----
template <int NF>
__global__ __launch_bounds__(256) void k_wide_group_fold(WideGroupFoldArgs A, unsigned vec16, const uint64_t *heads, int64_t m, const int64_t *offsets) {
    constexpr bool WIDE = true;
    const GroupFoldArgs &a = A.g;
    int64_t *const *const out_hi = A.out_hi;
#include "vdl_group_fold.inc"
}

int wf_grid(int64_t n, int per_lane) { return grid_for(n, kWfBlock, per_lane); }

}  // namespace

hipError_t launch_wide_fold_global(Src d, const uint64_t *vd, const uint64_t *vc, int64_t n, int64_t *scratch, int64_t *result, int64_t *result_hi, hipStream_t s) {
    (void)hipGetLastError();
    const int grid = fold_global_grid(n);
    k_wide_fold_global<<<grid, 256, 0, s>>>(d, vd, vc, n, scratch);
    k_wide_fold_global_finish<<<1, 256, 0, s>>>(scratch, grid, result, result_hi);
    return launch_status();
}
hipError_t launch_wide_fold_runs(Src d, const uint64_t *vd, const uint64_t *vc, const uint64_t *heads, const int64_t *wordhd, int64_t n, int64_t *out, int64_t *out_hi,
                                 uint64_t *vout, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    const int64_t nw = (n + 63) >> 6;
    k_wide_init_heads<<<grid_for(nw, 256, 1), 256, 0, s>>>(heads, nw, out, out_hi);
    k_wide_seg_fold<<<seg_fold_grid(n), 256, 0, s>>>(d, vd, vc, heads, wordhd, n, out, out_hi, vout);
    k_wide_join_heads<<<grid_for(nw, 256, 1), 256, 0, s>>>(heads, nw, out, out_hi);
    return launch_status();
}
hipError_t launch_wide_group_fold(const GroupFoldArgs &g, int64_t *const *out_hi, int64_t groups, const uint64_t *heads, int64_t m, const int64_t *offsets, hipStream_t s) {
    (void)hipGetLastError();
    const int64_t nb = (m + compact_tile() - 1) / compact_tile();
    if (nb <= 0 || g.nfold <= 0) return hipSuccess;
    if (g.nfold > kMaxGroupFolds) return hipErrorInvalidValue;
    WideGroupFoldArgs a;
    a.g = g;
    for (int j = 0; j < g.nfold; j++) {
        if (out_hi[j] && g.kind[j] != 0) return hipErrorInvalidValue;
        a.out_hi[j] = out_hi[j];
    }
    const unsigned vec16 = group_fold_vec16(g);
    if (g.nfold <= 2) k_wide_group_fold<2><<<(int)(nb * kGroupSplit), 256, 0, s>>>(a, vec16, heads, m, offsets);
    else k_wide_group_fold<4><<<(int)(nb * kGroupSplit), 256, 0, s>>>(a, vec16, heads, m, offsets);
    for (int j = 0; j < g.nfold && groups > 0; j++)           // the join at the packed results
        if (out_hi[j]) k_wide_join<<<wf_grid(groups, 4), kWfBlock, 0, s>>>(g.out[j], out_hi[j], groups);
    return launch_status();
}
hipError_t launch_wide_sign(const int64_t *lo, int64_t *hi, int64_t n, hipStream_t s) {
    (void)hipGetLastError();
    if (n > 0) k_wide_sign<<<wf_grid(n, 4), kWfBlock, 0, s>>>(lo, hi, n);
    return launch_status();
}
hipError_t launch_wide_fits(const int64_t *lo, const int64_t *hi, const uint64_t *valid, int64_t n, int64_t *flag, hipStream_t s) {
    (void)hipGetLastError();
    if (n > 0) k_wide_fits<<<wf_grid(n, 4), kWfBlock, 0, s>>>(lo, hi, valid, n, flag);
    return launch_status();
}
hipError_t launch_wide_fits_record(const int64_t *rec, const int64_t *hi, int64_t *flag, hipStream_t s) {
    (void)hipGetLastError();
    k_wide_fits_record<<<1, 1, 0, s>>>(rec, hi, flag);
    return launch_status();
}

}  // namespace vdl
