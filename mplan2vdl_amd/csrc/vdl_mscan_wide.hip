// vdl_mscan_wide.hip -- the WIDE-SUMS build of the multi-aggregate fused scans for gfx950 (vdl_plan_set_wide_sums; DESIGN.md section
// 5.17): the body of vdl_mscan_body.h compiled with VDL_WIDE, shape for shape the instantiations of vdl_mscan.hip, and the finish
// step that folds the blocks' (lo, hi) pairs with carry.  A translation unit of its own: the kernels of vdl_mscan.hip are built from
// the text they were built from before, and stay the code they were.
//
// Every SUM accumulator is a pair (lo: bits 0..63, hi: bits 64..127) of the exact two's-complement sum of the per-row int64 terms; lo
// is the word the plain kernels deliver.  Counts, MIN, MAX and FIRST stay one word; the finish step writes their sign extension.
#define VDL_WIDE 1
#include "vdl_kernels.h"
#include "vdl_mscan_body.h"
#include "vdl_mscan_variants.h"

namespace vdl {

namespace {

template <int NC, int U, bool VEC, bool NT, bool GROUPED, bool DER>
__global__ __launch_bounds__(kMsBlock) void k_mscan_wide(const MsArgs C, const MScanDesc *__restrict__ Dp) {
    mscan_body<NC, U, VEC, NT, GROUPED, DER>(C, C, *Dp, *Dp);
}

// out[w] = fold over blocks of partials[b][w], out_hi[w] = its bits 64..127: one wave per word, lanes stride over the blocks (the order
// of the fold is fixed: deterministic, as k_mscan_finish).  A SUM aggregate's word is folded as a pair, with carry, from the block's
// word and its high word behind the block's table; every other word as before, its high word the sign extension.
__global__ __launch_bounds__(256) void k_mscan_finish_wide(const MScanDesc *__restrict__ Dp, int nblocks, int grouped, int64_t *out, int64_t *out_hi) {
    const MScanDesc &D = *Dp;
    const int W = D.nagg + 1;
    const int nsum = wide_nsum(D, D.nagg);
    const int64_t words = grouped ? D.pcount * W + 1 : W;
    const int64_t stride = grouped ? words + D.pcount * nsum : words + nsum;      // one block's partials
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    if (i >= words) return;
    int rk = R_SUM, w = 0;
    if (!(grouped && i == words - 1)) {
        w = (int)(i % W);
        rk = w == 0 ? R_SUM : rk_of(D.agg[w - 1].kind);
    }
    if (w > 0 && rk == R_SUM) {
        const int64_t hi_at = (grouped ? words + (i / W) * nsum : words) + wide_nsum(D, w - 1);
        uint64_t lo = 0, hi = 0;
        for (int b = lane; b < nblocks; b += kWave) wide_add(lo, hi, (uint64_t)D.block_partials[(int64_t)b * stride + i], (uint64_t)D.block_partials[(int64_t)b * stride + hi_at]);
        wide_wave_reduce(lo, hi);
        if (lane == 0) { out[i] = (int64_t)lo; out_hi[i] = (int64_t)hi; }
        return;
    }
    int64_t x = r_identity(rk);
    for (int b = lane; b < nblocks; b += kWave) x = r_combine(rk, x, D.block_partials[(int64_t)b * stride + i]);
    x = wave_reduce(x, rk);
    if (lane == 0) { out[i] = x; out_hi[i] = x >> 63; }
}

// The merge of the ranks' gathered partial words of a sharded wide run (vdl_comm.cpp): one lane per word, merge_word_wide of
// vdl_kernels.h; the status as k_merge_words leaves it.  A few hundred words: a latency kernel.
__global__ __launch_bounds__(256) void k_merge_words_wide(const int64_t *__restrict__ g, int world, int64_t n_words, int64_t stride, const int32_t *__restrict__ ops,
                                                          int64_t *out, int64_t *out_hi, int64_t *status_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) {
        int64_t hi = 0;
        out[i] = merge_word_wide(g, world, n_words, ops[i], i, stride, &hi);
        out_hi[i] = hi;
    }
    if (i == 0 && status_out) {
        int64_t st = 0, who = -1;
        for (int r = world - 1; r >= 0; r--) {
            const int64_t x = g[(int64_t)r * stride + 2 * n_words];
            if (x != 0) { st = x; who = r; }
        }
        status_out[0] = st; status_out[1] = who;
    }
}

typedef void (*mscan_fn)(const MsArgs, const MScanDesc *);
#define VDL_MS(NC, U, VEC, NT, GR) k_mscan_wide<NC, U, VEC, NT, GR, false>
#define VDL_MSJ(NC, U, VEC, NT, GR) k_mscan_wide<NC, U, VEC, NT, GR, true>
const mscan_fn kMsWide[] = { VDL_MS_VARIANTS(VDL_MS, VDL_MSJ) };
#undef VDL_MS
#undef VDL_MSJ
constexpr int kNumMsWide = sizeof(kMsWide) / sizeof(kMsWide[0]);

}  // namespace

const void *mscan_wide_fn(int variant) { return variant >= 0 && variant < kNumMsWide ? (const void *)kMsWide[variant] : nullptr; }

hipError_t launch_mscan_wide_kernel(int variant, int grid, int block, size_t lds_bytes, hipStream_t s, const MsArgs &a, const MScanDesc *dev_desc) {
    if (variant < 0 || variant >= kNumMsWide || grid < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kMsWide[variant], dim3(grid), dim3(block), lds_bytes, s, a, dev_desc);
    return hipGetLastError();
}

hipError_t launch_mscan_finish_wide(const MScanDesc &d, const MScanDesc *dev_desc, int nblocks, bool grouped, int64_t *out, int64_t *out_hi, hipStream_t s) {
    if (!out || !out_hi) return hipErrorInvalidValue;
    const int64_t words = grouped ? d.pcount * (d.nagg + 1) + 1 : d.nagg + 1;
    k_mscan_finish_wide<<<(int)((words + 3) / 4), 256, 0, s>>>(dev_desc, nblocks, grouped ? 1 : 0, out, out_hi);
    return hipGetLastError();
}

hipError_t launch_merge_words_wide(const int64_t *gathered, int world, int64_t n_words, int64_t stride, const int32_t *ops, int64_t *out,
                                   int64_t *out_hi, int64_t *status_out, hipStream_t s) {
    (void)hipGetLastError();
    if (world < 1 || n_words < 0 || stride < 3 * n_words + 1 || !gathered || (n_words && (!ops || !out || !out_hi))) return hipErrorInvalidValue;
    if (n_words == 0 && !status_out) return hipSuccess;
    const int64_t lanes = n_words > 0 ? n_words : 1;
    k_merge_words_wide<<<(int)((lanes + 255) / 256), 256, 0, s>>>(gathered, world, n_words, stride, ops, out, out_hi, status_out);
    return hipGetLastError();
}

}  // namespace vdl
