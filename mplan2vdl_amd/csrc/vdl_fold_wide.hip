// vdl_fold_wide.hip -- wide sums in the per-operator folds for gfx950 (vdl_plan_set_wide_sums_tail; DESIGN.md section 5.17 "The tail").
// A translation unit of its own: the kernels of vdl_ops.hip are built from the text they were built from before, and stay the code
// they were.
//
// The split.  Every int64 term is x = H * 2^32 + L with L = x & 0xffffffff and H = x >> 32 (arithmetic).  Over at most 2^31 entries the
// plain int64 sum SH of the H never wraps (|SH| < 2^62), so the exact sum S = SH * 2^32 + SL needs no carry chain and no returning
// atomic while it is accumulated.  The low word of S is the wrapped int64 sum of the terms -- what the plain folds deliver -- and SL,
// which lies in [0, 2^63), is wrapped - (SH << 32) modulo 2^64 exactly.  So a wide fold carries TWO ordinary sums per result, both
// derived from ONE load of the term: the wrapped sum of x and the sum of x >> 32; wide_join_low makes bits 64..127 once per result.
// Order-independent and deterministic, because both sums are.
//
// k_wide_group_fold, k_wide_seg_fold and k_wide_fold_global are the kernels of vdl_ops.hip with the second sum beside the first:
// the same layouts, chunks, segments, carried runs and atomics (read those kernels' comments for why they are laid out as they are).
#include "vdl_device.h"
#include "vdl_kernels.h"

namespace vdl {

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

__device__ __forceinline__ void add_to(int64_t *addr, int64_t v) { atomicAdd((unsigned long long *)addr, (unsigned long long)v); }
__device__ __forceinline__ int64_t wsum(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }

// ---- k_fold_global, FoldSum, wide: per-block partials {sum, first control slot, count, sum of the high halves}, then one block ----
constexpr int kWideFoldBlocks = 2048;
__global__ __launch_bounds__(256) void k_wide_fold_global(Src d, const uint64_t *vd, const uint64_t *vc, int64_t n, int64_t *scratch) {
    constexpr int U = 8;
    const int64_t nw = (n + 63) >> 6;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t wstride = (int64_t)gridDim.x * (blockDim.x / kWave) * U;
    int64_t acc = 0, acch = 0, first = INT64_MAX, cnt = 0;
    by_kind(d.kind, [&](auto kd) {
        for (int64_t w0 = wave_index() * U; w0 < nw; w0 += wstride) {
            int64_t x[U];
            uint64_t mc[U], md[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t w = w0 + u < nw ? w0 + u : nw - 1;
                const int64_t i = (w << 6) + lane;
                x[u] = ldk_stream<decltype(kd)::value>(d, i < n ? i : 0);        // masked lanes read slot 0
                const int64_t rem = n - (w << 6);
                mc[u] = w0 + u < nw ? (rem < 64 ? (1ull << rem) - 1 : ~0ull) : 0ull;
            }
            if (vc) {
#pragma unroll
                for (int u = 0; u < U; u++) mc[u] &= vc[w0 + u < nw ? w0 + u : nw - 1];
            }
#pragma unroll
            for (int u = 0; u < U; u++) md[u] = mc[u];
            if (vd) {
#pragma unroll
                for (int u = 0; u < U; u++) md[u] &= vd[w0 + u < nw ? w0 + u : nw - 1];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t wbase = (w0 + u) << 6;
                if (mc[u] && first == INT64_MAX) first = wbase + __ffsll((long long)mc[u]) - 1;      // words come in ascending order per wave
                cnt += __popcll(md[u]);
                if ((md[u] >> lane) & 1ull) { acc = wsum(acc, x[u]); acch += x[u] >> 32; }         // one load, both sums
            }
        }
    });
    if (lane != 0) { first = INT64_MAX; cnt = 0; }
    __shared__ int64_t red[4][256 / kWave];
    acc = wave_reduce(acc, R_SUM); acch = wave_reduce(acch, R_SUM); first = wave_reduce(first, R_MIN); cnt = wave_reduce(cnt, R_SUM);
    if (lane == 0) { red[0][wave] = acc; red[1][wave] = first; red[2][wave] = cnt; red[3][wave] = acch; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / kWave; w++) { acc = wsum(acc, red[0][w]); first = r_combine(R_MIN, first, red[1][w]); cnt += red[2][w]; acch += red[3][w]; }
        int64_t *o = scratch + 4 * (int64_t)blockIdx.x;
        o[0] = acc; o[1] = first; o[2] = cnt; o[3] = acch;
    }
}
// the record {value, slot, count} as k_fold_global_finish leaves it, and the high word of the value (0 when nothing was folded)
__global__ __launch_bounds__(256) void k_wide_fold_global_finish(const int64_t *scratch, int nblocks, int64_t *result, int64_t *result_hi) {
    int64_t acc = 0, acch = 0, first = INT64_MAX, cnt = 0;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        const int64_t *o = scratch + 4 * (int64_t)b;
        acc = wsum(acc, o[0]); first = r_combine(R_MIN, first, o[1]); cnt += o[2]; acch += o[3];
    }
    __shared__ int64_t red[4][256 / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    acc = wave_reduce(acc, R_SUM); acch = wave_reduce(acch, R_SUM); first = wave_reduce(first, R_MIN); cnt = wave_reduce(cnt, R_SUM);
    if (lane == 0) { red[0][wave] = acc; red[1][wave] = first; red[2][wave] = cnt; red[3][wave] = acch; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / kWave; w++) { acc = wsum(acc, red[0][w]); first = r_combine(R_MIN, first, red[1][w]); cnt += red[2][w]; acch += red[3][w]; }
        int64_t l = 0, h = 0;
        if (cnt > 0) wide_join_low(acc, acch, &l, &h);
        result[0] = acc;
        result[1] = first == INT64_MAX ? -1 : 0;
        result[2] = cnt;
        result[3] = h;                                         // the record's fourth word: one fetch brings value and high word to the host
        result_hi[0] = h;
    }
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
    constexpr int U = kGatherUnroll;
    const int64_t nw = (n + 63) >> 6;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / kWave);
    const int64_t g = wave_index();
    const int64_t per = (nw + nwaves - 1) / nwaves;
    const int64_t w_end = (g + 1) * per < nw ? (g + 1) * per : nw;
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);        // lanes at or before mine
    by_kind(d.kind, [&](auto kd) {
        int64_t carry_h = -1, carry_x = 0, carry_xh = 0;      // wave-uniform: the run still open after the previous word, both sums
        for (int64_t w0 = g * per; w0 < w_end; w0 += U) {
            // the fast path of a long run (see k_seg_fold): 16 (8) whole words that continue the carried run are simply reduced -- both sums
            if (carry_h >= 0 && decltype(kd)::value == SRC_I64 && ((uintptr_t)d.p & 15u) == 0) {
                bool fast = false;
                if (lane < 16) {
                    const int64_t w = w0 + lane;
                    if (w < w_end && ((w + 1) << 6) <= n)
                        fast = heads[w] == 0 && (!vc || vc[w] == ~0ull) && (!vd || vd[w] == ~0ull) && w > 0 && wordhd[w - 1] == carry_h;
                }
                const unsigned fm = (unsigned)(__ballot(fast) & 0xFFFFull);
                const int K = fm == 0xFFFFu ? 16 : (fm & 0xFFu) == 0xFFu ? 8 : 0;
                if (K) {
                    const ll2 *base = (const ll2 *)((const int64_t *)d.p + (w0 << 6)) + lane;
                    ll2 v[8];
                    int64_t t = 0, th = 0;
#pragma unroll
                    for (int j = 0; j < 8; j++) if (j < K / 2) v[j] = base[j * kWave];
#pragma unroll
                    for (int j = 0; j < 8; j++) if (j < K / 2) { t = wsum(t, wsum(v[j].x, v[j].y)); th += ((int64_t)v[j].x >> 32) + ((int64_t)v[j].y >> 32); }
                    carry_x = wsum(carry_x, __shfl(wave_reduce(t, R_SUM), 0, kWave));
                    carry_xh += __shfl(wave_reduce(th, R_SUM), 0, kWave);
                    w0 += K - U;
                    continue;
                }
            }
            uint64_t hw_[U], okw_[U];
            int64_t x_[U], prev_[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int64_t w = w0 + u < w_end ? w0 + u : w_end - 1;
                const int64_t i = (w << 6) + lane;
                hw_[u] = heads[w];
                prev_[u] = w > 0 ? wordhd[w - 1] : -1;
                const int64_t rem = n - (w << 6);
                okw_[u] = rem < 64 ? (1ull << rem) - 1 : ~0ull;
                x_[u] = ldk<decltype(kd)::value>(d, i < n ? i : 0);
            }
            if (vc) {
#pragma unroll
                for (int u = 0; u < U; u++) okw_[u] &= vc[w0 + u < w_end ? w0 + u : w_end - 1];
            }
            if (vd) {
#pragma unroll
                for (int u = 0; u < U; u++) okw_[u] &= vd[w0 + u < w_end ? w0 + u : w_end - 1];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (w0 + u >= w_end) break;                    // wave-uniform
                const int64_t w = w0 + u;
                const uint64_t hw = hw_[u];
                if (hw == 0 && okw_[u] == ~0ull && carry_h >= 0 && prev_[u] == carry_h) {       // the word continues the carried run
                    carry_x = wsum(carry_x, __shfl(wave_reduce(x_[u], R_SUM), 0, kWave));
                    carry_xh += __shfl(wave_reduce(x_[u] >> 32, R_SUM), 0, kWave);
                    continue;
                }
                const uint64_t hm = hw & upto;                 // heads at or before this lane
                const int64_t h = hm ? (w << 6) + 63 - __clzll((long long)hm) : prev_[u];
                const bool ok = ((okw_[u] >> lane) & 1ull) != 0 && h >= 0;
                int64_t x = ok ? x_[u] : 0, xh = ok ? x_[u] >> 32 : 0;      // derived from the one load
                const int64_t hp = __shfl_up(h, 1, kWave);
                const uint64_t okm = __ballot(ok);
                const bool okp = lane > 0 && ((okm >> (lane - 1)) & 1ull);
                const bool starts = lane == 0 || !ok || !okp || hp != h;
                const uint64_t sm = __ballot(starts) & upto;
                const int seg0 = 63 - __clzll((long long)sm);  // first lane of my segment (bit 0 is always set)
#pragma unroll
                for (int off = 1; off < kWave; off <<= 1) {
                    const int64_t y = __shfl_up(x, off, kWave), yh = __shfl_up(xh, off, kWave);
                    if (lane - off >= seg0) { x = wsum(x, y); xh += yh; }
                }
                const int64_t hn = __shfl_down(h, 1, kWave);
                const bool okn = lane < kWave - 1 && ((okm >> (lane + 1)) & 1ull);
                const bool tail = ok && (lane == kWave - 1 || !okn || hn != h);
                bool whole = false;                            // a run that begins and ends inside this word with every slot taking part
                if ((hw >> lane) & 1) {
                    const uint64_t later = lane == kWave - 1 ? 0 : hw >> (lane + 1);
                    if (later) {
                        const int q = lane + __ffsll((long long)later);       // lane of the next head (<= 63)
                        const uint64_t range = (1ull << q) - (1ull << lane);
                        whole = (okm & range) == range;
                    }
                }
                const uint64_t wholem = __ballot(whole);
                const bool mine = tail && ((wholem >> seg0) & 1);              // my segment is such a run
                if (carry_h >= 0) {                            // the carried run: continued in this word's first segment, or written out
                    const bool ok0 = (okm & 1ull) != 0;
                    const int64_t h0 = __shfl(h, 0, kWave);
                    if (ok0 && h0 == carry_h) {
                        if (tail && seg0 == 0) { x = wsum(x, carry_x); xh += carry_xh; }
                    } else if (lane == 0) {
                        add_to(&out[carry_h], carry_x); add_to(&out_hi[carry_h], carry_xh);
                        atomicOr((unsigned long long *)&vout[carry_h >> 6], 1ull << (carry_h & 63));
                    }
                    carry_h = -1;
                }
                if ((okm >> (kWave - 1)) & 1ull) { carry_h = __shfl(h, kWave - 1, kWave); carry_x = __shfl(x, kWave - 1, kWave); carry_xh = __shfl(xh, kWave - 1, kWave); }
                if (mine) {
                    out[h] = x; out_hi[h] = xh;
                } else if (tail && lane != kWave - 1) {
                    add_to(&out[h], x); add_to(&out_hi[h], xh);
                    atomicOr((unsigned long long *)&vout[h >> 6], 1ull << (h & 63));
                }
                if (lane == 0 && wholem) atomicOr((unsigned long long *)&vout[w], wholem);
            }
        }
        if (carry_h >= 0 && lane == 0) {
            add_to(&out[carry_h], carry_x); add_to(&out_hi[carry_h], carry_xh);
            atomicOr((unsigned long long *)&vout[carry_h >> 6], 1ull << (carry_h & 63));
        }
    });
}

// ---- k_group_fold, wide: a FoldSum member with out_hi set folds its chunk twice out of the registers one load filled -- the terms into
// out, their high halves into out_hi.  The LDS stage stays one word per group and 16 KiB: it is RUN TWICE for such a member (the second
// sum's groups pass through it after the first's have been stored), because a doubled stage of 32 KiB would halve the blocks per CU
// for every member of the launch, wide or not, while the second pass costs one more sweep of stores the member needs anyway.
constexpr int kWgK = 8, kWgSplit = 2, kWgWords = 64;        // kGroupK, kGroupSplit, kCompactWords of vdl_ops.hip
template <int NF>
__global__ __launch_bounds__(256) void k_wide_group_fold(WideGroupFoldArgs A, unsigned vec16, const uint64_t *heads, int64_t m, const int64_t *offsets) {
    __shared__ int wprefix[kWgWords];
    __shared__ uint64_t wmask[kWgWords];
    __shared__ int64_t stage[256 / kWave][kWave * kWgK];                   // per wave: the results of its groups, by group
    constexpr int K = kWgK, NW = 256 / kWave, WW = kWave * K / 64;
    static_assert(kWgWords == kWgSplit * NW * WW, "a block's waves cover its share of the tile");
    const GroupFoldArgs &a = A.g;
    const int64_t nw = (m + 63) >> 6;
    const int64_t tile = blockIdx.x / kWgSplit;
    const int part = blockIdx.x % kWgSplit;
    const int64_t w0 = tile * kWgWords;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    if (tid < kWgWords) {
        const int64_t w = w0 + tid;
        const uint64_t hm = w < nw ? heads[w] : 0ull;
        wmask[tid] = hm;
        const int cnt = __popcll(hm);
        int incl = cnt;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) { const int y = __shfl_up(incl, off, kWave); if (lane >= off) incl += y; }
        wprefix[tid] = incl - cnt;
    }
    __syncthreads();
    const int wfirst = part * (NW * WW) + wave * WW;
    if (((w0 + wfirst) << 6) >= m) return;                         // wave-uniform; no barrier below
    const int64_t e0 = ((w0 + wfirst) << 6) + (int64_t)lane * K;
    const int nv = m - e0 >= K ? K : (m - e0 > 0 ? (int)(m - e0) : 0);
    const unsigned hb = (unsigned)(wmask[wfirst + (lane >> 3)] >> ((lane & 7) * 8)) & 0xffu;
    const int c = __popc(hb);
    int incl = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) { const int y = __shfl_up(incl, off, kWave); if (lane >= off) incl += y; }
    const int64_t B = offsets[tile] + wprefix[wfirst] + (incl - c);
    const int64_t Bw = offsets[tile] + wprefix[wfirst];
    const int ngw = __shfl(incl, kWave - 1, kWave);
    const uint64_t headlanes = __ballot(c != 0);
    const uint64_t below = (1ull << lane) - 1;
    const uint64_t starts = (headlanes << 1) | 1ull;
    const int seg0 = 63 - __clzll((long long)(starts & (below | (1ull << lane))));
    const bool first_head_lane = c != 0 && (headlanes & below) == 0;
    const uint64_t later = lane == kWave - 1 ? 0ull : headlanes >> (lane + 1);
    const int next_head = later ? lane + __ffsll((long long)later) : -1;
    const int fetch_from = next_head >= 0 ? next_head : kWave - 1;
    auto flush = [&](int64_t *out, int upto_groups) {              // the groups staged by this wave, stored by consecutive lanes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < upto_groups; k += kWave) out[Bw + k] = stage[wave][k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
    };
#pragma unroll
    for (int j0 = 0; j0 < kMaxGroupFolds; j0 += NF) {
        if (j0 >= a.nfold) break;                              // wave-uniform
        int64_t x[NF][K];
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (j0 + f >= a.nfold) break;
            const Src d = a.data[j0 + f];
            if (a.kind[j0 + f] == 3) {
#pragma unroll
                for (int j = 0; j < K; j++) x[f][j] = 1;
            } else if (((vec16 >> (j0 + f)) & 1u) && nv == K) {
                const ll2 *q = (const ll2 *)((const int64_t *)d.p + e0);
#pragma unroll
                for (int j = 0; j < K; j += 2) { const ll2 t = q[j >> 1]; x[f][j] = t.x; x[f][j + 1] = t.y; }
            } else {
#pragma unroll
                for (int j = 0; j < K; j++) x[f][j] = ld(d, j < nv ? e0 + j : (e0 < m ? e0 : 0));
            }
        }
#pragma unroll
        for (int f = 0; f < NF; f++) {
            if (j0 + f >= a.nfold) break;
            const int kind = a.kind[j0 + f];
            if (kind == 4) {                                   // FoldChoose: the first value of every run
                int64_t g = B - 1;
#pragma unroll
                for (int j = 0; j < K; j++)
                    if ((hb >> j) & 1u) { g++; stage[wave][g - Bw] = x[f][j]; }
                flush(a.out[j0 + f], ngw);
                continue;
            }
            const int rk = kind == 1 ? R_MIN : kind == 2 ? R_MAX : R_SUM;
            int64_t *const out_hi = A.out_hi[j0 + f];
            const int passes = kind == 0 && out_hi ? 2 : 1;    // wave-uniform
            for (int pass = 0; pass < passes; pass++) {
                int64_t *out = pass ? out_hi : a.out[j0 + f];
                if (pass) {                                    // the second sum, out of the same registers
#pragma unroll
                    for (int j = 0; j < K; j++) x[f][j] >>= 32;
                }
                by_reduction(rk, [&](auto rc) {
                    constexpr int R = decltype(rc)::value;
                    int64_t acc = r_identity(R), pre = r_identity(R), g = B - 1;
                    bool started = false;
#pragma unroll
                    for (int j = 0; j < K; j++) {
                        if ((hb >> j) & 1u) {
                            if (started) stage[wave][g - Bw] = acc; else pre = acc;
                            g++; acc = x[f][j]; started = true;
                        } else if (j < nv) {
                            acc = r_combine(R, acc, x[f][j]);
                        }
                    }
                    const int64_t tail = started ? acc : r_identity(R);
                    int64_t S = started ? pre : acc;
#pragma unroll
                    for (int off = 1; off < kWave; off <<= 1) {
                        const int64_t y = __shfl_up(S, off, kWave);
                        if (lane - off >= seg0) S = r_combine(R, S, y);
                    }
                    const int64_t cont = __shfl(S, fetch_from, kWave);
                    auto combine = [&](int64_t *addr, int64_t v) {
                        if (R == R_SUM) add_to(addr, v);
                        else if (R == R_MIN) atomicMin((long long *)addr, (long long)v);
                        else atomicMax((long long *)addr, (long long)v);
                    };
                    if (c != 0) {
                        if (next_head >= 0) stage[wave][g - Bw] = r_combine(R, tail, cont);
                        else combine(&out[g], lane == kWave - 1 ? tail : r_combine(R, tail, cont));
                        if (first_head_lane && B > 0) combine(&out[B - 1], S);
                    } else if (headlanes == 0 && lane == kWave - 1 && B > 0) {
                        combine(&out[B - 1], S);
                    }
                });
                flush(out, ngw - 1);
            }
        }
    }
}

int wf_grid(int64_t n, int per_lane) { return grid_for(n, kWfBlock, per_lane); }

}  // namespace

int wide_fold_scratch_blocks() { return kWideFoldBlocks; }
hipError_t launch_wide_fold_global(Src d, const uint64_t *vd, const uint64_t *vc, int64_t n, int64_t *scratch, int64_t *result, int64_t *result_hi, hipStream_t s) {
    (void)hipGetLastError();
    int grid = grid_for(n, 256, 8);
    if (grid > kWideFoldBlocks) grid = kWideFoldBlocks;
    k_wide_fold_global<<<grid, 256, 0, s>>>(d, vd, vc, n, scratch);
    k_wide_fold_global_finish<<<1, 256, 0, s>>>(scratch, grid, result, result_hi);
    return launch_status();
}
hipError_t launch_wide_fold_runs(Src d, const uint64_t *vd, const uint64_t *vc, const uint64_t *heads, const int64_t *wordhd, int64_t n, int64_t *out, int64_t *out_hi,
                                 uint64_t *vout, hipStream_t s) {
    (void)hipGetLastError();
    if (n <= 0) return hipSuccess;
    const int64_t nw = (n + 63) >> 6;
    int64_t g = (nw + 15) / 16;                      // as k_seg_fold is launched: a few thousand waves with a contiguous chunk of words each
    if (g > 2048) g = 2048;
    k_wide_init_heads<<<grid_for(nw, 256, 1), 256, 0, s>>>(heads, nw, out, out_hi);
    k_wide_seg_fold<<<(int)(g < 1 ? 1 : g), 256, 0, s>>>(d, vd, vc, heads, wordhd, n, out, out_hi, vout);
    k_wide_join_heads<<<grid_for(nw, 256, 1), 256, 0, s>>>(heads, nw, out, out_hi);
    return launch_status();
}
hipError_t launch_wide_group_fold(const WideGroupFoldArgs &a, const uint64_t *heads, int64_t m, const int64_t *offsets, hipStream_t s) {
    (void)hipGetLastError();
    const int64_t nb = (m + (int64_t)kWgWords * 64 - 1) / ((int64_t)kWgWords * 64);
    if (nb <= 0 || a.g.nfold <= 0) return hipSuccess;
    if (a.g.nfold > kMaxGroupFolds) return hipErrorInvalidValue;
    if (compact_tile() != (int64_t)kWgWords * 64) return hipErrorInvalidValue;      // heads / offsets are laid out per compaction tile of vdl_ops.hip
    unsigned vec16 = 0;
    for (int f = 0; f < a.g.nfold; f++)
        if (a.g.data[f].kind == SRC_I64 && ((uintptr_t)a.g.data[f].p & 15u) == 0) vec16 |= 1u << f;
    if (a.g.nfold <= 2) k_wide_group_fold<2><<<(int)(nb * kWgSplit), 256, 0, s>>>(a, vec16, heads, m, offsets);
    else k_wide_group_fold<4><<<(int)(nb * kWgSplit), 256, 0, s>>>(a, vec16, heads, m, offsets);
    return launch_status();
}
hipError_t launch_wide_join(const int64_t *lo, int64_t *hi, int64_t n, hipStream_t s) {
    (void)hipGetLastError();
    if (n > 0) k_wide_join<<<wf_grid(n, 4), kWfBlock, 0, s>>>(lo, hi, n);
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
