// vdl_fold_body.h -- the bodies of the segmented fold and of the global fold's finish step for gfx950, each written once and compiled
// twice: plain (WIDE = false) into the kernels of vdl_ops.hip, and with a second sum beside the first (WIDE = true; DESIGN.md section
// 5.17 "The tail") into the k_wide_* kernels of vdl_fold_wide.hip, a translation unit of its own -- as vdl_mscan_body.h is compiled by
// vdl_mscan.hip and vdl_mscan_wide.hip.  Also what the two files share of the other two fold kernels, k_fold_global and k_group_fold,
// whose texts are vdl_fold_global.inc and vdl_group_fold.inc (they say why they are no function templates).
//
// What WIDE means.  The fold is a FoldSum: `kind` is the constant 0, so by_reduction folds to R_SUM alone.  Beside every wrapped sum goes
// the sum of the terms' `>> 32`, derived from the same load (vdl_fold_wide.hip says why these two sums give the exact 128-bit one).
// Everything the second sum needs sits under `if constexpr (WIDE)` or in values that are constants when WIDE is false: the plain
// instantiations contain nothing of it.
#pragma once
#include "vdl_device.h"
#include "vdl_kernels.h"

namespace vdl {

constexpr int kFoldBlocks = 2048;                          // blocks of a global fold at most: what its callers' scratch holds
constexpr int kCompactWords = 64;                          // head words per compaction tile (4096 entries)
constexpr int kGroupK = 8, kGroupSplit = 2;                // k_group_fold: entries per lane, blocks per compaction tile

__device__ __forceinline__ void atomic_combine(int rk, int64_t *addr, int64_t v) {
    if (rk == R_SUM) atomicAdd((unsigned long long *)addr, (unsigned long long)v);
    else if (rk == R_MIN) atomicMin((long long *)addr, (long long)v);
    else atomicMax((long long *)addr, (long long)v);
}

// ---- the global (single-run) fold: per-block partials {value, first control slot, count} -- in a wide fold four words, the sum of the
// high halves fourth -- then one block.  kind: 0 sum, 1 min, 2 max, 3 count, 4 choose
static inline int fold_global_grid(int64_t n) {
    const int grid = grid_for(n, 256, 8);
    return grid > kFoldBlocks ? kFoldBlocks : grid;
}
// the record {value, slot, count}; a wide fold adds the high word of the value (0 when nothing was folded) as the record's fourth word
// -- one fetch brings value and high word to the host -- and as result_hi[0]
template <bool WIDE>
__device__ __forceinline__ void fold_global_finish_body(int kind_rt, Src d, const int64_t *scratch, int nblocks, int64_t *result, int64_t *result_hi) {
    constexpr int W = WIDE ? 4 : 3;
    const int kind = WIDE ? 0 : kind_rt;
    const int rk = kind == 1 ? R_MIN : kind == 2 ? R_MAX : R_SUM;
    const int ak = kind == 4 ? R_MIN : rk;
    int64_t acc = kind == 4 ? INT64_MAX : r_identity(rk), first = INT64_MAX, cnt = 0;
    [[maybe_unused]] int64_t acch = 0;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        acc = r_combine(ak, acc, scratch[W * (int64_t)b]);
        first = r_combine(R_MIN, first, scratch[W * (int64_t)b + 1]);
        cnt += scratch[W * (int64_t)b + 2];
        if constexpr (WIDE) acch += scratch[W * (int64_t)b + 3];
    }
    __shared__ int64_t red[W][256 / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    acc = wave_reduce(acc, ak); first = wave_reduce(first, R_MIN); cnt = wave_reduce(cnt, R_SUM);
    if constexpr (WIDE) acch = wave_reduce(acch, R_SUM);
    if (lane == 0) {
        red[0][wave] = acc; red[1][wave] = first; red[2][wave] = cnt;
        if constexpr (WIDE) red[3][wave] = acch;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / kWave; w++) {
            acc = r_combine(ak, acc, red[0][w]); first = r_combine(R_MIN, first, red[1][w]); cnt += red[2][w];
            if constexpr (WIDE) acch += red[3][w];
        }
        if (kind == 4) acc = cnt > 0 ? ld(d, acc) : 0;     // FoldChoose: the first datum of the run
        result[0] = acc;
        result[1] = first == INT64_MAX ? -1 : 0;     // the first (here: only) run of a vector starts at slot 0, whatever EPS slots precede its first member
        result[2] = cnt;
        if constexpr (WIDE) {
            int64_t l = 0, h = 0;
            if (cnt > 0) wide_join_low(acc, acch, &l, &h);
            result[3] = h;
            result_hi[0] = h;
        }
    }
}

// ---- the segmented fold: out[head] = the fold of the run that begins at `head`; in a wide fold the wrapped sum, and out_hi[head] =
// the sum of the run's high halves (joined afterwards) ----
static inline int seg_fold_grid(int64_t n) {     // a few thousand waves, each with a contiguous chunk of at least a few words
    const int64_t nw = (n + 63) >> 6;
    int64_t g = (nw + 15) / 16;                  // >= 4 words per wave (4 waves per block)
    if (g > 2048) g = 2048;
    return (int)(g < 1 ? 1 : g);
}
// kind: 0 sum, 1 min, 2 max, 3 count, 4 choose-pass (min over slot index of the data)
// Each wave walks a contiguous chunk of words and carries the value of the run that is open at a word's last lane
// into the next word, so a run costs one atomic per wave it touches instead of one per 64 slots: with few long runs
// (dense GROUP BY domains) the per-word atomics all landed on the same handful of addresses and serialised.
template <bool WIDE>
__device__ __forceinline__ void seg_fold_body(int kind_rt, Src d, const uint64_t *vd, const uint64_t *vc, const uint64_t *heads, const int64_t *wordhd, int64_t n,
                                              int64_t *out, int64_t *out_hi, uint64_t *vout) {
    constexpr int U = kGatherUnroll;
    const int kind = WIDE ? 0 : kind_rt;
    const int rk_rt = (kind == 1 || kind == 4) ? R_MIN : kind == 2 ? R_MAX : R_SUM;
    const int64_t nw = (n + 63) >> 6;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x / kWave);
    const int64_t g = wave_index();
    const int64_t per = (nw + nwaves - 1) / nwaves;
    const int64_t w_end = (g + 1) * per < nw ? (g + 1) * per : nw;
    const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);        // lanes at or before mine
    by_kind(d.kind, [&](auto kd) { by_reduction(rk_rt, [&](auto rc) {
        constexpr int rk = decltype(rc)::value;
        int64_t carry_h = -1, carry_x = r_identity(rk);       // wave-uniform: the run still open after the previous word
        [[maybe_unused]] int64_t carry_xh = 0;                // ... and the sum of its high halves
        auto put_carry = [&]() {                              // lane 0 writes the carried run out
            atomic_combine(rk, &out[carry_h], carry_x);
            if constexpr (WIDE) atomic_combine(R_SUM, &out_hi[carry_h], carry_xh);
            atomicOr((unsigned long long *)&vout[carry_h >> 6], 1ull << (carry_h & 63));
        };
        for (int64_t w0 = g * per; w0 < w_end; w0 += U) {
            // A long run (a dense-domain GROUP BY has a handful over millions of slots): while the next 16 (or 8) words begin no
            // run, hold a value in every slot and continue the run this wave carries, their 1024 (512) values are simply reduced --
            // lanes 0..15 look one word each, then every lane loads 16 (8) consecutive values with 16-byte loads: 8 (4) KB per wave
            // in flight instead of the 2 KB of the word-by-word path below, whose lane = slot layout the segments need
            // (60 M rows in 32 runs: 175 -> ~110 us).
            if (carry_h >= 0 && (kind >= 3 || (decltype(kd)::value == SRC_I64 && ((uintptr_t)d.p & 15u) == 0))) {
                bool fast = false;
                if (lane < 16) {
                    const int64_t w = w0 + lane;
                    if (w < w_end && ((w + 1) << 6) <= n)
                        fast = heads[w] == 0 && (!vc || vc[w] == ~0ull) && (!vd || vd[w] == ~0ull) && w > 0 && wordhd[w - 1] == carry_h;
                }
                const unsigned fm = (unsigned)(__ballot(fast) & 0xFFFFull);
                const int K = fm == 0xFFFFu ? 16 : (fm & 0xFFu) == 0xFFu ? 8 : 0;
                if (K) {
                    int64_t t = r_identity(rk);
                    if (kind < 3) {
                        const ll2 *base = (const ll2 *)((const int64_t *)d.p + (w0 << 6)) + lane;
                        ll2 v[8];
#pragma unroll
                        for (int j = 0; j < 8; j++) if (j < K / 2) v[j] = base[j * kWave];
#pragma unroll
                        for (int j = 0; j < 8; j++) if (j < K / 2) t = r_combine(rk, t, r_combine(rk, v[j].x, v[j].y));
                        t = __shfl(wave_reduce(t, rk), 0, kWave);
                        if constexpr (WIDE) {
                            int64_t th = 0;
#pragma unroll
                            for (int j = 0; j < 8; j++) if (j < K / 2) th += ((int64_t)v[j].x >> 32) + ((int64_t)v[j].y >> 32);
                            carry_xh += __shfl(wave_reduce(th, R_SUM), 0, kWave);
                        }
                    } else t = kind == 3 ? (int64_t)K * 64 : (w0 << 6);
                    carry_x = r_combine(rk, carry_x, t);
                    w0 += K - U;
                    continue;
                }
            }
            // operands of U words first (the words of a wave are processed in order: the carried run links them)
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
                x_[u] = kind < 3 ? ldk<decltype(kd)::value>(d, i < n ? i : 0) : (kind == 3 ? 1 : i);
            }
            if (vc) {
                uint64_t t[U];
#pragma unroll
                for (int u = 0; u < U; u++) t[u] = vc[w0 + u < w_end ? w0 + u : w_end - 1];
#pragma unroll
                for (int u = 0; u < U; u++) okw_[u] &= t[u];
            }
            if (vd) {
                uint64_t t[U];
#pragma unroll
                for (int u = 0; u < U; u++) t[u] = vd[w0 + u < w_end ? w0 + u : w_end - 1];
#pragma unroll
                for (int u = 0; u < U; u++) okw_[u] &= t[u];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (w0 + u >= w_end) break;                    // wave-uniform
                const int64_t w = w0 + u;
                const uint64_t hw = hw_[u];
                if (hw == 0 && okw_[u] == ~0ull && carry_h >= 0 && prev_[u] == carry_h) {
                    // no run begins in this word and all 64 slots take part: the word continues the run the wave carries (long
                    // runs -- a dense-domain GROUP BY has a handful -- are nearly all such words): one wave reduction, no segments
                    carry_x = r_combine(rk, carry_x, __shfl(wave_reduce(x_[u], rk), 0, kWave));
                    if constexpr (WIDE) carry_xh += __shfl(wave_reduce(x_[u] >> 32, R_SUM), 0, kWave);
                    continue;
                }
                const uint64_t hm = hw & upto;                 // heads at or before this lane
                const int64_t h = hm ? (w << 6) + 63 - __clzll((long long)hm) : prev_[u];
                const bool ok = ((okw_[u] >> lane) & 1ull) != 0 && h >= 0;
                int64_t x = ok ? x_[u] : r_identity(rk);
                [[maybe_unused]] int64_t xh = ok ? x_[u] >> 32 : 0;          // derived from the one load
                // lane segments = maximal stretches of consecutive active lanes with one head; an EPS slot
                // inside a run splits it into several segments, each adds its part to the same out[h]
                const int64_t hp = __shfl_up(h, 1, kWave);
                const uint64_t okm = __ballot(ok);
                const bool okp = lane > 0 && ((okm >> (lane - 1)) & 1ull);
                const bool starts = lane == 0 || !ok || !okp || hp != h;
                const uint64_t sm = __ballot(starts) & upto;
                const int seg0 = 63 - __clzll((long long)sm);  // first lane of my segment (bit 0 is always set)
#pragma unroll
                for (int off = 1; off < kWave; off <<= 1) {
                    const int64_t y = __shfl_up(x, off, kWave);
                    if (lane - off >= seg0) x = r_combine(rk, x, y);
                    if constexpr (WIDE) {
                        const int64_t yh = __shfl_up(xh, off, kWave);
                        if (lane - off >= seg0) xh += yh;
                    }
                }
                const int64_t hn = __shfl_down(h, 1, kWave);
                const bool okn = lane < kWave - 1 && ((okm >> (lane + 1)) & 1ull);
                const bool tail = ok && (lane == kWave - 1 || !okn || hn != h);
                // runs that begin and end inside this word with every slot taking part are one segment nobody else adds
                // to: a plain store and one validity update per word (a sparse GROUP BY has ~30 such runs per word,
                // and their atomics on out[] and on the same word of vout[] were most of the kernel)
                bool whole = false;
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
                // the run carried over from the previous word: continue it in this word's first segment, or write it out
                if (carry_h >= 0) {
                    const bool ok0 = (okm & 1ull) != 0;
                    const int64_t h0 = __shfl(h, 0, kWave);
                    if (ok0 && h0 == carry_h) {
                        if (tail && seg0 == 0) {
                            x = r_combine(rk, x, carry_x);
                            if constexpr (WIDE) xh += carry_xh;
                        }
                    } else if (lane == 0) {
                        put_carry();
                    }
                    carry_h = -1;
                }
                if ((okm >> (kWave - 1)) & 1ull) {             // lane 63 is that segment's tail
                    carry_h = __shfl(h, kWave - 1, kWave); carry_x = __shfl(x, kWave - 1, kWave);
                    if constexpr (WIDE) carry_xh = __shfl(xh, kWave - 1, kWave);
                }
                if (mine) {
                    out[h] = x;
                    if constexpr (WIDE) out_hi[h] = xh;
                } else if (tail && lane != kWave - 1) {
                    atomic_combine(rk, &out[h], x);
                    if constexpr (WIDE) atomic_combine(R_SUM, &out_hi[h], xh);
                    atomicOr((unsigned long long *)&vout[h >> 6], 1ull << (h & 63));
                }
                if (lane == 0 && wholem) atomicOr((unsigned long long *)&vout[w], wholem);   // runs from other words may set bits here too
            }
        }
        if (carry_h >= 0 && lane == 0) put_carry();
    }); });
}

// ---- every fold of one GROUP BY in one launch: the kernel's text is vdl_group_fold.inc, which says why it is no function template ----
// vec16 bit f: fold f's data is int64 at a 16-byte aligned address
static inline unsigned group_fold_vec16(const GroupFoldArgs &a) {
    unsigned vec16 = 0;
    for (int f = 0; f < a.nfold; f++)
        if (a.data[f].kind == SRC_I64 && ((uintptr_t)a.data[f].p & 15u) == 0) vec16 |= 1u << f;
    return vec16;
}

}  // namespace vdl
